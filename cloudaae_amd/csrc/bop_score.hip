// bop_score.hip -- the device side of BOP's pose errors: the pixel counts behind the visible surface discrepancy (VSD)
// and the symmetry-aware maximum distances MSSD and MSPD.  DESIGN.md, "BOP pose errors (VSD, MSSD, MSPD)", is the
// definition; tests/bop_score_reference.py restates it in NumPy.  All floating point is fp64 on exactly widened inputs,
// un-fused (the file is compiled with -ffp-contract=off), with the correctly rounded / and sqrt; every result of
// cloudaae_vsd_counts is an integer, and the maxima and minima of cloudaae_pose_max_dist are exact, so nothing depends
// on the order of execution, the batch or the run.
//
//   cloudaae_vsd_counts      four memsets and one launch.  A workgroup of 256 threads takes 2048 pixels of one sample,
//                            eight per thread: the distance factor m, D(dt), D(dg) and vis_g of a pixel are computed once
//                            and kept in registers, then every pose of the sample is read against them.  A predicate is
//                            counted by ballot + popcount per wave, the four waves meet in LDS, and one integer atomic per
//                            workgroup and counter (none for a zero) adds into the zeroed outputs.
//   cloudaae_pose_max_dist   a memset and two launches.  grid = (blocks of 128 points) x poses x samples: one (sample,
//                            pose) is spread over ceil(m / 128) workgroups.  A lane transforms its point under the
//                            estimate once and under every G S_s in turn; the squared distances meet as integer maxima
//                            on the bit pattern of the non-negative double (wave, LDS, one atomic per workgroup, symmetry
//                            and error); a second launch takes the minimum over the symmetries and the square root.
#include "common.h"
#include "depth_frame.h"
#include "pose_math.h"
#include "../../include/cloudaae_hip.h"

#include <limits.h>
#include <math.h>

namespace cloudaae {

typedef unsigned long long u64;

constexpr int VS_BLOCK = 256;
constexpr int VS_WAVES = VS_BLOCK / 64;
constexpr int VS_PIX = 8;                          // pixels of a thread
constexpr int VS_TILE = VS_BLOCK * VS_PIX;         // pixels of a workgroup
constexpr int VS_MAX_K = 16;                       // thresholds tau of a call (a choice: they live in registers)
constexpr int VS_SLOTS = 3 + VS_MAX_K;             // inter, union, visib_gt, over[k]

struct VsdArgs {
    int f, h, w, b, p, k, tiles;
    const unsigned short *depth_test, *depth_gt, *depth_est;
    const float *intrinsics;
    const int *frame_of;
    double delta;
    const double *tau;
    int *inter, *uni, *over, *visib_gt;
};

__global__ __launch_bounds__(VS_BLOCK) void vsd_counts_kernel(VsdArgs a)
{
    __shared__ int red[VS_WAVES][VS_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f)                       // (the whole workgroup: no barrier has been reached)
        return;
    const float *kk = a.intrinsics + 5 * (size_t)fr;
    const double fx = (double)kk[0], fy = (double)kk[1], cx = (double)kk[2], cy = (double)kk[3], factor = (double)kk[4];
    const int hw = a.h * a.w;
    const unsigned short *dt = a.depth_test + (size_t)fr * hw;
    const unsigned short *dg = a.depth_gt + (size_t)s * hw;
    const int first = tile * VS_TILE + tid;

    // once per pixel: m, D(dt), D(dg), valid_t, vis_g
    double m[VS_PIX], Dt[VS_PIX], Dg[VS_PIX];
    unsigned inside = 0, valid_t = 0, vis_g = 0;
    int n_vis = 0;
#pragma unroll
    for (int i = 0; i < VS_PIX; ++i) {
        const int pix = first + i * VS_BLOCK;
        m[i] = Dt[i] = Dg[i] = 0.0;
        bool vg = false;
        if (pix < hw) {
            const int u = pix % a.w, v = pix / a.w;
            const double xn = ((double)u - cx) / fx, yn = ((double)v - cy) / fy;
            m[i] = sqrt((xn * xn + yn * yn) + 1.0);
            const unsigned short t = dt[pix], g = dg[pix];
            Dt[i] = ((double)t / factor) * m[i];
            Dg[i] = ((double)g / factor) * m[i];
            const bool vt = t != 0;
            vg = g != 0 && (!vt || Dg[i] - Dt[i] <= a.delta);
            inside |= 1u << i;
            valid_t |= (unsigned)vt << i;
            vis_g |= (unsigned)vg << i;
        }
        n_vis += wave_count(vg);
    }

    double tau[VS_MAX_K];
#pragma unroll
    for (int k = 0; k < VS_MAX_K; ++k)
        tau[k] = k < a.k ? a.tau[(size_t)s * a.k + k] : 0.0;

    for (int p = 0; p < a.p; ++p) {
        const unsigned short *de = a.depth_est + ((size_t)s * a.p + p) * hw;
        int n_inter = 0, n_union = 0, n_over[VS_MAX_K];
#pragma unroll
        for (int k = 0; k < VS_MAX_K; ++k)
            n_over[k] = 0;
#pragma unroll
        for (int i = 0; i < VS_PIX; ++i) {
            const bool vg = (vis_g >> i) & 1u;
            bool ve = false;
            double diff = 0.0;
            if ((inside >> i) & 1u) {
                const unsigned short e = de[first + i * VS_BLOCK];
                const double De = ((double)e / factor) * m[i];
                ve = e != 0 && (!((valid_t >> i) & 1u) || De - Dt[i] <= a.delta || vg);
                diff = fabs(Dg[i] - De);
            }
            const bool both = vg && ve;
            const u64 both_mask = __builtin_amdgcn_ballot_w64(both);
            n_inter += __builtin_popcountll(both_mask);
            n_union += wave_count(vg || ve);
            if (both_mask) {                       // (wave-uniform)
#pragma unroll
                for (int k = 0; k < VS_MAX_K; ++k)
                    if (k < a.k)
                        n_over[k] += wave_count(both && diff >= tau[k]);
            }
        }
        if (lane == 0) {
            red[wv][0] = n_inter;
            red[wv][1] = n_union;
            red[wv][2] = p == 0 ? n_vis : 0;
#pragma unroll
            for (int k = 0; k < VS_MAX_K; ++k)
                red[wv][3 + k] = n_over[k];
        }
        __syncthreads();
        if (tid < 3 + a.k) {
            int sum = 0;
#pragma unroll
            for (int q = 0; q < VS_WAVES; ++q)
                sum += red[q][tid];
            if (sum != 0) {
                const size_t sp = (size_t)s * a.p + p;
                int *dst = tid == 0 ? a.inter + sp : tid == 1 ? a.uni + sp : tid == 2 ? a.visib_gt + s
                                                                                     : a.over + sp * a.k + (tid - 3);
                __hip_atomic_fetch_add(dst, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();                           // red is written again for the next pose
    }
}

// ---- MSSD, MSPD ------------------------------------------------------------------------------------------------------
constexpr int MD_BLOCK = 128;                      // points of a workgroup: one per lane
constexpr int MD_WAVES = MD_BLOCK / 64;

static int md_tiles(int m) { return ceil_div(m, MD_BLOCK); }

__device__ __forceinline__ int md_num_sym(const int *num_sym, int s, int smax)
{
    return min(max(num_sym[s], 1), smax);
}

// acc [b*p][smax][2]: the bit patterns of max_i |E x_i - G S x_i|^2 and of the largest squared pixel distance
__global__ __launch_bounds__(MD_BLOCK) void pose_max_dist_kernel(int p, int m, int tiles, const float *__restrict__ model,
                                                                int ps, long long cs, const double *__restrict__ est,
                                                                const double *__restrict__ gt, int smax,
                                                                const int *__restrict__ num_sym,
                                                                const double *__restrict__ sym,
                                                                const float *__restrict__ intrinsics, u64 *acc)
{
    __shared__ u64 red[MD_WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = blockIdx.x % tiles;
    const int sp = blockIdx.x / tiles;             // sample * p + pose
    const int s = sp / p;
    const int i = tile * MD_BLOCK + tid;
    const bool valid = i < m;
    const float *xp = model + (long long)s * cs + (long long)min(i, m - 1) * ps;
    const double x = (double)xp[0], y = (double)xp[1], z = (double)xp[2];
    double ex, ey, ez;
    icp_apply(est + 16ll * sp, x, y, z, ex, ey, ez);
    double fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0, ue = 0.0, ve = 0.0;
    if (intrinsics) {
        const float *kk = intrinsics + 5 * (size_t)s;
        fx = (double)kk[0], fy = (double)kk[1], cx = (double)kk[2], cy = (double)kk[3];
        ue = (fx * ex) / ez + cx;
        ve = (fy * ey) / ez + cy;
    }
    const int n = md_num_sym(num_sym, s, smax);
    for (int t = 0; t < n; ++t) {
        double sx, sy, sz, gx, gy, gz;
        icp_apply(sym + 16ll * ((long long)s * smax + t), x, y, z, sx, sy, sz);
        icp_apply(gt + 16ll * s, sx, sy, sz, gx, gy, gz);
        const double dx = ex - gx, dy = ey - gy, dz = ez - gz;
        double d3 = (dx * dx + dy * dy) + dz * dz, d2 = 0.0;
        if (intrinsics) {
            const double ug = (fx * gx) / gz + cx, vg = (fy * gy) / gz + cy;
            const double du = ue - ug, dv = ve - vg;
            d2 = (ez > 0.0 && gz > 0.0) ? du * du + dv * dv : (double)INFINITY;
        }
        if (!valid)
            d3 = d2 = 0.0;
        const u64 b3 = wave_max_u64(__builtin_bit_cast(u64, d3));
        const u64 b2 = wave_max_u64(__builtin_bit_cast(u64, d2));
        if (lane == 0) {
            red[wv][0] = b3;
            red[wv][1] = b2;
        }
        __syncthreads();
        if (tid < 2) {
            u64 best = red[0][tid];
#pragma unroll
            for (int q = 1; q < MD_WAVES; ++q)
                best = red[q][tid] > best ? red[q][tid] : best;
            u64 *cell = acc + 2 * ((size_t)sp * smax + t) + tid;
            // the plain read only spares atomics: the cell never shrinks, so what it shows is never above the maximum
            if (best > 0 && best > __atomic_load_n(cell, __ATOMIC_RELAXED))
                __hip_atomic_fetch_max(cell, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();                           // red is written again for the next symmetry
    }
}

// one lane per (sample, pose): the minimum over the symmetries (exact on the bits), then the square root
__global__ void pose_max_dist_finish_kernel(int n, int p, int smax, const int *__restrict__ num_sym,
                                            const u64 *__restrict__ acc, double *__restrict__ mssd,
                                            double *__restrict__ mspd)
{
    const int sp = blockIdx.x * blockDim.x + threadIdx.x;
    if (sp >= n)
        return;
    const int ns = md_num_sym(num_sym, sp / p, smax);
    const u64 *q = acc + 2 * (size_t)sp * smax;
    u64 b3 = q[0], b2 = q[1];
    for (int t = 1; t < ns; ++t) {
        b3 = q[2 * t] < b3 ? q[2 * t] : b3;
        b2 = q[2 * t + 1] < b2 ? q[2 * t + 1] : b2;
    }
    mssd[sp] = sqrt(__builtin_bit_cast(double, b3));
    if (mspd)
        mspd[sp] = sqrt(__builtin_bit_cast(double, b2));
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_vsd_counts(int f, int h, int w, const uint16_t *depth_test, const float *intrinsics, int b, int p,
                                     const int *frame_of, const uint16_t *depth_gt, const uint16_t *depth_est, double delta,
                                     int k, const double *tau, int *inter, int *uni, int *over, int *visib_gt,
                                     cloudaae_stream_t stream)
{
    const char *name = "cloudaae_vsd_counts";
    CLOUDAAE_REQUIRE(f >= 1 && h >= 1 && w >= 1 && b >= 1 && p >= 1, name, "f, h, w, b and p must be >= 1");
    CLOUDAAE_REQUIRE(k >= 1 && k <= VS_MAX_K, name, "k must lie in [1, 16]");
    CLOUDAAE_REQUIRE((long long)h * w <= FRAME_MAX_PIXELS, name, "h * w above 2^24");
    CLOUDAAE_REQUIRE((long long)b * p <= FRAME_MAX_TOTAL && (long long)b * p * ((long long)h * w) <= FRAME_MAX_TOTAL, name,
                     "b * p * h * w above 2^28");
    CLOUDAAE_REQUIRE(!isnan(delta), name, "delta is not a number");
    CLOUDAAE_REQUIRE(depth_test && intrinsics && frame_of && depth_gt && depth_est && tau && inter && uni && over && visib_gt,
                     name, "null pointer");
    VsdArgs a;
    a.f = f, a.h = h, a.w = w, a.b = b, a.p = p, a.k = k;
    a.tiles = ceil_div((long long)h * w, VS_TILE);
    a.depth_test = depth_test, a.depth_gt = depth_gt, a.depth_est = depth_est;
    a.intrinsics = intrinsics, a.frame_of = frame_of, a.delta = delta, a.tau = tau;
    a.inter = inter, a.uni = uni, a.over = over, a.visib_gt = visib_gt;
    hipStream_t sm = (hipStream_t)stream;
    const size_t bp = (size_t)b * p;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(inter, 0, sizeof(int) * bp, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(uni, 0, sizeof(int) * bp, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(over, 0, sizeof(int) * bp * k, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(visib_gt, 0, sizeof(int) * (size_t)b, sm), name);
    // b * tiles <= 2^28 / 2048 + b: below the grid limit
    hipLaunchKernelGGL(vsd_counts_kernel, dim3((unsigned)((long long)b * a.tiles)), dim3(VS_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API long long cloudaae_pose_max_dist_workspace_bytes(int b, int p, int smax)
{
    if (b < 1 || p < 1 || smax < 1)
        return -1;
    return (long long)sizeof(u64) * 2 * b * p * smax;
}

CLOUDAAE_API int cloudaae_pose_max_dist(int b, int p, int m, const float *model, int point_stride, long long cloud_stride,
                                        const double *est, const double *gt, int smax, const int *num_sym, const double *sym,
                                        const float *intrinsics, double *mssd, double *mspd, void *workspace,
                                        cloudaae_stream_t stream)
{
    const char *name = "cloudaae_pose_max_dist";
    CLOUDAAE_REQUIRE(b >= 1 && p >= 1 && m >= 1 && smax >= 1, name, "b, p, m and smax must be >= 1");
    CLOUDAAE_REQUIRE(point_stride >= 3, name, "point stride must be >= 3 floats");
    CLOUDAAE_REQUIRE(b == 1 || cloud_stride >= (long long)(m - 1) * point_stride + 3, name,
                     "cloud stride must not make clouds overlap");
    CLOUDAAE_REQUIRE(model && est && gt && num_sym && sym && mssd && workspace, name, "null pointer");
    CLOUDAAE_REQUIRE((intrinsics != nullptr) == (mspd != nullptr), name, "mspd and intrinsics go together: both or neither");
    const int tiles = md_tiles(m);
    CLOUDAAE_REQUIRE((long long)b * p * tiles <= INT_MAX && (long long)b * p * smax <= (1ll << 28), name,
                     "b * p * ceil(m / 128) above the grid limit of 2^31 - 1, or b * p * smax above 2^28");
    hipStream_t sm = (hipStream_t)stream;
    u64 *acc = static_cast<u64 *>(workspace);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(u64) * 2 * (size_t)b * p * smax, sm), name);
    hipLaunchKernelGGL(pose_max_dist_kernel, dim3(b * p * tiles), dim3(MD_BLOCK), 0, sm, p, m, tiles, model, point_stride,
                       cloud_stride, est, gt, smax, num_sym, sym, intrinsics, acc);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(pose_max_dist_finish_kernel, dim3(ceil_div((long long)b * p, 64)), dim3(64), 0, sm, b * p, p, smax,
                       num_sym, (const u64 *)acc, mssd, mspd);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
