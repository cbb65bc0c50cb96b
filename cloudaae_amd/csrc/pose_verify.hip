// pose_verify.hip -- the device side of pose verification: hypotheses composed from a base pose, the per-pixel agreement
// of each rendered hypothesis with the depth the camera saw, and the choice of the winner.  DESIGN.md, "Pose
// verification", is the definition; tests/pose_verify_reference.py restates it in NumPy.  The composition is fp64,
// un-fused (the file is compiled with -ffp-contract=off), products and sums in the written order; the counts are
// integer arithmetic on the uint16 depths widened to int, and the winner is chosen by integer cross-multiplication, so
// nothing depends on the order of execution, the batch or the run.
//
//   cloudaae_pose_compose       one launch, one lane per (sample, hypothesis): base_i H_{c,j}, its log map
//                               (icp_log_map of pose_math.h) and the float translation.
//   cloudaae_depth_fit_counts   three memsets and one launch.  A workgroup of 256 threads takes a run of 2048 pixels
//                               of one sample, eight CONSECUTIVE pixels per thread: the test depth, the label and seg
//                               are read once and kept in registers, then every hypothesis of the sample is streamed
//                               against them.  Where a run starts on a 16-byte boundary a lane reads its eight depths
//                               with one 16-byte load (the label: one 8-byte load); a run that does not, and the lanes
//                               of a run's tail, read pixel by pixel.  The choice is the workgroup's, per array, from
//                               the run's address.  A predicate is counted by ballot + popcount per wave, the four
//                               waves meet in LDS once per eight hypotheses, and one integer atomic per workgroup,
//                               hypothesis and non-zero counter adds into the zeroed outputs.  The next hypothesis'
//                               depths are loaded while the current ones are compared.  A wave whose part of a
//                               hypothesis is all zero skips the comparisons.
//   cloudaae_select_pose        one launch, one lane per sample: the largest num / den by int64 cross-multiplication.
#include "common.h"
#include "pose_math.h"
#include "../../include/cloudaae_hip.h"

#include <limits.h>
#include <math.h>

namespace cloudaae {

typedef unsigned long long u64;
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));

constexpr long long PV_MAX_PIXELS = 1ll << 24;     // H W
constexpr long long PV_MAX_TOTAL = 1ll << 28;      // B P H W, B P

// ---- cloudaae_pose_compose ---------------------------------------------------------------------------------------------
constexpr int PC_BLOCK = 64;

__global__ __launch_bounds__(PC_BLOCK) void pose_compose_kernel(int n, int p, const double *__restrict__ base,
                                                                const long long *__restrict__ class_id, int nclass,
                                                                const int *__restrict__ hyp_index, int n_total,
                                                                const double *__restrict__ hyp,
                                                                double *__restrict__ pose, double *__restrict__ rot_axag,
                                                                float *__restrict__ trans, int *__restrict__ valid)
{
    const int e = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (e >= n)
        return;
    const int i = e / p, j = e % p;
    // the class's members; anything that would leave the table is an empty set and is never followed
    int first = 0, count = 0;
    const long long cls = class_id[i];
    if (cls >= 0 && cls < nclass) {
        first = hyp_index[cls];
        count = hyp_index[cls + 1] - first;
        if (first < 0 || count < 0 || (long long)first + count > n_total)
            count = 0;
    }
    const bool ok = j < count;
    double H[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};       // an empty set: the identity
    if (count > 0) {
        const double *src = hyp + 16ll * (first + (ok ? j : 0));
        for (int k = 0; k < 12; ++k)
            H[k] = src[k];
    }
    const double *A = base + 16ll * i;
    double C[12], R[9], r[3];
    for (int row = 0; row < 3; ++row) {
        const double a0 = A[4 * row + 0], a1 = A[4 * row + 1], a2 = A[4 * row + 2], a3 = A[4 * row + 3];
        for (int c = 0; c < 3; ++c)
            C[4 * row + c] = (a0 * H[c] + a1 * H[4 + c]) + a2 * H[8 + c];
        C[4 * row + 3] = ((a0 * H[3] + a1 * H[7]) + a2 * H[11]) + a3;
    }
    for (int row = 0; row < 3; ++row)
        for (int c = 0; c < 3; ++c)
            R[3 * row + c] = C[4 * row + c];
    icp_log_map(R, r);
    double *out = pose + 16ll * e;
    for (int k = 0; k < 12; ++k)
        out[k] = C[k];
    out[12] = out[13] = out[14] = 0.0;
    out[15] = 1.0;
    for (int k = 0; k < 3; ++k) {
        rot_axag[3ll * e + k] = r[k];
        trans[3ll * e + k] = (float)C[4 * k + 3];
    }
    valid[e] = ok ? 1 : 0;
}

// ---- cloudaae_depth_fit_counts -----------------------------------------------------------------------------------------
constexpr int DF_BLOCK = 256;
constexpr int DF_WAVES = DF_BLOCK / 64;
constexpr int DF_PIX = 8;                          // consecutive pixels of a thread: 16 bytes of depth
constexpr int DF_TILE = DF_BLOCK * DF_PIX;         // pixels of a workgroup
constexpr int DF_COUNTERS = 6;                     // rendered, consistent, in_front, behind, unknown, explained
constexpr int DF_SLOTS = DF_COUNTERS + 2;          // + seg_total (hypothesis 0 only) + the sum of |d - t|
constexpr int DF_CHUNK = 8;                        // hypotheses between two meetings of the workgroup
static_assert(DF_CHUNK * DF_SLOTS <= DF_BLOCK, "one thread per (hypothesis of a chunk, slot)");

struct DepthFitArgs {
    int f, h, w, b, p, tiles;
    const unsigned short *depth_test, *depth_hyp;
    const unsigned char *label;
    const int *frame_of, *want, *tau;
    int *counts, *seg_total;
    long long *abs_sum;
};

// the lane's eight depths of a run of n pixels: one 16-byte load where the run is aligned and the lane lies inside,
// else pixel by pixel with zeros past the end
__device__ __forceinline__ void df_load8(const unsigned short *run, int n, int off, bool aligned, int v[DF_PIX])
{
    if (aligned && off + DF_PIX <= n) {
        const uint4v q = *reinterpret_cast<const uint4v *>(run + off);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = (int)(q[i] & 0xffffu);
            v[2 * i + 1] = (int)(q[i] >> 16);
        }
    } else {
#pragma unroll
        for (int i = 0; i < DF_PIX; ++i)
            v[i] = off + i < n ? (int)run[off + i] : 0;
    }
}

__global__ __launch_bounds__(DF_BLOCK) void depth_fit_counts_kernel(DepthFitArgs a)
{
    __shared__ int red[DF_CHUNK][DF_WAVES][DF_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f)                       // (the whole workgroup: no barrier has been reached)
        return;
    const int hw = a.h * a.w;
    const int start = tile * DF_TILE;              // the run: pixels start .. start + n - 1 of the frame
    const int n = hw - start < DF_TILE ? hw - start : DF_TILE;
    const int off = tid * DF_PIX;
    const int tau = a.tau[s];

    // once per pixel: t and seg
    int t[DF_PIX];
    const unsigned short *trun = a.depth_test + (size_t)fr * hw + start;
    df_load8(trun, n, off, ((uintptr_t)trun & 15u) == 0, t);
    unsigned seg = 0;
    if (a.label) {
        const unsigned char *lrun = a.label + (size_t)fr * hw + start;
        const int want = a.want[s];
        if (((uintptr_t)lrun & 7u) == 0 && off + DF_PIX <= n) {
            const uint2v q = *reinterpret_cast<const uint2v *>(lrun + off);
#pragma unroll
            for (int i = 0; i < DF_PIX; ++i)
                seg |= (unsigned)((int)((q[i >> 2] >> (8 * (i & 3))) & 0xffu) == want && t[i] != 0) << i;
        } else {
#pragma unroll
            for (int i = 0; i < DF_PIX; ++i)
                seg |= (unsigned)(off + i < n && (int)lrun[off + i] == want && t[i] != 0) << i;
        }
    }
    int n_seg = 0;
#pragma unroll
    for (int i = 0; i < DF_PIX; ++i)
        n_seg += wave_count((seg >> i) & 1u);

    // the hypotheses, DF_CHUNK at a time: a wave leaves its counts of each in LDS, and the workgroup meets once per chunk.
    // The depths of the next hypothesis are on their way while the current ones are compared.
    const unsigned short *hyp0 = a.depth_hyp + (size_t)s * a.p * hw + start;
    int d[DF_PIX], nx[DF_PIX];
    df_load8(hyp0, n, off, ((uintptr_t)hyp0 & 15u) == 0, nx);
    for (int j0 = 0; j0 < a.p; j0 += DF_CHUNK) {
        const int nj = a.p - j0 < DF_CHUNK ? a.p - j0 : DF_CHUNK;
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
#pragma unroll
            for (int i = 0; i < DF_PIX; ++i)
                d[i] = nx[i];
            if (j + 1 < a.p) {
                const unsigned short *drun = hyp0 + (size_t)(j + 1) * hw;
                df_load8(drun, n, off, ((uintptr_t)drun & 15u) == 0, nx);
            }
            int cnt[DF_COUNTERS] = {0, 0, 0, 0, 0, 0};
            int asum = 0;
            const bool any = ((d[0] | d[1]) | (d[2] | d[3])) | ((d[4] | d[5]) | (d[6] | d[7]));
            if (__builtin_amdgcn_ballot_w64(any)) {    // (wave-uniform) a wave whose part is all zero counts nothing
#pragma unroll
                for (int i = 0; i < DF_PIX; ++i) {
                    const bool rend = d[i] != 0, both = rend && t[i] != 0;
                    const int diff = d[i] - t[i], mag = diff < 0 ? -diff : diff;
                    const bool cons = both && mag <= tau;
                    cnt[0] += wave_count(rend);
                    cnt[1] += wave_count(cons);
                    cnt[2] += wave_count(both && -diff > tau);
                    cnt[3] += wave_count(both && diff > tau);
                    cnt[4] += wave_count(rend && t[i] == 0);
                    cnt[5] += wave_count(cons && ((seg >> i) & 1u));
                    asum += cons ? mag : 0;
                }
            }
            // at most 512 * 65535: an int holds the wave's and the workgroup's sum
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                asum += __builtin_amdgcn_ds_bpermute((lane ^ o) << 2, asum);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < DF_COUNTERS; ++k)
                    red[jj][wv][k] = cnt[k];
                red[jj][wv][DF_COUNTERS] = j == 0 ? n_seg : 0;
                red[jj][wv][DF_COUNTERS + 1] = asum;
            }
        }
        __syncthreads();
        if (tid < nj * DF_SLOTS) {                 // one thread per (hypothesis of the chunk, slot)
            const int jj = tid / DF_SLOTS, slot = tid % DF_SLOTS;
            const size_t sp = (size_t)s * a.p + (j0 + jj);
            int sum = 0;
#pragma unroll
            for (int q = 0; q < DF_WAVES; ++q)
                sum += red[jj][q][slot];
            if (sum != 0) {
                if (slot < DF_COUNTERS)
                    __hip_atomic_fetch_add(a.counts + sp * DF_COUNTERS + slot, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else if (slot == DF_COUNTERS)
                    __hip_atomic_fetch_add(a.seg_total + s, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else
                    __hip_atomic_fetch_add(a.abs_sum + sp, (long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();                           // red is written again for the next chunk
    }
}

// ---- cloudaae_select_pose ----------------------------------------------------------------------------------------------
constexpr int SP_BLOCK = 64;

// num and den of hypothesis j (0 / 1 for "no score"): the segment rule or the silhouette rule
__device__ __forceinline__ void sp_fraction(const int *c, int seg_total, int valid, int mode, long long &num,
                                            long long &den)
{
    if (mode == 0) {
        num = c[5];
        den = (long long)seg_total + c[2];
    } else {
        num = c[1];
        den = ((long long)c[1] + c[2]) + c[3];
    }
    if (den <= 0 || num < 0 || valid == 0) {
        num = 0;
        den = 1;
    }
}

__global__ __launch_bounds__(SP_BLOCK) void select_pose_kernel(int b, int p, const int *__restrict__ counts,
                                                               const int *__restrict__ seg_total,
                                                               const int *__restrict__ valid,
                                                               const double *__restrict__ pose, int mode,
                                                               int *__restrict__ best, double *__restrict__ score,
                                                               double *__restrict__ pose_best, double *__restrict__ margin)
{
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= b)
        return;
    const int st = seg_total[i];
    const size_t row = (size_t)i * p;
    int win = 0, second = -1;
    long long wn = 0, wd = 1, rn = 0, rd = 1;      // the winner's and the runner-up's fraction
    for (int j = 0; j < p; ++j) {
        long long num, den;
        sp_fraction(counts + (row + j) * DF_COUNTERS, st, valid[row + j], mode, num, den);
        score[row + j] = num == 0 ? 0.0 : (double)num / (double)den;
        if (j == 0) {
            wn = num, wd = den;
        } else if (num * wd > wn * den) {          // strictly larger: ties stay with the lower index
            second = win, rn = wn, rd = wd;
            win = j, wn = num, wd = den;
        } else if (second < 0 || num * rd > rn * den) {
            second = j, rn = num, rd = den;
        }
    }
    best[i] = win;
    const double ws = wn == 0 ? 0.0 : (double)wn / (double)wd, rs = rn == 0 ? 0.0 : (double)rn / (double)rd;
    margin[i] = second < 0 ? 0.0 : ws - rs;
    for (int k = 0; k < 16; ++k)
        pose_best[16ll * i + k] = pose[16ll * (row + win) + k];
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_pose_compose(int b, const double *base, const long long *class_id, int nclass, const int *hyp_index,
                                       int n_total, const double *hyp, int p, double *pose, double *rot_axag, float *trans,
                                       int *valid, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_pose_compose";
    CLOUDAAE_REQUIRE(b >= 1 && p >= 1 && (long long)b * p <= PV_MAX_TOTAL, name, "b and p must be >= 1 and b * p <= 2^28");
    CLOUDAAE_REQUIRE(nclass >= 1 && n_total >= 0 && n_total <= (1 << 24), name, "nclass must be >= 1 and n_total in [0, 2^24]");
    CLOUDAAE_REQUIRE(base && class_id && hyp_index && pose && rot_axag && trans && valid, name, "null pointer");
    CLOUDAAE_REQUIRE(hyp || n_total == 0, name, "hyp is null with n_total > 0");
    const int n = b * p;
    hipLaunchKernelGGL(pose_compose_kernel, dim3(ceil_div(n, PC_BLOCK)), dim3(PC_BLOCK), 0, (hipStream_t)stream, n, p, base,
                       class_id, nclass, hyp_index, n_total, hyp, pose, rot_axag, trans, valid);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_depth_fit_counts(int f, int h, int w, const uint16_t *depth_test, const uint8_t *label, int b, int p,
                                           const int *frame_of, const int *want, const uint16_t *depth_hyp, const int *tau,
                                           int *counts, int *seg_total, long long *abs_sum, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_fit_counts";
    CLOUDAAE_REQUIRE(f >= 1 && h >= 1 && w >= 1 && b >= 1 && p >= 1, name, "f, h, w, b and p must be >= 1");
    CLOUDAAE_REQUIRE((long long)h * w <= PV_MAX_PIXELS, name, "h * w above 2^24");
    CLOUDAAE_REQUIRE((long long)b * p <= PV_MAX_TOTAL && (long long)b * p * ((long long)h * w) <= PV_MAX_TOTAL, name,
                     "b * p * h * w above 2^28");
    CLOUDAAE_REQUIRE(depth_test && frame_of && depth_hyp && tau && counts && seg_total && abs_sum, name, "null pointer");
    CLOUDAAE_REQUIRE(want || !label, name, "a label image needs want");
    DepthFitArgs a;
    a.f = f, a.h = h, a.w = w, a.b = b, a.p = p;
    a.tiles = ceil_div((long long)h * w, DF_TILE);
    a.depth_test = depth_test, a.depth_hyp = depth_hyp, a.label = label;
    a.frame_of = frame_of, a.want = want, a.tau = tau;
    a.counts = counts, a.seg_total = seg_total, a.abs_sum = abs_sum;
    hipStream_t sm = (hipStream_t)stream;
    const size_t bp = (size_t)b * p;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * bp * DF_COUNTERS, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(seg_total, 0, sizeof(int) * (size_t)b, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(abs_sum, 0, sizeof(long long) * bp, sm), name);
    // b * tiles <= 2^28 / 2048 + b: below the grid limit
    hipLaunchKernelGGL(depth_fit_counts_kernel, dim3((unsigned)((long long)b * a.tiles)), dim3(DF_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_select_pose(int b, int p, const int *counts, const int *seg_total, const int *valid,
                                      const double *pose, int mode, int *best, double *score, double *pose_best,
                                      double *margin, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_select_pose";
    CLOUDAAE_REQUIRE(b >= 1 && p >= 1 && (long long)b * p <= PV_MAX_TOTAL, name, "b and p must be >= 1 and b * p <= 2^28");
    CLOUDAAE_REQUIRE(mode == 0 || mode == 1, name, "mode must be 0 (segment rule) or 1 (silhouette rule)");
    CLOUDAAE_REQUIRE(counts && seg_total && valid && pose && best && score && pose_best && margin, name, "null pointer");
    hipLaunchKernelGGL(select_pose_kernel, dim3(ceil_div(b, SP_BLOCK)), dim3(SP_BLOCK), 0, (hipStream_t)stream, b, p, counts,
                       seg_total, valid, pose, mode, best, score, pose_best, margin);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
