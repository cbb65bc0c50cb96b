// pose_score.hip -- ADD and ADD-S of estimated 6D poses against the ground truth, the diameter of an object model and
// the 4x4 pose matrices they take.  The definition, in float64, is written out in DESIGN.md ("Pose scores") and
// restated in NumPy by tests/pose_score_reference.py.
//
// ADD-S is a nearest-neighbour search of m x m pairs per sample and pose; the diameter a farthest-pair search of the
// same shape.  Both run the same exact fp64 brute force:
//   - grid = (tiles of PS_QUERIES = 64 queries) x poses x samples, flattened: b = p = 1, m = 2048 starts 32 workgroups
//     of 8 waves, one sample is spread over the machine;
//   - lane l of EVERY wave of a workgroup holds query 64 * tile + l in registers (g_i: the model point under the
//     ground truth); the candidates (e_j: the model under the estimate) are transformed PS_TILE = 512 at a time, one
//     per thread, into LDS, so m is not bounded by LDS; wave w scans candidates [64 w, 64 w + 64) of the tile: all
//     lanes read the same LDS address (a broadcast, no bank conflict) and keep their running minimum in a register;
//   - the eight waves' minima meet in LDS (min is exact: no order to fix), wave 0 takes the square roots and sums
//     its 64 terms by a butterfly, and lane 0 stores the tile's two partial sums;
//   - a second, tiny kernel adds the tiles' partial sums in ascending tile order and divides by m.  No
//     floating-point atomics, no order that depends on b, p or the launch: bit-reproducible.
#include "common.h"
#include "../../include/cloudaae_hip.h"
#include "pose_math.h"

#include <limits.h>
#include <math.h>

using namespace cloudaae;

namespace {

constexpr int PS_QUERIES = 64;                    // queries of a workgroup: one per lane
constexpr int PS_WAVES = 8;
constexpr int PS_THREADS = PS_QUERIES * PS_WAVES;
constexpr int PS_TILE = PS_THREADS;               // candidates staged per pass: one per thread, 64 per wave

static int ps_tiles(int m) { return ceil_div(m, PS_QUERIES); }

// FARTHEST = false: out[l] = min_j |q_l - E x_j|^2 with q_l = G x_i, i = 64 tile + l (E, G: 3x4 row-major, fp64).
// FARTHEST = true : out[l] = max_j |x_i - x_j|^2 (no transform).  Result in every lane of wave 0 (the other waves
// return garbage); lanes with i >= m work on point m - 1.  qx, qy, qz: the lane's query, returned.
template <bool FARTHEST>
__device__ __forceinline__ double ps_scan(const float *__restrict__ X, int ps, int m, int tile, const double *E,
                                          const double *G, double (*cand)[3], double (*red)[PS_QUERIES], double &qx,
                                          double &qy, double &qz)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    {
        const int i = min(tile * PS_QUERIES + lane, m - 1);
        const float *x = X + (long long)i * ps;
        if (FARTHEST) {
            qx = (double)x[0];
            qy = (double)x[1];
            qz = (double)x[2];
        } else {
            icp_apply(G, (double)x[0], (double)x[1], (double)x[2], qx, qy, qz);
        }
    }
    double best = FARTHEST ? 0.0 : INFINITY;
    for (int t0 = 0; t0 < m; t0 += PS_TILE) {
        const int jn = min(PS_TILE, m - t0);
        __syncthreads();                                  // the previous pass has been read
        if (tid < jn) {
            const float *x = X + (long long)(t0 + tid) * ps;
            if (FARTHEST) {
                cand[tid][0] = (double)x[0];
                cand[tid][1] = (double)x[1];
                cand[tid][2] = (double)x[2];
            } else {
                icp_apply(E, (double)x[0], (double)x[1], (double)x[2], cand[tid][0], cand[tid][1], cand[tid][2]);
            }
        }
        __syncthreads();
        const double (*cw)[3] = cand + 64 * w;            // this wave's 64 candidates of the pass
        const int cnt = jn - 64 * w;                      // wave-uniform
        if (cnt >= 64) {
            for (int j0 = 0; j0 < 64; j0 += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int j = j0 + u;
                    const double dx = qx - cw[j][0], dy = qy - cw[j][1], dz = qz - cw[j][2];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    best = FARTHEST ? fmax(best, d2) : fmin(best, d2);
                }
            }
        } else {
            for (int j = 0; j < cnt; ++j) {
                const double dx = qx - cw[j][0], dy = qy - cw[j][1], dz = qz - cw[j][2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                best = FARTHEST ? fmax(best, d2) : fmin(best, d2);
            }
        }
    }
    red[w][lane] = best;
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int k = 1; k < PS_WAVES; ++k)
            best = FARTHEST ? fmax(best, red[k][lane]) : fmin(best, red[k][lane]);
    }
    return best;
}

// partial [b*p][tiles][2]: the tile's sums of |g_i - e_i| and of sqrt(nn_d2[i]) (lanes in butterfly order)
__global__ void __launch_bounds__(PS_THREADS)
pose_score_tile_kernel(int p, int m, int tiles, const float *__restrict__ model, int ps, long long cs,
                       const double *__restrict__ est, const double *__restrict__ gt, double *__restrict__ nn_d2,
                       double *__restrict__ partial)
{
    __shared__ double cand[PS_TILE][3];
    __shared__ double red[PS_WAVES][PS_QUERIES];
    __shared__ double mats[24];
    const int tid = threadIdx.x, lane = tid & 63;
    const int tile = blockIdx.x % tiles;
    const int sp = blockIdx.x / tiles;                    // sample * p + pose
    const int s = sp / p;
    if (tid < 12)
        mats[tid] = est[16LL * sp + tid];
    else if (tid < 24)
        mats[tid] = gt[16LL * s + (tid - 12)];
    __syncthreads();
    const float *X = model + (long long)s * cs;
    double qx, qy, qz;
    const double nn = ps_scan<false>(X, ps, m, tile, mats, mats + 12, cand, red, qx, qy, qz);
    if (tid < 64) {
        const int i = tile * PS_QUERIES + lane;
        double a = 0.0, d = 0.0;
        if (i < m) {
            const float *x = X + (long long)i * ps;
            double ex, ey, ez;
            icp_apply(mats, (double)x[0], (double)x[1], (double)x[2], ex, ey, ez);
            const double dx = qx - ex, dy = qy - ey, dz = qz - ez;
            a = sqrt((dx * dx + dy * dy) + dz * dz);
            d = sqrt(nn);
            if (nn_d2)
                nn_d2[(long long)sp * m + i] = nn;
        }
        a = wave_sum(a);
        d = wave_sum(d);
        if (lane == 0) {
            partial[2 * ((long long)sp * tiles + tile)] = a;
            partial[2 * ((long long)sp * tiles + tile) + 1] = d;
        }
    }
}

// one lane per (sample, pose): the tiles' sums in ascending tile order, divided by m
__global__ void pose_score_finish_kernel(int n, int m, int tiles, const double *__restrict__ partial,
                                         double *__restrict__ add, double *__restrict__ adds)
{
    const int sp = blockIdx.x * blockDim.x + threadIdx.x;
    if (sp >= n)
        return;
    const double *q = partial + 2LL * sp * tiles;
    double a = q[0], d = q[1];
    for (int t = 1; t < tiles; ++t) {
        a += q[2 * t];
        d += q[2 * t + 1];
    }
    add[sp] = a / (double)m;
    adds[sp] = d / (double)m;
}

// partial [c][tiles]: the largest squared distance from a point of the tile to any point of the cloud
__global__ void __launch_bounds__(PS_THREADS)
cloud_diameter_tile_kernel(int m, int tiles, const float *__restrict__ model, int ps, long long cs,
                           double *__restrict__ partial)
{
    __shared__ double cand[PS_TILE][3];
    __shared__ double red[PS_WAVES][PS_QUERIES];
    const int tile = blockIdx.x % tiles, c = blockIdx.x / tiles;
    double qx, qy, qz;
    double far = ps_scan<true>(model + (long long)c * cs, ps, m, tile, nullptr, nullptr, cand, red, qx, qy, qz);
    if (threadIdx.x < 64) {
        far = fmax(far, __shfl_xor(far, 32, 64));
        far = fmax(far, __shfl_xor(far, 16, 64));
        far = fmax(far, __shfl_xor(far, 8, 64));
        far = fmax(far, __shfl_xor(far, 4, 64));
        far = fmax(far, __shfl_xor(far, 2, 64));
        far = fmax(far, __shfl_xor(far, 1, 64));
        if (threadIdx.x == 0)
            partial[(long long)c * tiles + tile] = far;
    }
}

__global__ void cloud_diameter_finish_kernel(int n, int tiles, const double *__restrict__ partial,
                                             double *__restrict__ diam)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n)
        return;
    double far = 0.0;
    for (int t = 0; t < tiles; ++t)
        far = fmax(far, partial[(long long)c * tiles + t]);
    diam[c] = sqrt(far);
}

__global__ void pose_matrix_kernel(int n, const void *__restrict__ rot, int rot_is_f64,
                                   const float *__restrict__ trans, double *__restrict__ out)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n)
        return;
    double r[3], R[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        r[a] = rot_is_f64 ? static_cast<const double *>(rot)[3LL * c + a]
                          : (double)static_cast<const float *>(rot)[3LL * c + a];
    icp_rodrigues(r[0], r[1], r[2], R);
    double *T = out + 16LL * c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        T[4 * a] = R[3 * a];
        T[4 * a + 1] = R[3 * a + 1];
        T[4 * a + 2] = R[3 * a + 2];
        T[4 * a + 3] = (double)trans[3LL * c + a];
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

__global__ void pose_stack_kernel(int n, const double *__restrict__ first,
                                  const double *__restrict__ second, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;     // over n * 32 doubles
    if (i >= n * 32)
        return;
    const int c = i >> 5, k = i & 31;
    out[i] = k < 16 ? first[16LL * c + k] : second[16LL * c + (k - 16)];
}

const long long PS_MAX_GRID = INT_MAX;

}  // namespace

CLOUDAAE_API long long cloudaae_pose_score_workspace_bytes(int b, int p, int m)
{
    if (b < 1 || p < 1 || m < 1)
        return -1;
    return (long long)sizeof(double) * 2 * b * p * ps_tiles(m);
}

CLOUDAAE_API int cloudaae_pose_score(int b, int p, int m, const float *model, int point_stride, long long cloud_stride,
                                     const double *est, const double *gt, double *add, double *adds, double *nn_d2,
                                     void *workspace, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_pose_score";
    CLOUDAAE_REQUIRE(b >= 1 && p >= 1 && m >= 1, name, "b, p and m must be >= 1");
    CLOUDAAE_REQUIRE(point_stride >= 3, name, "point stride must be >= 3 floats");
    CLOUDAAE_REQUIRE(b == 1 || cloud_stride >= (long long)(m - 1) * point_stride + 3, name,
                     "cloud stride must not make clouds overlap");
    CLOUDAAE_REQUIRE(model && est && gt && add && adds && workspace, name, "null pointer");
    const int tiles = ps_tiles(m);
    CLOUDAAE_REQUIRE((long long)b * p * tiles <= PS_MAX_GRID, name, "b * p * ceil(m / 64) above the grid limit of 2^31 - 1");
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(pose_score_tile_kernel, dim3(b * p * tiles), dim3(PS_THREADS), 0, (hipStream_t)stream, p, m,
                       tiles, model, point_stride, cloud_stride, est, gt, nn_d2, partial);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(pose_score_finish_kernel, dim3(ceil_div((long long)b * p, 64)), dim3(64), 0, (hipStream_t)stream,
                       b * p, m, tiles, partial, add, adds);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API long long cloudaae_cloud_diameter_workspace_bytes(int c, int m)
{
    if (c < 1 || m < 1)
        return -1;
    return (long long)sizeof(double) * c * ps_tiles(m);
}

CLOUDAAE_API int cloudaae_cloud_diameter(int c, int m, const float *model, int point_stride, long long cloud_stride,
                                         double *diam, void *workspace, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_cloud_diameter";
    CLOUDAAE_REQUIRE(c >= 1 && m >= 1, name, "c and m must be >= 1");
    CLOUDAAE_REQUIRE(point_stride >= 3, name, "point stride must be >= 3 floats");
    CLOUDAAE_REQUIRE(c == 1 || cloud_stride >= (long long)(m - 1) * point_stride + 3, name,
                     "cloud stride must not make clouds overlap");
    CLOUDAAE_REQUIRE(model && diam && workspace, name, "null pointer");
    const int tiles = ps_tiles(m);
    CLOUDAAE_REQUIRE((long long)c * tiles <= PS_MAX_GRID, name, "c * ceil(m / 64) above the grid limit of 2^31 - 1");
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(cloud_diameter_tile_kernel, dim3(c * tiles), dim3(PS_THREADS), 0, (hipStream_t)stream, m, tiles,
                       model, point_stride, cloud_stride, partial);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(cloud_diameter_finish_kernel, dim3(ceil_div(c, 64)), dim3(64), 0, (hipStream_t)stream, c, tiles,
                       partial, diam);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_pose_matrix(int b, const void *rot, int rot_is_f64, const float *trans, double *out,
                                      cloudaae_stream_t stream)
{
    const char *name = "cloudaae_pose_matrix";
    CLOUDAAE_REQUIRE(b >= 1, name, "b must be >= 1");
    CLOUDAAE_REQUIRE(rot_is_f64 == 0 || rot_is_f64 == 1, name, "rot_is_f64 must be 0 or 1");
    CLOUDAAE_REQUIRE(rot && trans && out, name, "null pointer");
    hipLaunchKernelGGL(pose_matrix_kernel, dim3(ceil_div(b, 64)), dim3(64), 0, (hipStream_t)stream, b, rot, rot_is_f64,
                       trans, out);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_pose_stack(int b, const double *first, const double *second, double *out,
                                     cloudaae_stream_t stream)
{
    const char *name = "cloudaae_pose_stack";
    CLOUDAAE_REQUIRE(b >= 1 && b <= (1 << 24), name, "b must lie in [1, 2^24]");
    CLOUDAAE_REQUIRE(first && second && out, name, "null pointer");
    hipLaunchKernelGGL(pose_stack_kernel, dim3(ceil_div(32LL * b, 256)), dim3(256), 0, (hipStream_t)stream, b, first,
                       second, out);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
