// symmetry.hip -- the device side of the symmetry search: the directed Hausdorff distance of a point set, moved by each of
// many rigid transforms, from a second point set.  DESIGN.md, "Object symmetries", is the definition;
// tests/symmetry_reference.py restates it in NumPy.  All floating point is fp64 on exactly widened inputs, un-fused (the
// file is compiled with -ffp-contract=off), with the correctly rounded sqrt; the minima and maxima are exact, so nothing
// depends on the order of execution, the grid or the run.
//
//   cloudaae_transform_hausdorff   a memset and two launches.  A workgroup of 128 lanes takes 128 queries and SY_R = 4
//                                  consecutive candidates: a lane transforms its query under the four candidates once and
//                                  keeps the twelve coordinates and four running minima in registers.  The targets pass
//                                  through LDS as doubles, 1024 at a time (24 KiB); every lane reads the same target, so
//                                  LDS broadcasts it, and one read of three doubles serves 4 x 9 fp64 operations.  The
//                                  minima of a lane meet as integer maxima on the bit pattern of the non-negative double
//                                  (wave, LDS, one atomic per workgroup and candidate after a plain look); a second launch
//                                  takes the square root and applies limit2.
//                                  grid = (tiles of 128 queries) x (groups of 4 candidates), the query tile being the slow
//                                  index: a later tile of a candidate group that finds all four published maxima above
//                                  limit2 already leaves at once.  The result is +inf for those either way.
#include "common.h"
#include "pose_math.h"
#include "../../include/cloudaae_hip.h"

#include <limits.h>
#include <math.h>

namespace cloudaae {

typedef unsigned long long u64;

constexpr int SY_BLOCK = 128;                      // queries of a workgroup: one per lane
constexpr int SY_WAVES = SY_BLOCK / 64;
constexpr int SY_R = 4;                            // candidates of a workgroup
constexpr int SY_TILE = 1024;                      // targets staged in LDS at a time
constexpr int SY_MAX_C = 1 << 20;
constexpr int SY_MAX_POINTS = 1 << 24;             // m and n
constexpr size_t SY_LDS_BYTES = sizeof(double) * 3 * SY_TILE + sizeof(u64) * SY_WAVES * SY_R;

// acc [c]: the bit pattern of max_i min_j |T_c x_i - y_j|^2, zeroed before the launch
__global__ __launch_bounds__(SY_BLOCK) void transform_hausdorff_kernel(int c, int m, int groups,
                                                                      const float *__restrict__ queries, int qs, int n,
                                                                      const float *__restrict__ targets, int ts,
                                                                      const double *__restrict__ transforms,
                                                                      double limit2, u64 *acc)
{
    extern __shared__ __attribute__((aligned(16))) char sy_lds[];
    double *tx = reinterpret_cast<double *>(sy_lds), *ty = tx + SY_TILE, *tz = ty + SY_TILE;
    u64 *red = reinterpret_cast<u64 *>(tz + SY_TILE);          // [SY_WAVES][SY_R]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int group = blockIdx.x % groups, tile = blockIdx.x / groups;
    const int c0 = group * SY_R;

    // what is published never shrinks and never exceeds the maximum: a candidate already above limit2 stays +inf
    if (tid < SY_R) {
        const u64 seen = __hip_atomic_load(acc + min(c0 + tid, c - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        red[tid] = __builtin_bit_cast(double, seen) > limit2 ? 1 : 0;
    }
    __syncthreads();
    bool decided = true;
#pragma unroll
    for (int r = 0; r < SY_R; ++r)
        decided = decided && red[r] != 0;
    __syncthreads();                               // red is written again below
    if (decided)                                   // (the whole workgroup: every lane read the same four words)
        return;

    const int i = tile * SY_BLOCK + tid;
    const bool valid = i < m;
    const float *xp = queries + (long long)min(i, m - 1) * qs;
    const double x = (double)xp[0], y = (double)xp[1], z = (double)xp[2];
    double px[SY_R], py[SY_R], pz[SY_R], best[SY_R];
#pragma unroll
    for (int r = 0; r < SY_R; ++r) {
        icp_apply(transforms + 16ll * min(c0 + r, c - 1), x, y, z, px[r], py[r], pz[r]);
        best[r] = (double)INFINITY;
    }

    for (int j0 = 0; j0 < n; j0 += SY_TILE) {
        const int cnt = min(SY_TILE, n - j0);
        if (j0)
            __syncthreads();                       // the tile before is read no more
        for (int k = tid; k < cnt; k += SY_BLOCK) {
            const float *tp = targets + (long long)(j0 + k) * ts;
            tx[k] = (double)tp[0];
            ty[k] = (double)tp[1];
            tz[k] = (double)tp[2];
        }
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const double ux = tx[k], uy = ty[k], uz = tz[k];
#pragma unroll
            for (int r = 0; r < SY_R; ++r) {
                const double dx = px[r] - ux, dy = py[r] - uy, dz = pz[r] - uz;
                const double d = (dx * dx + dy * dy) + dz * dz;
                best[r] = fmin(best[r], d);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < SY_R; ++r) {
        const u64 b = wave_max_u64(valid ? __builtin_bit_cast(u64, best[r]) : 0ull);
        if (lane == 0)
            red[wv * SY_R + r] = b;
    }
    __syncthreads();
    if (tid < SY_R && c0 + tid < c) {
        u64 top = red[tid];
#pragma unroll
        for (int q = 1; q < SY_WAVES; ++q)
            top = red[q * SY_R + tid] > top ? red[q * SY_R + tid] : top;
        u64 *cell = acc + (c0 + tid);
        // the plain read only spares atomics: the cell never shrinks, so what it shows is never above the maximum
        if (top > 0 && top > __atomic_load_n(cell, __ATOMIC_RELAXED))
            __hip_atomic_fetch_max(cell, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one lane per candidate: the square root, or +inf above limit2
__global__ void transform_hausdorff_finish_kernel(int c, const u64 *__restrict__ acc, double limit2,
                                                  double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c)
        return;
    const double h2 = __builtin_bit_cast(double, acc[i]);
    out[i] = h2 <= limit2 ? sqrt(h2) : (double)INFINITY;
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API long long cloudaae_transform_hausdorff_workspace_bytes(int c)
{
    if (c < 1 || c > SY_MAX_C)
        return -1;
    return (long long)sizeof(u64) * c;
}

CLOUDAAE_API int cloudaae_transform_hausdorff(int c, int m, const float *queries, int q_stride, int n, const float *targets,
                                              int t_stride, const double *transforms, double limit2, double *out,
                                              void *workspace, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_transform_hausdorff";
    CLOUDAAE_REQUIRE(c >= 1 && c <= SY_MAX_C, name, "c must lie in [1, 2^20]");
    CLOUDAAE_REQUIRE(m >= 1 && m <= SY_MAX_POINTS && n >= 1 && n <= SY_MAX_POINTS, name, "m and n must lie in [1, 2^24]");
    CLOUDAAE_REQUIRE(q_stride >= 3 && t_stride >= 3, name, "point strides must be >= 3 floats");
    CLOUDAAE_REQUIRE(limit2 >= 0.0, name, "limit2 must be >= 0 (+inf allowed) and a number");
    CLOUDAAE_REQUIRE(queries && targets && transforms && out && workspace, name, "null pointer");
    const int groups = ceil_div(c, SY_R), tiles = ceil_div(m, SY_BLOCK);
    CLOUDAAE_REQUIRE((long long)groups * tiles <= INT_MAX, name, "ceil(c / 4) * ceil(m / 128) above the grid limit of 2^31 - 1");
    hipStream_t sm = (hipStream_t)stream;
    u64 *acc = static_cast<u64 *>(workspace);
    CLOUDAAE_CHECK_HIP(allow_dynamic_lds<transform_hausdorff_kernel>(SY_LDS_BYTES, SY_LDS_BYTES), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(u64) * (size_t)c, sm), name);
    hipLaunchKernelGGL(transform_hausdorff_kernel, dim3((unsigned)(groups * tiles)), dim3(SY_BLOCK), SY_LDS_BYTES, sm, c, m,
                       groups, queries, q_stride, n, targets, t_stride, transforms, limit2, acc);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(transform_hausdorff_finish_kernel, dim3(ceil_div(c, 256)), dim3(256), 0, sm, c, (const u64 *)acc, limit2,
                       out);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
