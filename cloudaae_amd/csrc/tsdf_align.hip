// tsdf_align.hip -- one Gauss-Newton step that aligns depth frames on the signed distance field of a fused volume, for b
// samples (gfx950): every observed pixel of a window is back-projected, carried into the object's frame by the current
// pose, and reads the trilinear field value there as its residual and the field's gradient as its normal.  No raycast and
// no second normal map.  DESIGN.md, "Scanning on the field", is the definition; tests/sdf_align_reference.py restates it in
// NumPy.  Everything is fp64 on exactly widened integers and fp32 values, un-fused (the file is compiled with
// -ffp-contract=off), in the order written here.
//
//   cloudaae_tsdf_align_step   two launches, shaped as cloudaae_depth_align_step.  tsdf_align_sums_kernel: a workgroup of 256
//                              lanes takes a run of 2048 window pixels of one sample, eight CONSECUTIVE ones per lane, and
//                              stores its 28 partial sums and its count to the workspace.  tsdf_align_solve_kernel: one wave
//                              per sample adds the runs in run order, solves the 6 x 6 system by LDL^T and writes U pose_in.
//
// No floating-point atomic, no ticket, no workgroup waits for another: a sample's result is the same bits run to run and
// whatever else is in the batch.  The sample's pose and camera sit at addresses that are the same in every lane of the
// workgroup; the eight states of a pixel's cell are loaded together before the values are formed, as the raycast does
// (tsdf_field.h).  The sums, their reduction, the solve and the pose write are depth_gn.h's, unchanged.
#include "common.h"
#include "depth_gn.h"
#include "tsdf_field.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

namespace cloudaae {

struct TsdfAlignArgs {
    TsdfVolume vol;
    const int4 *state;
    int min_count;
    double front;
    int f, h, w, wh, ww, tiles;
    const unsigned short *depth;
    const unsigned char *label;                    // or null
    const int *want;                               // or null; the filter is on only with both
    const int *frame_of, *origin;
    const float *intr_win;
    const double *pose_in;
    double *part_sums;                             // [b, tiles, 28]
    int *part_count;                               // [b, tiles]
};

// one axis of q = R^T (p - t), a two-level sum, as a grid coordinate: g = (q - origin) / s - 0.5
__device__ __forceinline__ double ta_grid(double r0, double r1, double r2, const double (&e)[3], double origin, double s)
{
    const double q = (r0 * e[0] + r1 * e[1]) + r2 * e[2];
    return (q - origin) / s - 0.5;
}

// The row (J, r) of window pixel (x, y) whose frame depth is d != 0 -> false when the pixel has none.
__device__ __forceinline__ bool ta_row(const TsdfAlignArgs &a, const Pinhole<double> &cam, const double *A, int x, int y, int d,
                                       double (&J)[6], double &r)
{
    double p[3];
    backproject(cam, x, y, d, p);
    const double e[3] = {p[0] - A[3], p[1] - A[7], p[2] - A[11]};
    const double gx = ta_grid(A[0], A[4], A[8], e, a.vol.ox, a.vol.s);
    const double gy = ta_grid(A[1], A[5], A[9], e, a.vol.oy, a.vol.s);
    const double gz = ta_grid(A[2], A[6], A[10], e, a.vol.oz, a.vol.s);
    const int nx = a.vol.nx, ny = a.vol.ny, nz = a.vol.nz;
    if (!(gx >= 0.0 && gx <= (double)(nx - 1) && gy >= 0.0 && gy <= (double)(ny - 1) && gz >= 0.0 &&
          gz <= (double)(nz - 1)))                 // in float64, before any conversion; a NaN fails
        return false;
    const int i = tsdf_ray_cell(gx, nx), j = tsdf_ray_cell(gy, ny), k = tsdf_ray_cell(gz, nz);
    double v[8];
    if (!tsdf_cell_values(a.state, nx, ny, i, j, k, a.min_count, v))
        return false;
    const double fy = gy - (double)j, fz = gz - (double)k;
    const TsdfTrilinear t = tsdf_trilinear(v, gx - (double)i, fy, fz);
    double g[3];
    tsdf_trilinear_gradient(v, t, fy, fz, g);
    const double gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    if (t.val >= TSDF_QUANT || !(gg > 0.0) || !isfinite(gg))   // truncated free space: the field is flat; (a NaN fails gg > 0)
        return false;
    r = (t.val / TSDF_QUANT) * a.front;
    const double scale = (a.front / TSDF_QUANT) / a.vol.s;
    const double o0 = g[0] * scale, o1 = g[1] * scale, o2 = g[2] * scale;      // the gradient in metres per metre, object frame
    const double n0 = (A[0] * o0 + A[1] * o1) + A[2] * o2;                     // n = R grad, camera frame, not normalised
    const double n1 = (A[4] * o0 + A[5] * o1) + A[6] * o2;
    const double n2 = (A[8] * o0 + A[9] * o1) + A[10] * o2;
    J[0] = -(p[1] * n2 - p[2] * n1);
    J[1] = -(p[2] * n0 - p[0] * n2);
    J[2] = -(p[0] * n1 - p[1] * n0);
    J[3] = -n0, J[4] = -n1, J[5] = -n2;
    return true;
}

__global__ __launch_bounds__(GN_BLOCK) void tsdf_align_sums_kernel(TsdfAlignArgs a)
{
    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f)                       // (the whole workgroup: no barrier has been reached)
        return;
    const int n = a.wh * a.ww;                     // window pixels of a sample
    const int q0 = tile * GN_RUN + tid * GN_PIX;   // the lane's first window pixel (may lie past n)
    const Pinhole<double> cam = pinhole<double>(a.intr_win + 5 * (size_t)s);
    const double *A = a.pose_in + 16 * (size_t)s;  // the same address in every lane: scalar loads
    const size_t frame = (size_t)fr * a.h * a.w;
    const unsigned short *pix = a.depth + frame;
    const long long u0 = a.origin[2 * s], v0 = a.origin[2 * s + 1];
    const int wanted = a.label != nullptr && a.want != nullptr ? a.want[fr] : 0;   // 0: every pixel with a depth

    double acc[GN_SUMS];
#pragma unroll
    for (int k = 0; k < GN_SUMS; ++k)
        acc[k] = 0.0;
    int count = 0;
    int y = q0 / a.ww, x = q0 - y * a.ww;
#pragma unroll 1
    for (int i = 0; i < GN_PIX; ++i) {
        if (q0 + i < n) {
            const int d = gn_depth(pix, a.h, a.w, u0 + x, v0 + y, 0);
            // (d != 0: the pixel lies inside the frame, so the label's index does too)
            if (d != 0 && (wanted == 0 || (int)a.label[frame + (size_t)(v0 + y) * a.w + (size_t)(u0 + x)] == wanted)) {
                double J[6], r;
                if (ta_row(a, cam, A, x, y, d, J, r)) {
                    ++count;
                    gn_add_row(acc, J, r);
                }
            }
        }
        if (++x == a.ww)
            x = 0, ++y;
    }
    gn_store_run(acc, count, (size_t)s * a.tiles + tile, a.part_sums, a.part_count);
}

// one wave per sample: lane k < 28 adds sum k of the sample's runs in run order, lane 28 the counts; lane 0 solves
__global__ __launch_bounds__(64) void tsdf_align_solve_kernel(int f, int tiles, const int *__restrict__ frame_of,
                                                             const double *__restrict__ part_sums,
                                                             const int *__restrict__ part_count,
                                                             const double *__restrict__ pose_in, int *__restrict__ n_pairs,
                                                             double *__restrict__ x_out, int *__restrict__ status,
                                                             double *__restrict__ pose_out)
{
    __shared__ double total[GN_SUMS];
    __shared__ int total_count;
    const int s = blockIdx.x, lane = threadIdx.x;
    const int fr = frame_of[s];
    const bool live = fr >= 0 && fr < f;               // (the whole wave)
    if (lane < GN_SUMS) {
        total[lane] = gn_add_runs(live, s, tiles, part_sums, GN_SUMS, lane);
    } else if (lane == GN_SUMS) {
        const int v = gn_add_runs(live, s, tiles, part_count, 1, 0);
        total_count = v;
        n_pairs[s] = v;
    }
    __syncthreads();
    if (lane != 0)
        return;
    double sm[GN_SUMS], x[6], U[12];
#pragma unroll
    for (int k = 0; k < GN_SUMS; ++k)
        sm[k] = total[k];
    int st = !live ? 4 : total_count < 6 ? 1 : 0;
    if (st == 0)
        st = gn_solve(sm, x, U);
    gn_write_update(s, st, x, U, pose_in, x_out, status, pose_out);
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API long long cloudaae_tsdf_align_step_workspace(int b, int wh, int ww)
{
    return gn_within_limits(1, 1, 1, b, wh, ww) ? gn_runs(b, wh, ww, nullptr).bytes : 0;
}

CLOUDAAE_API int cloudaae_tsdf_align_step(int nx, int ny, int nz, double ox, double oy, double oz, double voxel, const int *state,
                                          int min_count, double front, int f, int h, int w, const uint16_t *depth,
                                          const uint8_t *label, const int *want, int b, const int *frame_of, const int *origin,
                                          int wh, int ww, const float *intr_win, const double *pose_in, int *n_pairs, double *x,
                                          int *status, double *pose_out, void *workspace, long long workspace_size,
                                          cloudaae_stream_t stream)
{
    const char *name = "cloudaae_tsdf_align_step";
    CLOUDAAE_REQUIRE(tsdf_volume_ok(nx, ny, nz), name, TSDF_VOLUME_LIMITS);
    CLOUDAAE_REQUIRE(tsdf_frame_ok(ox, oy, oz, voxel), name, TSDF_FRAME_LIMITS);
    CLOUDAAE_REQUIRE(min_count >= 1, name, "min_count must be >= 1");
    CLOUDAAE_REQUIRE(isfinite(front) && front > 0.0, name, "front must be finite and > 0");
    CLOUDAAE_REQUIRE(gn_within_limits(f, h, w, b, wh, ww), name, CLOUDAAE_GN_LIMITS);
    CLOUDAAE_REQUIRE(state && depth && frame_of && origin && intr_win && pose_in && n_pairs && x && status && pose_out && workspace,
                     name, "null pointer");
    CLOUDAAE_REQUIRE(((uintptr_t)state & 15u) == 0, name, "the state must be 16-byte aligned");
    const GnRuns g = gn_runs(b, wh, ww, workspace);
    CLOUDAAE_REQUIRE(((uintptr_t)workspace & 7u) == 0 && workspace_size >= g.bytes, name,
                     "the workspace is smaller than cloudaae_tsdf_align_step_workspace or not 8-byte aligned");
    TsdfAlignArgs a;
    a.vol = TsdfVolume{nx, ny, nz, ox, oy, oz, voxel};
    a.state = (const int4 *)state, a.min_count = min_count, a.front = front;
    a.f = f, a.h = h, a.w = w, a.wh = wh, a.ww = ww;
    a.tiles = g.runs;
    a.depth = depth, a.label = label, a.want = want;
    a.frame_of = frame_of, a.origin = origin, a.intr_win = intr_win, a.pose_in = pose_in;
    a.part_sums = g.part_sums;
    a.part_count = g.part_count;
    hipStream_t sm = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_align_sums_kernel, dim3((unsigned)g.all), dim3(GN_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(tsdf_align_solve_kernel, dim3((unsigned)b), dim3(64), 0, sm, f, a.tiles, frame_of,
                       (const double *)a.part_sums, (const int *)a.part_count, pose_in, n_pairs, x, status, pose_out);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
