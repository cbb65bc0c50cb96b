// depth_align.hip -- one Gauss-Newton step of dense depth-image alignment for b tracks: the object rendered at the
// predicted pose into a window of wh x ww pixels is paired, pixel by pixel, with the depth the camera saw at the same
// pixel, and one point-to-plane update is solved from the pairs (gfx950).  DESIGN.md, "Tracking", is the definition;
// tests/track_reference.py restates it in NumPy.  Everything is fp64 on exactly widened integers and fp32 values,
// un-fused (the file is compiled with -ffp-contract=off), in the order written here.
//
//   cloudaae_depth_align_step   two launches.  depth_align_sums_kernel: a workgroup of 256 lanes takes a run of 2048
//                               window pixels of one sample, eight CONSECUTIVE ones per lane.  A lane adds the 28 sums of
//                               its pairs in pixel order, the wave reduces by a butterfly, the four waves add in order
//                               through LDS, and the workgroup stores its 28 partial sums and its count to the
//                               workspace.  depth_align_solve_kernel: one wave per sample adds the runs in run order,
//                               solves the 6 x 6 system by LDL^T and writes U pose_in.
//
// No floating-point atomic, no ticket, no workgroup waits for another: a sample's result is the same bits run to run and
// whatever else is in the batch.  The ten depth taps of a pair (the pixel and its four neighbours in either image) are
// plain loads, as in depth_noise.hip: neighbouring lanes share their cache lines.
//
// Here are the pairing, the normals of the two depth images and the plane row.  What the step shares with the contour term
// of depth_contour.hip is in depth_gn.h: the limits and the launch shape (gn_within_limits, gn_runs), the bounds-checked
// depth load (gn_depth; the window's camera and its back-projection are depth_frame.h's), the 28 sums of a row (gn_add_row), the workgroup's
// reduction (gn_store_run), the sum over a sample's runs (gn_add_runs), the LDL^T solve with x -> U (gn_solve) and the
// write of U pose_in (gn_write_update).  icp_plane_update of icp.hip restates that factorisation on its own layout of sums.
#include "common.h"
#include "depth_gn.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

namespace cloudaae {

// An image addressed by WINDOW coordinates: window pixel (x, y) is image pixel (x + ox, y + oy) of an image [h, w].
// The hypothesis image is the window itself (ox = oy = 0, h = wh, w = ww); the test image is the frame (ox = u0, oy = v0).
struct DaImage {
    const unsigned short *pix;
    int h, w;
    long long ox, oy;
};

// the depth at window pixel (x, y); 0 where that is no pixel of the image
__device__ __forceinline__ int da_depth(const DaImage &im, int x, int y)
{
    return gn_depth(im.pix, im.h, im.w, im.ox + x, im.oy + y, 0);
}

// the neighbour (x, y) of a pixel of depth zs: valid when inside the image, with depth, and within `jump` units of zs
__device__ __forceinline__ bool da_tap(const DaImage &im, const Pinhole<double> &c, int x, int y, int zs, int jump, double (&p)[3])
{
    const int z = da_depth(im, x, y);
    const int diff = z - zs, mag = diff < 0 ? -diff : diff;
    if (z == 0 || mag > jump)
        return false;
    backproject(c, x, y, z, p);
    return true;
}

// the difference along one axis: central when both neighbours are valid, one-sided with the valid one, else none
__device__ __forceinline__ bool da_axis(const DaImage &im, const Pinhole<double> &c, int x, int y, int dx, int dy, int zs, int jump,
                                       const double (&centre)[3], double (&g)[3])
{
    double lo[3], hi[3];
    const bool vlo = da_tap(im, c, x - dx, y - dy, zs, jump, lo), vhi = da_tap(im, c, x + dx, y + dy, zs, jump, hi);
    if (!vlo && !vhi)
        return false;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        g[k] = (vhi ? hi[k] : centre[k]) - (vlo ? lo[k] : centre[k]);
    return true;
}

// The unsigned unit normal of the image at window pixel (x, y), whose depth zs is not 0 and whose point is `centre`.
// false: the pixel is flat.
__device__ __forceinline__ bool da_normal(const DaImage &im, const Pinhole<double> &c, int x, int y, int zs, int jump,
                                         const double (&centre)[3], double (&n)[3])
{
    double gx[3], gy[3];
    const bool hx = da_axis(im, c, x, y, 1, 0, zs, jump, centre, gx), hy = da_axis(im, c, x, y, 0, 1, zs, jump, centre, gy);
    if (!hx || !hy)
        return false;
    double v[3];
    v[0] = gx[1] * gy[2] - gx[2] * gy[1];
    v[1] = gx[2] * gy[0] - gx[0] * gy[2];
    v[2] = gx[0] * gy[1] - gx[1] * gy[0];
    const double nn = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (!(nn > 0.0) || !isfinite(nn))              // (a NaN fails the first comparison)
        return false;
    const double len = sqrt(nn);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        n[k] = v[k] / len;
    return true;
}

struct DepthAlignArgs {
    int f, h, w, wh, ww, tiles;
    const unsigned short *depth_test, *depth_hyp;
    const int *frame_of, *origin, *gate, *jump;
    const float *intr_win;
    double cos_min;
    double *part_sums;                             // [b, tiles, 28]
    int *part_count;                               // [b, tiles]
};

__global__ __launch_bounds__(GN_BLOCK) void depth_align_sums_kernel(DepthAlignArgs a)
{
    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f)                       // (the whole workgroup: no barrier has been reached)
        return;
    const int n = a.wh * a.ww;                     // window pixels of a sample
    const int q0 = tile * GN_RUN + tid * GN_PIX;   // the lane's first window pixel (may lie past n)
    const int gate = a.gate[s], jump = a.jump[s];
    const bool use_normals = a.cos_min > 0.0;
    const Pinhole<double> cam = pinhole<double>(a.intr_win + 5 * (size_t)s);
    DaImage hyp, test;
    hyp.pix = a.depth_hyp + (size_t)s * n;
    hyp.h = a.wh, hyp.w = a.ww, hyp.ox = 0, hyp.oy = 0;
    test.pix = a.depth_test + (size_t)fr * a.h * a.w;
    test.h = a.h, test.w = a.w, test.ox = a.origin[2 * s], test.oy = a.origin[2 * s + 1];

    double acc[GN_SUMS];
#pragma unroll
    for (int k = 0; k < GN_SUMS; ++k)
        acc[k] = 0.0;
    int count = 0;
    int y = q0 / a.ww, x = q0 - y * a.ww;
#pragma unroll 1
    for (int i = 0; i < GN_PIX; ++i) {
        if (q0 + i < n) {
            const int d = (int)hyp.pix[q0 + i];
            const int t = d != 0 ? da_depth(test, x, y) : 0;
            const int diff = d - t, mag = diff < 0 ? -diff : diff;
            if (d != 0 && t != 0 && mag <= gate) {
                double p[3], q[3], nh[3], mo[3];
                backproject(cam, x, y, d, p);
                backproject(cam, x, y, t, q);
                bool pair = da_normal(hyp, cam, x, y, d, jump, p, nh);
                if (pair && use_normals) {
                    pair = da_normal(test, cam, x, y, t, jump, q, mo);
                    if (pair)
                        pair = fabs((nh[0] * mo[0] + nh[1] * mo[1]) + nh[2] * mo[2]) >= a.cos_min;
                }
                if (pair) {
                    const double ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
                    const double r = (ex * nh[0] + ey * nh[1]) + ez * nh[2];
                    double J[6];
                    J[0] = p[1] * nh[2] - p[2] * nh[1];
                    J[1] = p[2] * nh[0] - p[0] * nh[2];
                    J[2] = p[0] * nh[1] - p[1] * nh[0];
                    J[3] = nh[0], J[4] = nh[1], J[5] = nh[2];
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
__global__ __launch_bounds__(64) void depth_align_solve_kernel(int f, int tiles, const int *__restrict__ frame_of,
                                                              const double *__restrict__ part_sums,
                                                              const int *__restrict__ part_count,
                                                              const double *__restrict__ pose_in, int *__restrict__ n_pairs,
                                                              double *__restrict__ sums, double *__restrict__ x_out,
                                                              int *__restrict__ status, double *__restrict__ pose_out)
{
    __shared__ double total[GN_SUMS];
    __shared__ int total_count;
    const int s = blockIdx.x, lane = threadIdx.x;
    const int fr = frame_of[s];
    const bool live = fr >= 0 && fr < f;               // (the whole wave)
    if (lane < GN_SUMS) {
        const double v = gn_add_runs(live, s, tiles, part_sums, GN_SUMS, lane);
        total[lane] = v;
        sums[(size_t)s * GN_SUMS + lane] = v;
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

CLOUDAAE_API long long cloudaae_depth_align_step_workspace_bytes(int b, int wh, int ww)
{
    return gn_within_limits(1, 1, 1, b, wh, ww) ? gn_runs(b, wh, ww, nullptr).bytes : 0;
}

CLOUDAAE_API int cloudaae_depth_align_step(int f, int h, int w, const uint16_t *depth_test, int b, const int *frame_of,
                                           const int *origin, int wh, int ww, const uint16_t *depth_hyp, const float *intr_win,
                                           const int *gate, const int *jump, double cos_min, const double *pose_in,
                                           int *n_pairs, double *sums, double *x, int *status, double *pose_out,
                                           void *workspace, long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_align_step";
    CLOUDAAE_REQUIRE(gn_within_limits(f, h, w, b, wh, ww), name, CLOUDAAE_GN_LIMITS);
    CLOUDAAE_REQUIRE(!isnan(cos_min), name, "cos_min must be a number");
    CLOUDAAE_REQUIRE(depth_test && frame_of && origin && depth_hyp && intr_win && gate && jump && pose_in && n_pairs && sums &&
                         x && status && pose_out && workspace,
                     name, "null pointer");
    const GnRuns g = gn_runs(b, wh, ww, workspace);
    CLOUDAAE_REQUIRE(((uintptr_t)workspace & 7u) == 0 && workspace_bytes >= g.bytes, name,
                     "the workspace is smaller than cloudaae_depth_align_step_workspace_bytes or not 8-byte aligned");
    DepthAlignArgs a;
    a.f = f, a.h = h, a.w = w, a.wh = wh, a.ww = ww;
    a.tiles = g.runs;
    a.depth_test = depth_test, a.depth_hyp = depth_hyp;
    a.frame_of = frame_of, a.origin = origin, a.gate = gate, a.jump = jump;
    a.intr_win = intr_win;
    a.cos_min = cos_min;
    a.part_sums = g.part_sums;
    a.part_count = g.part_count;
    hipStream_t sm = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_align_sums_kernel, dim3((unsigned)g.all), dim3(GN_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(depth_align_solve_kernel, dim3((unsigned)b), dim3(64), 0, sm, f, a.tiles, frame_of,
                       (const double *)a.part_sums, (const int *)a.part_count, pose_in, n_pairs, sums, x, status, pose_out);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
