// depth_contour.hip -- the occluding-contour term of depth-image tracking (gfx950): the nearest observed depth edge of every
// window pixel, the rows that pull the rendered object's occluding edges onto them, and the solve of the plane sums of
// depth_align.hip and these rows together.  DESIGN.md, "Contours", is the definition; tests/contour_reference.py restates
// it in NumPy.  Integers where the definition has integers, fp64 otherwise on exactly widened values, un-fused (the file is
// compiled with -ffp-contract=off), in the order written here.
//
//   cloudaae_depth_edge_nearest   one launch.  A workgroup of 256 lanes takes a tile of 32 x 32 pixels of one sample's
//                                 window: it stages the frame's depth under the tile with a halo of R + 1 into LDS, forms
//                                 the edge masks of the tile with a halo of R, takes per row of that and column of the tile
//                                 the nearest edge within |i| <= R (the smaller i on a tie), and per pixel the smallest
//                                 (i i + j j, j) over the rows |j| <= R among those inside the disc.
//   cloudaae_depth_contour_sums   two launches, as cloudaae_depth_align_step: depth_contour_sums_kernel adds the 28 sums of a
//                                 run of 2048 window pixels, eight consecutive ones per lane, in pixel order, the u row
//                                 before the v row; depth_contour_finish_kernel adds a sample's runs in run order.
//   cloudaae_depth_align_solve    one launch, one wave per sample: plane + w contour, the LDL^T solve, U pose_in.
//
// Why the two passes give the nearest edge by the key (i i + j j, j, i): within a row j the key grows with |i|, so the row's
// best candidate is its edge of smallest |i|, the one at -|i| when both sides have one, and when that one lies outside the
// disc so do all others of the row; candidates of different rows differ in j, which comes before i.
//
// No floating-point atomic, no ticket, no workgroup waits for another: a sample's result is the same bits run to run and
// whatever else is in the batch.
//
// Here are the nearest map, the pairing of the rendered edges with it, the two contour rows and the total of the two terms.
// What the sums and the solve share with the plane step of depth_align.hip is in depth_gn.h: the limits and the launch shape
// (gn_within_limits, gn_runs), the bounds-checked depth load (gn_depth, here with -1 outside the image, which dc_open reads;
// the window's camera and its back-projection are depth_frame.h's), the 28 sums of a row (gn_add_row), the workgroup's reduction
// (gn_store_run), the sum over a sample's runs (gn_add_runs), the LDL^T solve with x -> U (gn_solve) and the write of
// U pose_in (gn_write_update): weight 0 gives the plane step's own pose because both run that one text.
#include "common.h"
#include "depth_gn.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

namespace cloudaae {

constexpr int DC_MAX_RADIUS = 32;

constexpr int EN_TILE = 32;                        // the nearest map's tile side
constexpr int EN_MASK_SIDE = EN_TILE + 2 * DC_MAX_RADIUS;      // tile + halo R, at the largest R
constexpr int EN_DEPTH_SIDE = EN_MASK_SIDE + 2;                // tile + halo R + 1
constexpr int EN_NONE = 127;                       // a row without an edge within R (R <= 32 < 127)

// ---- the nearest map --------------------------------------------------------------------------------------------------------
struct EdgeNearestArgs {
    int f, h, w, wh, ww, tiles_x, tiles_y, radius;
    const unsigned short *depth_test;
    const int *frame_of, *origin, *step;
    int *nearest;                                  // [b, wh, ww]
};

__global__ __launch_bounds__(GN_BLOCK) void depth_edge_nearest_kernel(EdgeNearestArgs a)
{
    __shared__ unsigned short zs[EN_DEPTH_SIDE * EN_DEPTH_SIDE];       // 19 208 B
    __shared__ unsigned char mask[EN_MASK_SIDE * EN_MASK_SIDE];        //  9 216 B
    __shared__ signed char row_near[EN_MASK_SIDE * EN_TILE];           //  3 072 B
    const int tid = threadIdx.x;
    const int per_sample = a.tiles_x * a.tiles_y;
    const int s = blockIdx.x / per_sample, rem = blockIdx.x - s * per_sample;
    const int x0 = (rem % a.tiles_x) * EN_TILE, y0 = (rem / a.tiles_x) * EN_TILE;    // the tile's first window pixel
    int *out = a.nearest + (size_t)s * a.wh * a.ww;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f) {                     // (the whole workgroup: no barrier has been reached)
        for (int e = tid; e < EN_TILE * EN_TILE; e += GN_BLOCK) {
            const int x = x0 + (e & (EN_TILE - 1)), y = y0 + e / EN_TILE;
            if (x < a.ww && y < a.wh)
                out[(size_t)y * a.ww + x] = -1;
        }
        return;
    }
    const int R = a.radius, step = a.step[s];
    const int side_m = EN_TILE + 2 * R, side_d = side_m + 2;
    const unsigned short *frame = a.depth_test + (size_t)fr * a.h * a.w;
    // frame pixel of entry (0, 0) of the staged depth; entry (c, r) of the masks is entry (c + 1, r + 1) of the depth
    const long long ud = (long long)a.origin[2 * s] + x0 - (R + 1), vd = (long long)a.origin[2 * s + 1] + y0 - (R + 1);

    for (int e = tid; e < side_d * side_d; e += GN_BLOCK) {
        const int r = e / side_d, c = e - r * side_d;
        const long long u = ud + c, v = vd + r;
        unsigned short z = 0;
        if (u >= 0 && u < a.w && v >= 0 && v < a.h)
            z = frame[(size_t)v * a.w + (size_t)u];
        zs[e] = z;
    }
    __syncthreads();
    for (int e = tid; e < side_m * side_m; e += GN_BLOCK) {
        const int r = e / side_m, c = e - r * side_m;
        const long long u = ud + c + 1, v = vd + r + 1;
        const int at = (r + 1) * side_d + (c + 1);
        const int z = (int)zs[at];
        int m = 0;
        if (z != 0) {                              // (a pixel outside the frame was staged as 0)
            const int zl = (int)zs[at - 1], zr = (int)zs[at + 1], zu = (int)zs[at - side_d], zb = (int)zs[at + side_d];
            m |= (u - 1 >= 0 && (zl == 0 || zl - z > step)) ? 1 : 0;
            m |= (u + 1 < a.w && (zr == 0 || zr - z > step)) ? 2 : 0;
            m |= (v - 1 >= 0 && (zu == 0 || zu - z > step)) ? 4 : 0;
            m |= (v + 1 < a.h && (zb == 0 || zb - z > step)) ? 8 : 0;
        }
        mask[e] = (unsigned char)m;
    }
    __syncthreads();
    for (int e = tid; e < side_m * EN_TILE; e += GN_BLOCK) {
        const int r = e / EN_TILE, c = e & (EN_TILE - 1);
        const unsigned char *row = mask + r * side_m + c + R;          // the pixel of column c itself
        int best = row[0] != 0 ? 0 : EN_NONE;
        for (int k = 1; k <= R && best == EN_NONE; ++k)
            best = row[-k] != 0 ? -k : row[k] != 0 ? k : EN_NONE;
        row_near[e] = (signed char)best;
    }
    __syncthreads();
    const int rr = R * R;
    for (int e = tid; e < EN_TILE * EN_TILE; e += GN_BLOCK) {
        const int y = e / EN_TILE, x = e & (EN_TILE - 1);
        if (x0 + x >= a.ww || y0 + y >= a.wh)
            continue;
        int best_d = rr + 1, best_i = 0, best_j = 0;
        for (int j = -R; j <= R; ++j) {            // ascending j: the smaller j wins a tie in the distance
            const int i = (int)row_near[(y + R + j) * EN_TILE + x];
            const int d = i * i + j * j;           // (EN_NONE squared is beyond every R R)
            if (d < best_d)
                best_d = d, best_i = i, best_j = j;
        }
        int code = -1;
        if (best_d <= rr)
            code = ((int)mask[(y + R + best_j) * side_m + x + R + best_i] << 16) | ((best_j + R) << 8) | (best_i + R);
        out[(size_t)(y0 + y) * a.ww + (x0 + x)] = code;
    }
}

// ---- the contour sums -------------------------------------------------------------------------------------------------------
// one bit of an edge mask: the neighbour lies inside the image (gn_depth gave no -1) and is empty or more than `step`
// farther than z
__device__ __forceinline__ bool dc_open(int z_nb, int z, int step)
{
    return z_nb >= 0 && (z_nb == 0 || z_nb - z > step);
}

struct ContourSumsArgs {
    int f, h, w, wh, ww, runs, radius;
    const unsigned short *depth_test, *depth_hyp;
    const int *frame_of, *origin, *gate, *step, *nearest;
    const float *intr_win;
    double *part_sums;                             // [b, runs, 28]
    int *part_rows;                                // [b, runs]
};

__global__ __launch_bounds__(GN_BLOCK) void depth_contour_sums_kernel(ContourSumsArgs a)
{
    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.runs, run = blockIdx.x % a.runs;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f)                       // (the whole workgroup: no barrier has been reached)
        return;
    const int n = a.wh * a.ww;                     // window pixels of a sample
    const int q0 = run * GN_RUN + tid * GN_PIX;    // the lane's first window pixel (may lie past n)
    const int gate = a.gate[s], step = a.step[s], R = a.radius;
    const Pinhole<double> cam = pinhole<double>(a.intr_win + 5 * (size_t)s);
    const unsigned short *hyp = a.depth_hyp + (size_t)s * n;
    const unsigned short *test = a.depth_test + (size_t)fr * a.h * a.w;
    const int *near = a.nearest + (size_t)s * n;
    const long long u0 = a.origin[2 * s], v0 = a.origin[2 * s + 1];

    double acc[GN_SUMS];
#pragma unroll
    for (int e = 0; e < GN_SUMS; ++e)
        acc[e] = 0.0;
    int rows = 0;
    int y = q0 / a.ww, x = q0 - y * a.ww;
#pragma unroll 1
    for (int px = 0; px < GN_PIX; ++px) {
        if (q0 + px < n) {
            const int d = (int)hyp[q0 + px];
            int m = 0;
            if (d != 0) {
                m |= dc_open(gn_depth(hyp, a.wh, a.ww, x - 1, y, -1), d, step) ? 1 : 0;
                m |= dc_open(gn_depth(hyp, a.wh, a.ww, x + 1, y, -1), d, step) ? 2 : 0;
                m |= dc_open(gn_depth(hyp, a.wh, a.ww, x, y - 1, -1), d, step) ? 4 : 0;
                m |= dc_open(gn_depth(hyp, a.wh, a.ww, x, y + 1, -1), d, step) ? 8 : 0;
            }
            const int code = m != 0 ? near[q0 + px] : -1;
            if (code >= 0 && (code >> 16) == m) {
                const int i = (code & 255) - R, j = ((code >> 8) & 255) - R;
                const int t = gn_depth(test, a.h, a.w, u0 + x + i, v0 + y + j, -1);  // (-1: a code that points outside the frame)
                const int diff = d - t, mag = diff < 0 ? -diff : diff;
                if (t >= 0 && mag <= gate) {
                    double p[3];
                    backproject(cam, x, y, d, p);
                    rows += 2;
#pragma unroll 1
                    for (int axis = 0; axis < 2; ++axis) {             // the u row, then the v row
                        const double off = axis == 0 ? -(double)i : -(double)j;
                        const double r = (off * p[2]) / (axis == 0 ? cam.fx : cam.fy);
                        const double g0 = axis == 0 ? 1.0 : 0.0, g1 = axis == 0 ? 0.0 : 1.0;
                        const double g2 = -((axis == 0 ? p[0] : p[1]) / p[2]);
                        double J[6];
                        J[0] = p[1] * g2 - p[2] * g1;
                        J[1] = p[2] * g0 - p[0] * g2;
                        J[2] = p[0] * g1 - p[1] * g0;
                        J[3] = g0, J[4] = g1, J[5] = g2;
                        gn_add_row(acc, J, r);
                    }
                }
            }
        }
        if (++x == a.ww)
            x = 0, ++y;
    }
    gn_store_run(acc, rows, (size_t)s * a.runs + run, a.part_sums, a.part_rows);
}

// one wave per sample: lane k < 28 adds sum k of the sample's runs in run order, lane 28 the rows
__global__ __launch_bounds__(64) void depth_contour_finish_kernel(int f, int runs, const int *__restrict__ frame_of,
                                                                 const double *__restrict__ part_sums,
                                                                 const int *__restrict__ part_rows, int *__restrict__ n_rows,
                                                                 double *__restrict__ sums)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const int fr = frame_of[s];
    const bool live = fr >= 0 && fr < f;               // (the whole wave)
    if (lane < GN_SUMS)
        sums[(size_t)s * GN_SUMS + lane] = gn_add_runs(live, s, runs, part_sums, GN_SUMS, lane);
    else if (lane == GN_SUMS)
        n_rows[s] = gn_add_runs(live, s, runs, part_rows, 1, 0);
}

// ---- the combined solve -----------------------------------------------------------------------------------------------------
// one wave per sample: lane k < 28 forms plane[k] + w contour[k]; lane 0 decides the status, solves and writes the pose
__global__ __launch_bounds__(64) void depth_align_combined_solve_kernel(const double *__restrict__ plane_sums,
                                                                       const int *__restrict__ n_pairs,
                                                                       const int *__restrict__ plane_status,
                                                                       const double *__restrict__ contour_sums,
                                                                       const int *__restrict__ n_rows, double weight,
                                                                       const double *__restrict__ pose_in,
                                                                       double *__restrict__ x_out, int *__restrict__ status,
                                                                       double *__restrict__ pose_out)
{
    __shared__ double total[GN_SUMS];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (lane < GN_SUMS)
        total[lane] = plane_sums[(size_t)s * GN_SUMS + lane] + weight * contour_sums[(size_t)s * GN_SUMS + lane];
    __syncthreads();
    if (lane != 0)
        return;
    double sm[GN_SUMS], x[6], U[12];
#pragma unroll
    for (int k = 0; k < GN_SUMS; ++k)
        sm[k] = total[k];
    int st = plane_status[s] == 4 ? 4 : (long long)n_pairs[s] + (long long)n_rows[s] < 6 ? 1 : 0;
    if (st == 0)
        st = gn_solve(sm, x, U);
    gn_write_update(s, st, x, U, pose_in, x_out, status, pose_out);
}

static const char *const DC_LIMITS = CLOUDAAE_GN_LIMITS "; 1 <= radius <= 32";

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_depth_edge_nearest(int f, int h, int w, const uint16_t *depth_test, int b, const int *frame_of,
                                             const int *origin, int wh, int ww, const int *step, int radius, int *nearest,
                                             cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_edge_nearest";
    CLOUDAAE_REQUIRE(gn_within_limits(f, h, w, b, wh, ww) && radius >= 1 && radius <= DC_MAX_RADIUS, name, DC_LIMITS);
    CLOUDAAE_REQUIRE(depth_test && frame_of && origin && step && nearest, name, "null pointer");
    EdgeNearestArgs a;
    a.f = f, a.h = h, a.w = w, a.wh = wh, a.ww = ww, a.radius = radius;
    a.tiles_x = ceil_div(ww, EN_TILE), a.tiles_y = ceil_div(wh, EN_TILE);
    a.depth_test = depth_test;
    a.frame_of = frame_of, a.origin = origin, a.step = step;
    a.nearest = nearest;
    // b * tiles <= b * (wh + 31) * (ww + 31) / 1024 < 2^28 + b: below the grid limit
    const long long blocks = (long long)b * a.tiles_x * a.tiles_y;
    hipLaunchKernelGGL(depth_edge_nearest_kernel, dim3((unsigned)blocks), dim3(GN_BLOCK), 0, (hipStream_t)stream, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API long long cloudaae_depth_contour_sums_workspace_bytes(int b, int wh, int ww)
{
    return gn_within_limits(1, 1, 1, b, wh, ww) ? gn_runs(b, wh, ww, nullptr).bytes : 0;
}

CLOUDAAE_API int cloudaae_depth_contour_sums(int f, int h, int w, const uint16_t *depth_test, int b, const int *frame_of,
                                             const int *origin, int wh, int ww, const uint16_t *depth_hyp, const float *intr_win,
                                             const int *gate, const int *step, int radius, const int *nearest, int *n_rows,
                                             double *sums, void *workspace, long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_contour_sums";
    CLOUDAAE_REQUIRE(gn_within_limits(f, h, w, b, wh, ww) && radius >= 1 && radius <= DC_MAX_RADIUS, name, DC_LIMITS);
    CLOUDAAE_REQUIRE(depth_test && frame_of && origin && depth_hyp && intr_win && gate && step && nearest && n_rows && sums &&
                         workspace,
                     name, "null pointer");
    const GnRuns g = gn_runs(b, wh, ww, workspace);
    CLOUDAAE_REQUIRE(((uintptr_t)workspace & 7u) == 0 && workspace_bytes >= g.bytes, name,
                     "the workspace is smaller than cloudaae_depth_contour_sums_workspace_bytes or not 8-byte aligned");
    ContourSumsArgs a;
    a.f = f, a.h = h, a.w = w, a.wh = wh, a.ww = ww, a.radius = radius;
    a.runs = g.runs;
    a.depth_test = depth_test, a.depth_hyp = depth_hyp;
    a.frame_of = frame_of, a.origin = origin, a.gate = gate, a.step = step, a.nearest = nearest;
    a.intr_win = intr_win;
    a.part_sums = g.part_sums;
    a.part_rows = g.part_count;
    hipStream_t sm = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_contour_sums_kernel, dim3((unsigned)g.all), dim3(GN_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(depth_contour_finish_kernel, dim3((unsigned)b), dim3(64), 0, sm, f, a.runs, frame_of,
                       (const double *)a.part_sums, (const int *)a.part_rows, n_rows, sums);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_depth_align_solve(int b, const double *plane_sums, const int *n_pairs, const int *plane_status,
                                            const double *contour_sums, const int *n_rows, double weight, const double *pose_in,
                                            double *x, int *status, double *pose_out, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_align_solve";
    CLOUDAAE_REQUIRE(b >= 1 && b <= FRAME_MAX_TOTAL, name, "outside the limits: 1 <= b <= 2^28");
    CLOUDAAE_REQUIRE(!isnan(weight), name, "weight must be a number");
    CLOUDAAE_REQUIRE(plane_sums && n_pairs && plane_status && contour_sums && n_rows && pose_in && x && status && pose_out, name,
                     "null pointer");
    hipLaunchKernelGGL(depth_align_combined_solve_kernel, dim3((unsigned)b), dim3(64), 0, (hipStream_t)stream, plane_sums, n_pairs,
                       plane_status, contour_sums, n_rows, weight, pose_in, x, status, pose_out);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
