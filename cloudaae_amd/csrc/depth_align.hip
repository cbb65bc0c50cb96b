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
// plain loads, as in depth_noise.hip: neighbouring lanes share their cache lines.  The LDL^T solve and x -> U restate
// icp_plane_update of icp.hip; the product U pose_in is formed as cloudaae_pose_compose forms its products.
#include "common.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

namespace cloudaae {

constexpr long long DA_MAX_PIXELS = 1ll << 24;     // h w, wh ww
constexpr long long DA_MAX_TOTAL = 1ll << 28;      // b wh ww

constexpr int DA_BLOCK = 256;
constexpr int DA_WAVES = DA_BLOCK / 64;
constexpr int DA_PIX = 8;                          // consecutive window pixels of a lane
constexpr int DA_TILE = DA_BLOCK * DA_PIX;         // window pixels of a workgroup
constexpr int DA_SUMS = 28;                        // sum r^2, A's upper triangle by rows (21), b (6)

// The window's camera: the row (fx, fy, cx - u0, cy - v0, factor_depth), widened
struct DaCam {
    double fx, fy, cx, cy, factor;
};

// An image addressed by WINDOW coordinates: window pixel (x, y) is image pixel (x + ox, y + oy) of an image [h, w].
// The hypothesis image is the window itself (ox = oy = 0, h = wh, w = ww); the test image is the frame (ox = u0, oy = v0).
struct DaImage {
    const unsigned short *pix;
    int h, w;
    long long ox, oy;
};

// the depth at window pixel (x, y); 0 where that is no pixel of the image (nothing is read there)
__device__ __forceinline__ int da_depth(const DaImage &im, int x, int y)
{
    const long long u = im.ox + x, v = im.oy + y;
    if (u < 0 || u >= im.w || v < 0 || v >= im.h)
        return 0;
    return (int)im.pix[(size_t)v * im.w + (size_t)u];
}

// P(x, y, z) = (((x - cxw) dm) / fx, ((y - cyw) dm) / fy, dm) with dm = z / factor_depth
__device__ __forceinline__ void da_backproject(const DaCam &c, int x, int y, int z, double (&p)[3])
{
    const double dm = (double)z / c.factor;
    p[0] = (((double)x - c.cx) * dm) / c.fx;
    p[1] = (((double)y - c.cy) * dm) / c.fy;
    p[2] = dm;
}

// the neighbour (x, y) of a pixel of depth zs: valid when inside the image, with depth, and within `jump` units of zs
__device__ __forceinline__ bool da_tap(const DaImage &im, const DaCam &c, int x, int y, int zs, int jump, double (&p)[3])
{
    const int z = da_depth(im, x, y);
    const int diff = z - zs, mag = diff < 0 ? -diff : diff;
    if (z == 0 || mag > jump)
        return false;
    da_backproject(c, x, y, z, p);
    return true;
}

// the difference along one axis: central when both neighbours are valid, one-sided with the valid one, else none
__device__ __forceinline__ bool da_axis(const DaImage &im, const DaCam &c, int x, int y, int dx, int dy, int zs, int jump,
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
__device__ __forceinline__ bool da_normal(const DaImage &im, const DaCam &c, int x, int y, int zs, int jump,
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

__global__ __launch_bounds__(DA_BLOCK) void depth_align_sums_kernel(DepthAlignArgs a)
{
    __shared__ double red[DA_WAVES][DA_SUMS];
    __shared__ int red_count[DA_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f)                       // (the whole workgroup: no barrier has been reached)
        return;
    const int n = a.wh * a.ww;                     // window pixels of a sample
    const int q0 = tile * DA_TILE + tid * DA_PIX;  // the lane's first window pixel (may lie past n)
    const int gate = a.gate[s], jump = a.jump[s];
    const bool use_normals = a.cos_min > 0.0;
    DaCam cam;
    {
        const float *k = a.intr_win + 5 * (size_t)s;
        cam.fx = (double)k[0], cam.fy = (double)k[1], cam.cx = (double)k[2], cam.cy = (double)k[3], cam.factor = (double)k[4];
    }
    DaImage hyp, test;
    hyp.pix = a.depth_hyp + (size_t)s * n;
    hyp.h = a.wh, hyp.w = a.ww, hyp.ox = 0, hyp.oy = 0;
    test.pix = a.depth_test + (size_t)fr * a.h * a.w;
    test.h = a.h, test.w = a.w, test.ox = a.origin[2 * s], test.oy = a.origin[2 * s + 1];

    double acc[DA_SUMS];
#pragma unroll
    for (int k = 0; k < DA_SUMS; ++k)
        acc[k] = 0.0;
    int count = 0;
    int y = q0 / a.ww, x = q0 - y * a.ww;
#pragma unroll 1
    for (int i = 0; i < DA_PIX; ++i) {
        if (q0 + i < n) {
            const int d = (int)hyp.pix[q0 + i];
            const int t = d != 0 ? da_depth(test, x, y) : 0;
            const int diff = d - t, mag = diff < 0 ? -diff : diff;
            if (d != 0 && t != 0 && mag <= gate) {
                double p[3], q[3], nh[3], mo[3];
                da_backproject(cam, x, y, d, p);
                da_backproject(cam, x, y, t, q);
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
                    acc[0] += r * r;
                    int e = 1;
#pragma unroll
                    for (int g = 0; g < 6; ++g)
#pragma unroll
                        for (int c = g; c < 6; ++c)
                            acc[e++] += J[g] * J[c];
#pragma unroll
                    for (int g = 0; g < 6; ++g)
                        acc[22 + g] += J[g] * r;
                }
            }
        }
        if (++x == a.ww)
            x = 0, ++y;
    }
#pragma unroll
    for (int k = 0; k < DA_SUMS; ++k)
        acc[k] = wave_sum(acc[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        count += __shfl_xor(count, off, 64);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DA_SUMS; ++k)
            red[wv][k] = acc[k];
        red_count[wv] = count;
    }
    __syncthreads();
    const size_t run = (size_t)s * a.tiles + tile;
    if (tid < DA_SUMS) {
        double v = red[0][tid];
#pragma unroll
        for (int k = 1; k < DA_WAVES; ++k)
            v += red[k][tid];
        a.part_sums[run * DA_SUMS + tid] = v;
    } else if (tid == DA_SUMS) {
        int v = red_count[0];
#pragma unroll
        for (int k = 1; k < DA_WAVES; ++k)
            v += red_count[k];
        a.part_count[run] = v;
    }
}

// A x = -b by LDL^T without pivoting on the sums s = (sum r^2, A's upper triangle by rows, b); x = (alpha, beta, gamma, t);
// U = [Rz(gamma) Ry(beta) Rx(alpha) | t] (3 x 4).  -> 0, or 2 for a pivot that is not a finite number > 0, 3 for a
// solution with a component that is not finite.  Every loop is unrolled: the arrays stay in registers.
__device__ __forceinline__ int da_solve(const double (&s)[DA_SUMS], double (&x)[6], double (&U)[12])
{
    double A[6][6], L[6][6], d[6];
    {
        int e = 1;
#pragma unroll
        for (int g = 0; g < 6; ++g)
#pragma unroll
            for (int c = g; c < 6; ++c) {
                A[g][c] = s[e];
                A[c][g] = s[e];
                ++e;
            }
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k)
            dj -= (L[j][k] * L[j][k]) * d[k];
        bad = bad || !(dj > 0.0) || !isfinite(dj);     // (the first bad pivot decides; what follows it is not used)
        d[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k)
                v -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = v / dj;
        }
    }
    if (bad)
        return 2;
#pragma unroll
    for (int i = 0; i < 6; ++i) {                      // L y = -b
        double v = -s[22 + i];
#pragma unroll
        for (int k = 0; k < i; ++k)
            v -= L[i][k] * x[k];
        x[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)                        // D z = y
        x[i] = x[i] / d[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {                     // L^T x = z
        double v = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k)
            v -= L[k][i] * x[k];
        x[i] = v;
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        finite = finite && isfinite(x[i]);
    if (!finite)
        return 3;
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    U[0] = cg * cb;
    U[1] = (cg * sb) * sa - sg * ca;
    U[2] = (cg * sb) * ca + sg * sa;
    U[3] = x[3];
    U[4] = sg * cb;
    U[5] = (sg * sb) * sa + cg * ca;
    U[6] = (sg * sb) * ca - cg * sa;
    U[7] = x[4];
    U[8] = -sb;
    U[9] = cb * sa;
    U[10] = cb * ca;
    U[11] = x[5];
    return 0;
}

// one wave per sample: lane k < 28 adds sum k of the sample's runs in run order, lane 28 the counts; lane 0 solves
__global__ __launch_bounds__(64) void depth_align_solve_kernel(int f, int tiles, const int *__restrict__ frame_of,
                                                              const double *__restrict__ part_sums,
                                                              const int *__restrict__ part_count,
                                                              const double *__restrict__ pose_in, int *__restrict__ n_pairs,
                                                              double *__restrict__ sums, double *__restrict__ x_out,
                                                              int *__restrict__ status, double *__restrict__ pose_out)
{
    __shared__ double total[DA_SUMS];
    __shared__ int total_count;
    const int s = blockIdx.x, lane = threadIdx.x;
    const int fr = frame_of[s];
    const bool live = fr >= 0 && fr < f;               // (the whole wave)
    if (lane < DA_SUMS) {
        double v = 0.0;
        if (live)
            for (int r = 0; r < tiles; ++r)
                v += part_sums[((size_t)s * tiles + r) * DA_SUMS + lane];
        total[lane] = v;
        sums[(size_t)s * DA_SUMS + lane] = v;
    } else if (lane == DA_SUMS) {
        int v = 0;
        if (live)
            for (int r = 0; r < tiles; ++r)
                v += part_count[(size_t)s * tiles + r];
        total_count = v;
        n_pairs[s] = v;
    }
    __syncthreads();
    if (lane != 0)
        return;
    double sm[DA_SUMS], x[6], U[12];
#pragma unroll
    for (int k = 0; k < DA_SUMS; ++k)
        sm[k] = total[k];
    int st = !live ? 4 : total_count < 6 ? 1 : 0;
    if (st == 0)
        st = da_solve(sm, x, U);
    const double *T = pose_in + 16 * (size_t)s;
    double *out = pose_out + 16 * (size_t)s;
    status[s] = st;
    if (st != 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            x_out[6 * (size_t)s + k] = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            out[k] = T[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        x_out[6 * (size_t)s + k] = x[k];
#pragma unroll
    for (int row = 0; row < 3; ++row) {
        const double u0 = U[4 * row + 0], u1 = U[4 * row + 1], u2 = U[4 * row + 2], u3 = U[4 * row + 3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[4 * row + c] = (u0 * T[c] + u1 * T[4 + c]) + u2 * T[8 + c];
        out[4 * row + 3] = ((u0 * T[3] + u1 * T[7]) + u2 * T[11]) + u3;
    }
    out[12] = out[13] = out[14] = 0.0;
    out[15] = 1.0;
}

static bool da_within_limits(long long f, long long h, long long w, long long b, long long wh, long long ww)
{
    return f >= 1 && h >= 1 && w >= 1 && b >= 1 && wh >= 1 && ww >= 1 && h * w <= DA_MAX_PIXELS && wh * ww <= DA_MAX_PIXELS &&
           b * (wh * ww) <= DA_MAX_TOTAL;
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API long long cloudaae_depth_align_step_workspace_bytes(int b, int wh, int ww)
{
    if (!da_within_limits(1, 1, 1, b, wh, ww))
        return 0;
    const long long runs = (long long)b * ceil_div((long long)wh * ww, DA_TILE);
    return runs * (long long)(DA_SUMS * sizeof(double)) + (runs * (long long)sizeof(int) + 7) / 8 * 8;
}

CLOUDAAE_API int cloudaae_depth_align_step(int f, int h, int w, const uint16_t *depth_test, int b, const int *frame_of,
                                           const int *origin, int wh, int ww, const uint16_t *depth_hyp, const float *intr_win,
                                           const int *gate, const int *jump, double cos_min, const double *pose_in,
                                           int *n_pairs, double *sums, double *x, int *status, double *pose_out,
                                           void *workspace, long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_align_step";
    CLOUDAAE_REQUIRE(da_within_limits(f, h, w, b, wh, ww), name,
                     "outside the limits: f, h, w, b, wh, ww >= 1; h * w <= 2^24; wh * ww <= 2^24; b * wh * ww <= 2^28");
    CLOUDAAE_REQUIRE(!isnan(cos_min), name, "cos_min must be a number");
    CLOUDAAE_REQUIRE(depth_test && frame_of && origin && depth_hyp && intr_win && gate && jump && pose_in && n_pairs && sums &&
                         x && status && pose_out && workspace,
                     name, "null pointer");
    CLOUDAAE_REQUIRE(((uintptr_t)workspace & 7u) == 0 && workspace_bytes >= cloudaae_depth_align_step_workspace_bytes(b, wh, ww),
                     name, "the workspace is smaller than cloudaae_depth_align_step_workspace_bytes or not 8-byte aligned");
    DepthAlignArgs a;
    a.f = f, a.h = h, a.w = w, a.wh = wh, a.ww = ww;
    a.tiles = ceil_div((long long)wh * ww, DA_TILE);
    a.depth_test = depth_test, a.depth_hyp = depth_hyp;
    a.frame_of = frame_of, a.origin = origin, a.gate = gate, a.jump = jump;
    a.intr_win = intr_win;
    a.cos_min = cos_min;
    const long long runs = (long long)b * a.tiles;
    a.part_sums = (double *)workspace;
    a.part_count = (int *)(a.part_sums + runs * DA_SUMS);
    hipStream_t sm = (hipStream_t)stream;
    // b * tiles <= 2^28 / 2048 + b: below the grid limit
    hipLaunchKernelGGL(depth_align_sums_kernel, dim3((unsigned)runs), dim3(DA_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(depth_align_solve_kernel, dim3((unsigned)b), dim3(64), 0, sm, f, a.tiles, frame_of,
                       (const double *)a.part_sums, (const int *)a.part_count, pose_in, n_pairs, sums, x, status, pose_out);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
