// depth_gn.h -- what the two terms of depth-image tracking share: the point-to-plane step (depth_align.hip) and the
// occluding-contour term with the combined solve (depth_contour.hip) both add rows (J[6], r) of one Gauss-Newton system into
// 28 sums per run of 2048 window pixels, add a sample's runs in run order, and solve the 6 x 6 system for the pose update.
// Here are the limits and the launch shape, the workspace's layout, the row accumulation, the
// workgroup's reduction, the sum over a sample's runs, the LDL^T solve and the write of the updated pose.  DESIGN.md,
// "Tracking" and "Contours", are the definitions.  Both includers are compiled un-fused (-ffp-contract=off) and without
// packed fp32, so this text gives the same bits in both.  One restatement of the factorisation remains: icp_plane_update of
// icp.hip, on another layout of the sums.
#pragma once
#include "common.h"
#include "depth_frame.h"
#include "workspace.h"

#include <math.h>

namespace cloudaae {

constexpr int GN_BLOCK = 256;
constexpr int GN_WAVES = GN_BLOCK / 64;
constexpr int GN_PIX = 8;                          // consecutive window pixels of a lane
constexpr int GN_RUN = GN_BLOCK * GN_PIX;          // window pixels of a workgroup of a sums kernel
constexpr int GN_SUMS = 28;                        // sum r^2, A's upper triangle by rows (21), b (6)

#define CLOUDAAE_GN_LIMITS "outside the limits: f, h, w, b, wh, ww >= 1; h * w <= 2^24; wh * ww <= 2^24; b * wh * ww <= 2^28"

static inline bool gn_within_limits(long long f, long long h, long long w, long long b, long long wh, long long ww)
{
    // (f frames are indexed, only b windows are read: the frames' total has no limit, one frame's pixels have)
    return f >= 1 && frame_within_limits(1, 1, h, w) && frame_within_limits(1, b, wh, ww);
}

// The runs of b windows of wh x ww pixels and where their partial results lie in a workspace: part_sums [b, runs, 28]
// doubles, then part_count [b, runs] ints, padded to 8 bytes.  (workspace may be null: the size alone is asked for.)
struct GnRuns {
    int runs;                                      // of one sample
    long long all;                                 // b runs: the sums kernel's grid, <= 2^28 / 2048 + b, below the grid limit
    long long bytes;                               // of the workspace
    double *part_sums;
    int *part_count;
};

static inline GnRuns gn_runs(int b, int wh, int ww, void *workspace)
{
    GnRuns g;
    g.runs = ceil_div((long long)wh * ww, GN_RUN);
    g.all = (long long)b * g.runs;
    Carver ws(workspace);
    g.part_sums = ws.take<double>((size_t)g.all * GN_SUMS, 8);
    g.part_count = ws.take<int>((size_t)g.all, 8);
    g.bytes = (long long)ws.bytes();
    return g;
}

// (the window's camera is depth_frame.h's Pinhole<double> of the row (fx, fy, cx - u0, cy - v0, factor_depth))

// the depth of image [h, w] at pixel (u, v); `outside` where that is no pixel of the image (nothing is read there)
__device__ __forceinline__ int gn_depth(const unsigned short *pix, int h, int w, long long u, long long v, int outside)
{
    if (u < 0 || u >= w || v < 0 || v >= h)
        return outside;
    return (int)pix[(size_t)v * w + (size_t)u];
}

// one row (J, r) into the sums
__device__ __forceinline__ void gn_add_row(double (&acc)[GN_SUMS], const double (&J)[6], double r)
{
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

// The lanes' sums and counts of a workgroup of GN_BLOCK lanes become run `run` of the workspace: a butterfly within the wave,
// the four waves in order through LDS.  Every lane of the workgroup calls it (it holds a barrier).
__device__ __forceinline__ void gn_store_run(double (&acc)[GN_SUMS], int count, size_t run, double *part_sums, int *part_count)
{
    __shared__ double red[GN_WAVES][GN_SUMS];
    __shared__ int red_count[GN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < GN_SUMS; ++k)
        acc[k] = wave_sum(acc[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        count += __shfl_xor(count, off, 64);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < GN_SUMS; ++k)
            red[wv][k] = acc[k];
        red_count[wv] = count;
    }
    __syncthreads();
    if (tid < GN_SUMS) {
        double v = red[0][tid];
#pragma unroll
        for (int k = 1; k < GN_WAVES; ++k)
            v += red[k][tid];
        part_sums[run * GN_SUMS + tid] = v;
    } else if (tid == GN_SUMS) {
        int v = red_count[0];
#pragma unroll
        for (int k = 1; k < GN_WAVES; ++k)
            v += red_count[k];
        part_count[run] = v;
    }
}

// entry k of the `width` entries of each of sample s's runs, added in run order (0 for a sample that is not live): the sums
// with width 28, the counts with width 1
template <typename T>
__device__ __forceinline__ T gn_add_runs(bool live, int s, int runs, const T *part, int width, int k)
{
    T v = 0;
    if (live)
        for (int r = 0; r < runs; ++r)
            v += part[((size_t)s * runs + r) * width + k];
    return v;
}

// A x = -b by LDL^T without pivoting on the sums s = (sum r^2, A's upper triangle by rows, b); x = (alpha, beta, gamma, t);
// U = [Rz(gamma) Ry(beta) Rx(alpha) | t] (3 x 4).  -> 0, or 2 for a pivot that is not a finite number > 0, 3 for a
// solution with a component that is not finite.  Every loop is unrolled: the arrays stay in registers.
__device__ __forceinline__ int gn_solve(const double (&s)[GN_SUMS], double (&x)[6], double (&U)[12])
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

// What one lane writes for sample s: the status; on status 0 x and U pose_in, the product formed as cloudaae_pose_compose
// forms its products; on any other status x = 0 and pose_in bit for bit (x and U are not read then).
__device__ __forceinline__ void gn_write_update(int s, int st, const double (&x)[6], const double (&U)[12],
                                                const double *pose_in, double *x_out,
                                                int *status, double *pose_out)
{
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

} // namespace cloudaae
