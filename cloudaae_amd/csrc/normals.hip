// normals.hip -- surface normals of packed point sets by the covariance of a radius neighbourhood (DESIGN.md,
// "Surface normals", has the definition; tests/normals_reference.py restates it in NumPy).
//
// Two launches:
//   nrm_grid_kernel   one workgroup per support set: bounding box, a uniform grid of NRM_GRID^3 cells of edge
//                     h = max(r (1 + 2^-10), extent / (NRM_GRID - 1)), counting sort of the set into cell order.  The
//                     cell counts (16 KiB) are the only thing in LDS; the sorted points live in the workspace, so a set
//                     may have any size.  The scatter's cursors are atomic, so its order inside a cell is free; a
//                     second pass ranks every point of a cell by its index and writes the final array: the order the
//                     sums below are taken in is (cell, index), the same in every run and for every S.
//   nrm_query_kernel  one lane per query, NRM_QBLOCK queries per workgroup, (ceil(K / NRM_QBLOCK), S) workgroups: the
//                     queries of ONE set spread over the machine.  Two passes over the 27 cells around the query (count
//                     and mean, then covariance), cyclic Jacobi on the 3x3 matrix, orientation.  fp64 on the widened
//                     coordinates, every sum in the array's order, no atomics on floating-point values.
#include "common.h"
#include "workspace.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

using namespace cloudaae;

namespace {

constexpr int NRM_THREADS = 1024;
constexpr int NRM_GRID = 16;                               // cells per axis
constexpr int NRM_CELLS = NRM_GRID * NRM_GRID * NRM_GRID;
constexpr int NRM_QBLOCK = 64;
constexpr int NRM_JACOBI_SWEEPS = 16;
constexpr long long NRM_MAX_POINTS = 1ll << 28;            // int offsets

struct NrmGrid {                                           // per set, in the workspace
    double ox, oy, oz, inv_h;
};

// the workspace of s sets of m points in all (null: the size alone is asked for)
struct NrmWorkspace {
    NrmGrid *grids;                                        // [s]
    int *cell_start;                                       // [s, NRM_CELLS + 1]
    float4 *tmp, *sorted;                                  // [m] each
    size_t bytes;
};

NrmWorkspace nrm_workspace(int s, long long m, void *workspace)
{
    Carver ws(workspace);
    NrmWorkspace L;
    L.grids = ws.take<NrmGrid>((size_t)s);
    L.cell_start = ws.take<int>((size_t)s * (NRM_CELLS + 1));
    L.tmp = ws.take<float4>((size_t)m);
    L.sorted = ws.take<float4>((size_t)m);
    L.bytes = ws.bytes();
    return L;
}

// the bounds of set s inside the packed array, whatever the offsets hold
__device__ __forceinline__ void nrm_bounds(const int *off, int s, long long m, int &lo, int &n)
{
    const long long a = min(max((long long)off[s], 0ll), m), b = min(max((long long)off[s + 1], a), m);
    lo = (int)a;
    n = (int)(b - a);
}

__device__ __forceinline__ int nrm_axis(double v, double o, double inv_h)
{
    return (int)fmin(fmax(floor((v - o) * inv_h), 0.0), (double)(NRM_GRID - 1));
}

__device__ __forceinline__ int nrm_cell(const NrmGrid &G, float x, float y, float z)
{
    return (nrm_axis((double)z, G.oz, G.inv_h) * NRM_GRID + nrm_axis((double)y, G.oy, G.inv_h)) * NRM_GRID +
           nrm_axis((double)x, G.ox, G.inv_h);
}

__global__ __launch_bounds__(NRM_THREADS) void nrm_grid_kernel(
    const int *__restrict__ off, long long m, const float *__restrict__ xyz, int ps, float radius,
    NrmGrid *__restrict__ grids, int *__restrict__ cell_start, float4 *__restrict__ tmp, float4 *__restrict__ sorted)
{
    __shared__ int cells[NRM_CELLS];                       // counts, then cursors
    __shared__ int part[NRM_THREADS];
    __shared__ float red[6][NRM_THREADS / 64];
    __shared__ NrmGrid g;
    const int s = blockIdx.x, t = threadIdx.x;
    int lo, n;
    nrm_bounds(off, s, m, lo, n);
    if (n <= 0)
        return;                                            // the query kernel does not look at an empty set's grid
    int *start = cell_start + (long long)s * (NRM_CELLS + 1);
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = t; k < n; k += NRM_THREADS)
        for (int d = 0; d < 3; ++d) {
            const float v = xyz[(long long)(lo + k) * ps + d];
            mn[d] = fminf(mn[d], v);
            mx[d] = fmaxf(mx[d], v);
        }
    for (int d = 0; d < 3; ++d)
        for (int o = 32; o > 0; o >>= 1) {
            mn[d] = fminf(mn[d], __shfl_xor(mn[d], o));
            mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], o));
        }
    if ((t & 63) == 0)
        for (int d = 0; d < 3; ++d) {
            red[d][t >> 6] = mn[d];
            red[3 + d][t >> 6] = mx[d];
        }
    for (int c = t; c < NRM_CELLS; c += NRM_THREADS)
        cells[c] = 0;
    __syncthreads();
    if (t == 0) {
        double lo3[3], ext = 0.0;
        for (int d = 0; d < 3; ++d) {
            float a = red[d][0], b = red[3 + d][0];
            for (int k = 1; k < NRM_THREADS / 64; ++k) {
                a = fminf(a, red[d][k]);
                b = fmaxf(b, red[3 + d][k]);
            }
            lo3[d] = (double)a;
            ext = fmax(ext, (double)b - (double)a);
        }
        const double h = fmax((double)radius * (1.0 + 1.0 / 1024.0), ext / (NRM_GRID - 1));
        g.ox = lo3[0];
        g.oy = lo3[1];
        g.oz = lo3[2];
        g.inv_h = 1.0 / h;
        grids[s] = g;
    }
    __syncthreads();
    const NrmGrid G = g;
    for (int k = t; k < n; k += NRM_THREADS) {
        const float *p = xyz + (long long)(lo + k) * ps;
        atomicAdd(&cells[nrm_cell(G, p[0], p[1], p[2])], 1);
    }
    __syncthreads();
    // exclusive scan of the counts: NRM_CELLS / NRM_THREADS per thread, then across the threads
    constexpr int PER = NRM_CELLS / NRM_THREADS;
    int sum = 0;
    for (int k = 0; k < PER; ++k)
        sum += cells[t * PER + k];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < NRM_THREADS; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int k = 0; k < PER; ++k) {
        const int v = cells[t * PER + k];
        start[t * PER + k] = run;
        cells[t * PER + k] = run;                          // cursor
        run += v;
    }
    if (t == NRM_THREADS - 1)
        start[NRM_CELLS] = run;
    __syncthreads();
    for (int k = t; k < n; k += NRM_THREADS) {
        const float *p = xyz + (long long)(lo + k) * ps;
        const int c = nrm_cell(G, p[0], p[1], p[2]);
        const int q = atomicAdd(&cells[c], 1);             // q in [start[c], start[c + 1]) subset of [0, n)
        tmp[lo + q] = make_float4(p[0], p[1], p[2], __int_as_float(k));
    }
    __syncthreads();                                       // tmp and start of this set: written by this workgroup
    // the cell's points in index order: rank = the cell's points with a smaller index (cursors now = the cells' ends)
    for (int k = t; k < n; k += NRM_THREADS) {
        const float4 p = tmp[lo + k];
        const int c = nrm_cell(G, p.x, p.y, p.z);
        const int a = start[c], b = cells[c], me = __float_as_int(p.w);
        int rank = 0;
        for (int j = a; j < b; ++j)
            rank += __float_as_int(tmp[lo + j].w) < me;
        sorted[lo + a + rank] = p;
    }
}

// f(q) for every point of the 27 cells around cell (cx, cy, cz), in the sorted array's order
template <typename F>
__device__ __forceinline__ void nrm_for_each(const int *start, const float4 *pts, int cx, int cy, int cz, F f)
{
    for (int zz = max(cz - 1, 0); zz <= min(cz + 1, NRM_GRID - 1); ++zz)
        for (int yy = max(cy - 1, 0); yy <= min(cy + 1, NRM_GRID - 1); ++yy) {
            const int row = (zz * NRM_GRID + yy) * NRM_GRID;
            const int a = start[row + max(cx - 1, 0)], b = start[row + min(cx + 1, NRM_GRID - 1) + 1];
            for (int k = a; k < b; ++k)
                f(pts[k]);
        }
}

// Eigen-decomposition of the symmetric 3x3 matrix (a00 a01 a02; . a11 a12; . . a22) by cyclic Jacobi rotations:
// w = the eigenvalues in ascending order, v = the unit eigenvector of w[0] (the first of equal diagonal entries).
__device__ inline void nrm_jacobi3(double a00, double a01, double a02, double a11, double a12, double a22, double *w,
                                   double *v)
{
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < NRM_JACOBI_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (fabs(apq) <= 1e-300 || fabs(apq) <= 1e-18 * (fabs(A[p][p]) + fabs(A[q][q]))) {
                    A[p][q] = A[q][p] = 0.0;
                    continue;
                }
                rotated = true;
                const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                const int r = 3 - p - q;                   // the third index
                const double arp = A[r][p], arq = A[r][q];
                A[r][p] = A[p][r] = c * arp - s * arq;
                A[r][q] = A[q][r] = s * arp + c * arq;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double vip = V[i][p], viq = V[i][q];
                    V[i][p] = c * vip - s * viq;
                    V[i][q] = s * vip + c * viq;
                }
            }
        }
        if (!rotated)
            break;
    }
    double low = A[0][0], x = V[0][0], y = V[1][0], z = V[2][0];
#pragma unroll
    for (int i = 1; i < 3; ++i)
        if (A[i][i] < low) {
            low = A[i][i];
            x = V[0][i];
            y = V[1][i];
            z = V[2][i];
        }
    const double nn = sqrt((x * x + y * y) + z * z);
    v[0] = x / nn;
    v[1] = y / nn;
    v[2] = z / nn;
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
    const double lo01 = fmin(d0, d1), hi01 = fmax(d0, d1);
    w[0] = fmin(lo01, d2);
    w[2] = fmax(hi01, d2);
    w[1] = fmax(lo01, fmin(hi01, d2));
}

__global__ __launch_bounds__(NRM_QBLOCK) void nrm_query_kernel(
    const int *__restrict__ off, long long m, const NrmGrid *__restrict__ grids, const int *__restrict__ cell_start,
    const float4 *__restrict__ sorted, int k, const float *__restrict__ queries, int qps, long long qss, float radius,
    int min_nb, int has_vp, double vx, double vy, double vz, double *__restrict__ normals, double *__restrict__ eig,
    int *__restrict__ count)
{
    const int s = blockIdx.y, i = blockIdx.x * NRM_QBLOCK + threadIdx.x;
    if (i >= k)
        return;
    int lo, n;
    nrm_bounds(off, s, m, lo, n);
    const float *q = queries + (long long)s * qss + (long long)i * qps;
    const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
    const double r = (double)radius, r2 = r * r;
    const long long o = (long long)s * k + i;
    int cnt = 0;
    double nx = 0.0, ny = 0.0, nz = 1.0, w[3] = {0.0, 0.0, 0.0};
    if (n > 0) {
        const NrmGrid G = grids[s];
        const int *start = cell_start + (long long)s * (NRM_CELLS + 1);
        const float4 *pts = sorted + lo;
        const int cx = nrm_axis(x, G.ox, G.inv_h), cy = nrm_axis(y, G.oy, G.inv_h), cz = nrm_axis(z, G.oz, G.inv_h);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        nrm_for_each(start, pts, cx, cy, cz, [&](const float4 p) {
            const double dx = x - (double)p.x, dy = y - (double)p.y, dz = z - (double)p.z;
            if (((dx * dx + dy * dy) + dz * dz) < r2) {
                ++cnt;
                sx += (double)p.x;
                sy += (double)p.y;
                sz += (double)p.z;
            }
        });
        if (cnt >= min_nb) {
            const double c = (double)cnt, mx = sx / c, my = sy / c, mz = sz / c;
            double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
            nrm_for_each(start, pts, cx, cy, cz, [&](const float4 p) {
                const double dx = x - (double)p.x, dy = y - (double)p.y, dz = z - (double)p.z;
                if (((dx * dx + dy * dy) + dz * dz) < r2) {
                    const double ex = (double)p.x - mx, ey = (double)p.y - my, ez = (double)p.z - mz;
                    c00 += ex * ex;
                    c01 += ex * ey;
                    c02 += ex * ez;
                    c11 += ey * ey;
                    c12 += ey * ez;
                    c22 += ez * ez;
                }
            });
            double v[3];
            nrm_jacobi3(c00 / c, c01 / c, c02 / c, c11 / c, c12 / c, c22 / c, w, v);
            nx = v[0];
            ny = v[1];
            nz = v[2];
            if (has_vp && ((nx * (x - vx) + ny * (y - vy)) + nz * (z - vz)) > 0.0) {
                nx = -nx;
                ny = -ny;
                nz = -nz;
            }
        }
    }
    normals[3 * o] = nx;
    normals[3 * o + 1] = ny;
    normals[3 * o + 2] = nz;
    eig[3 * o] = w[0];
    eig[3 * o + 1] = w[1];
    eig[3 * o + 2] = w[2];
    count[o] = cnt;
}

}  // namespace

CLOUDAAE_API long long cloudaae_estimate_normals_workspace_bytes(int s, long long max_points)
{
    if (s < 1 || max_points < 1 || max_points > NRM_MAX_POINTS)
        return -1;
    return (long long)nrm_workspace(s, max_points, nullptr).bytes;
}

CLOUDAAE_API int cloudaae_estimate_normals(int s, const int *offsets, const float *xyz, int xyz_point_stride,
                                           long long max_points, int k, const float *queries, int query_point_stride,
                                           long long query_set_stride, float radius, int min_neighbors,
                                           const double *viewpoint, double *normals, double *eigenvalues, int *count,
                                           void *workspace, long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_estimate_normals";
    CLOUDAAE_REQUIRE(s >= 1 && s <= 65535, name, "s must lie in [1, 65535]");
    CLOUDAAE_REQUIRE(k >= 1, name, "k must be >= 1");
    CLOUDAAE_REQUIRE(max_points >= 1 && max_points <= NRM_MAX_POINTS, name, "max_points must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE((long long)s * k <= (1ll << 30), name, "s * k above the limit of 2^30 queries");
    CLOUDAAE_REQUIRE(radius > 0.0f && isfinite(radius), name, "radius must be a finite number > 0");
    CLOUDAAE_REQUIRE(min_neighbors >= 3, name, "min_neighbors must be >= 3");
    CLOUDAAE_REQUIRE(xyz_point_stride >= 3 && query_point_stride >= 3, name, "point strides must be >= 3 floats");
    CLOUDAAE_REQUIRE(s == 1 || query_set_stride >= (long long)(k - 1) * query_point_stride + 3, name,
                     "query_set_stride must not make the query sets overlap");
    CLOUDAAE_REQUIRE(offsets && xyz && queries && normals && eigenvalues && count && workspace, name, "null pointer");
    CLOUDAAE_REQUIRE(!viewpoint || (isfinite(viewpoint[0]) && isfinite(viewpoint[1]) && isfinite(viewpoint[2])), name,
                     "viewpoint must be finite");
    const NrmWorkspace L = nrm_workspace(s, max_points, workspace);
    CLOUDAAE_REQUIRE(workspace_bytes >= (long long)L.bytes, name,
                     "workspace smaller than cloudaae_estimate_normals_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nrm_grid_kernel, dim3(s), dim3(NRM_THREADS), 0, st, offsets, max_points, xyz, xyz_point_stride,
                       radius, L.grids, L.cell_start, L.tmp, L.sorted);
    hipLaunchKernelGGL(nrm_query_kernel, dim3(ceil_div(k, NRM_QBLOCK), s), dim3(NRM_QBLOCK), 0, st, offsets, max_points,
                       L.grids, L.cell_start, L.sorted, k, queries, query_point_stride, query_set_stride, radius,
                       min_neighbors, viewpoint ? 1 : 0, viewpoint ? viewpoint[0] : 0.0, viewpoint ? viewpoint[1] : 0.0,
                       viewpoint ? viewpoint[2] : 0.0, normals, eigenvalues, count);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
