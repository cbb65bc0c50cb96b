// mesh_cluster.hip -- simplified meshes (gfx950): uniform vertex clustering with quadric-error placement.  All vertices of a
// grid cell become one vertex, placed where the summed squared distances to the planes of the cell's triangles are smallest.
// DESIGN.md, "Simplified meshes", is the definition; tests/simplify_reference.py restates it in NumPy.  Integers where the
// definition has integers, fp64 otherwise on exactly widened float32 values, un-fused (the file is compiled with
// -ffp-contract=off), in the order written here.
//
//   cloudaae_mesh_cluster_keys       one launch, a lane per vertex: the vertex's cell key, or -1.
//   cloudaae_mesh_cluster_sums       one launch, a wave per cell: the lanes stride over the cell's vertex list and then over its
//                                    corner list, each lane adds its terms into 13 registers in list order, a fixed butterfly
//                                    (wave_sum) joins the lanes and lane 0 stores the cell's 16 doubles and two counts.
//   cloudaae_mesh_cluster_place      one launch, a lane per cell: cyclic Jacobi on the cell's 3 x 3 matrix in registers, the
//                                    truncated solve, the cell test, the error.
//   cloudaae_mesh_cluster_triangles  one launch, a lane per triangle: the rotated triple of cell ranks as one key, or -1.
//
// No atomic of any kind and no workgroup waits for another: every cell belongs to one wave (or lane), and the order of its
// additions follows from the lists alone -- the same bits run to run and whatever else is in the mesh.
#include "common.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

namespace cloudaae {

constexpr long long MC_MAX_ITEMS = ((1ll << 31) - 1) / 3;   // V, T < 2^31 / 3: 3 V and 3 T index int32 arrays
constexpr int MC_MAX_DIM = 1 << 20;
constexpr int MC_MAX_CELLS = 1 << 21;
constexpr int MC_RANK_BITS = 21;
constexpr int MC_BLOCK = 256;
constexpr int MC_WAVES = MC_BLOCK / 64;
constexpr int MC_SWEEPS = 8;

struct McGrid {
    double ox, oy, oz, c;
};

// the centre of cell index g along an axis with origin o
__device__ __forceinline__ double mc_centre(double o, int g, double c) { return o + ((double)g + 0.5) * c; }

// ---- keys -------------------------------------------------------------------------------------------------------------------
// floor((p - o) / c) of one axis, tested against [0, n) in float64 before the conversion; a NaN fails
__device__ __forceinline__ bool mc_axis(float p, double o, double c, int n, long long &g)
{
    const double fl = floor(((double)p - o) / c);
    const bool ok = fl >= 0.0 && fl < (double)n;
    g = ok ? (long long)fl : 0;
    return ok;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_keys_kernel(int V, const float *__restrict__ vertices, McGrid g, int nx, int ny,
                                                         int nz, long long *__restrict__ key)
{
    const long long v = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V)
        return;
    long long gx, gy, gz;
    bool ok = mc_axis(vertices[3 * v + 0], g.ox, g.c, nx, gx);
    ok = mc_axis(vertices[3 * v + 1], g.oy, g.c, ny, gy) && ok;
    ok = mc_axis(vertices[3 * v + 2], g.oz, g.c, nz, gz) && ok;
    key[v] = ok ? (gz * ny + gy) * nx + gx : -1ll;
}

// ---- sums -------------------------------------------------------------------------------------------------------------------
struct McSumsArgs {
    int V, T, C;
    const float *vertices;
    const int *triangles;
    const int *rank;
    const int *cell_grid;
    McGrid g;
    const int *vert_order;
    long long n_vert_order;
    const long long *vert_start;
    const int *corner_order;
    long long n_corner_order;
    const long long *corner_start;
    double *sums;
    int *counts;
};

// the part [lo, hi) of a list of n entries that a cell's two starts name: starts that are not a prefix sum read nothing outside
__device__ __forceinline__ void mc_range(const long long *start, int cell, long long n, long long &lo, long long &hi)
{
    lo = start[cell], hi = start[cell + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_sums_kernel(McSumsArgs a)
{
    const int cell = (int)blockIdx.x * MC_WAVES + (int)(threadIdx.x >> 6);      // the same in every lane of the wave
    if (cell >= a.C)
        return;
    const int lane = lane_id();
    const double zx = mc_centre(a.g.ox, a.cell_grid[3 * cell + 0], a.g.c), zy = mc_centre(a.g.oy, a.cell_grid[3 * cell + 1], a.g.c),
                 zz = mc_centre(a.g.oz, a.cell_grid[3 * cell + 2], a.g.c);
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, e = 0.0;
    int n_v = 0, n_c = 0;

    long long lo, hi;
    mc_range(a.vert_start, cell, a.n_vert_order, lo, hi);
#pragma unroll 1
    for (long long at = lo + lane; at < hi; at += 64) {
        const int v = a.vert_order[at];
        if (v < 0 || v >= a.V || a.rank[v] != cell)                             // out of range, or not this cell's: skipped
            continue;
        m0 += (double)a.vertices[3 * (size_t)v + 0] - zx;
        m1 += (double)a.vertices[3 * (size_t)v + 1] - zy;
        m2 += (double)a.vertices[3 * (size_t)v + 2] - zz;
        n_v += 1;
    }

    mc_range(a.corner_start, cell, a.n_corner_order, lo, hi);
    const long long corners = 3ll * a.T;
#pragma unroll 1
    for (long long at = lo + lane; at < hi; at += 64) {
        const int corner = a.corner_order[at];
        if (corner < 0 || corner >= corners)
            continue;
        const int t = corner / 3, k = corner - 3 * t;
        const int i0 = a.triangles[3 * (size_t)t + 0], i1 = a.triangles[3 * (size_t)t + 1], i2 = a.triangles[3 * (size_t)t + 2];
        if (i0 < 0 || i0 >= a.V || i1 < 0 || i1 >= a.V || i2 < 0 || i2 >= a.V)  // a dropped triangle
            continue;
        const int r0 = a.rank[i0], r1 = a.rank[i1], r2 = a.rank[i2];
        if (r0 < 0 || r1 < 0 || r2 < 0 || (k == 0 ? r0 : k == 1 ? r1 : r2) != cell)
            continue;
        const float *p0 = a.vertices + 3 * (size_t)i0, *p1 = a.vertices + 3 * (size_t)i1, *p2 = a.vertices + 3 * (size_t)i2;
        const double q00 = (double)p0[0] - zx, q01 = (double)p0[1] - zy, q02 = (double)p0[2] - zz;
        const double u0 = ((double)p1[0] - zx) - q00, u1 = ((double)p1[1] - zy) - q01, u2 = ((double)p1[2] - zz) - q02;
        const double w0 = ((double)p2[0] - zx) - q00, w1 = ((double)p2[1] - zy) - q01, w2 = ((double)p2[2] - zz) - q02;
        const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
        const double d = -((n0 * q00 + n1 * q01) + n2 * q02);
        a00 += n0 * n0, a01 += n0 * n1, a02 += n0 * n2, a11 += n1 * n1, a12 += n1 * n2, a22 += n2 * n2;
        b0 += n0 * d, b1 += n1 * d, b2 += n2 * d;
        e += d * d;
        n_c += 1;
    }

    m0 = wave_sum(m0), m1 = wave_sum(m1), m2 = wave_sum(m2);
    a00 = wave_sum(a00), a01 = wave_sum(a01), a02 = wave_sum(a02), a11 = wave_sum(a11), a12 = wave_sum(a12), a22 = wave_sum(a22);
    b0 = wave_sum(b0), b1 = wave_sum(b1), b2 = wave_sum(b2), e = wave_sum(e);
    int tv = n_v, tc = n_c;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        tv += __shfl_xor(tv, off, 64);
        tc += __shfl_xor(tc, off, 64);
    }
    if (lane == 0) {
        double *out = a.sums + 16 * (size_t)cell;
        out[0] = m0, out[1] = m1, out[2] = m2;
        out[3] = a00, out[4] = a01, out[5] = a02, out[6] = a11, out[7] = a12, out[8] = a22;
        out[9] = b0, out[10] = b1, out[11] = b2, out[12] = e;
        out[13] = 0.0, out[14] = 0.0, out[15] = 0.0;
        a.counts[2 * (size_t)cell + 0] = tv;
        a.counts[2 * (size_t)cell + 1] = tc;
    }
}

// ---- placement --------------------------------------------------------------------------------------------------------------
// one rotation of cyclic Jacobi on the pair (p, q), r the third index: nothing when a_pq == 0; theta = (a_qq - a_pp) / (2 a_pq),
// t = sign(theta) / (|theta| + sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c.  v0, v1, v2 are the rows of V.
__device__ __forceinline__ void mc_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q,
                                          double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0)
        return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq, arq = s * rp + c * rq;
    double x = v0p, y = v0q;
    v0p = c * x - s * y, v0q = s * x + c * y;
    x = v1p, y = v1q;
    v1p = c * x - s * y, v1q = s * x + c * y;
    x = v2p, y = v2q;
    v2p = c * x - s * y, v2q = s * x + c * y;
}

__device__ __forceinline__ double mc_dot(double a0, double a1, double a2, double x0, double x1, double x2)
{
    return (a0 * x0 + a1 * x1) + a2 * x2;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_place_kernel(int C, const double *__restrict__ sums, const int *__restrict__ counts,
                                                          const int *__restrict__ cell_grid, McGrid g, double eps,
                                                          double *__restrict__ pos, unsigned char *__restrict__ how,
                                                          double *__restrict__ err)
{
    const int cell = (int)blockIdx.x * MC_BLOCK + (int)threadIdx.x;
    if (cell >= C)
        return;
    const double *s = sums + 16 * (size_t)cell;
    const double n_v = (double)counts[2 * (size_t)cell];
    const double mx = s[0] / n_v, my = s[1] / n_v, mz = s[2] / n_v;
    const double A00 = s[3], A01 = s[4], A02 = s[5], A11 = s[6], A12 = s[7], A22 = s[8], B0 = s[9], B1 = s[10], B2 = s[11], E = s[12];

    double a00 = A00, a01 = A01, a02 = A02, a11 = A11, a12 = A12, a22 = A22;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
#pragma unroll 1
    for (int sweep = 0; sweep < MC_SWEEPS; ++sweep) {
        mc_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);       // (0, 1), r = 2
        mc_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);       // (0, 2), r = 1
        mc_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);       // (1, 2), r = 0
    }
    double lmax = a11 > a00 ? a11 : a00;
    lmax = a22 > lmax ? a22 : lmax;
    const bool usable = isfinite(a00) && isfinite(a11) && isfinite(a22) && lmax > 0.0;

    const double r0 = -B0 - mc_dot(A00, A01, A02, mx, my, mz), r1 = -B1 - mc_dot(A01, A11, A12, mx, my, mz),
                 r2 = -B2 - mc_dot(A02, A12, A22, mx, my, mz);
    double x0 = mx, x1 = my, x2 = mz;
    int kept = 0;
    if (usable) {
        const double cut = eps * lmax;
        if (a00 > cut) {
            const double coef = mc_dot(v00, v10, v20, r0, r1, r2) / a00;
            x0 = x0 + v00 * coef, x1 = x1 + v10 * coef, x2 = x2 + v20 * coef;
            kept += 1;
        }
        if (a11 > cut) {
            const double coef = mc_dot(v01, v11, v21, r0, r1, r2) / a11;
            x0 = x0 + v01 * coef, x1 = x1 + v11 * coef, x2 = x2 + v21 * coef;
            kept += 1;
        }
        if (a22 > cut) {
            const double coef = mc_dot(v02, v12, v22, r0, r1, r2) / a22;
            x0 = x0 + v02 * coef, x1 = x1 + v12 * coef, x2 = x2 + v22 * coef;
            kept += 1;
        }
        const double half = g.c / 2.0;
        if (!(fabs(x0) <= half && fabs(x1) <= half && fabs(x2) <= half)) {      // outside the closed cell, or not a number
            x0 = mx, x1 = my, x2 = mz;
            kept += 4;
        }
    } else {
        kept = 4;
    }
    pos[3 * (size_t)cell + 0] = mc_centre(g.ox, cell_grid[3 * cell + 0], g.c) + x0;
    pos[3 * (size_t)cell + 1] = mc_centre(g.oy, cell_grid[3 * cell + 1], g.c) + x1;
    pos[3 * (size_t)cell + 2] = mc_centre(g.oz, cell_grid[3 * cell + 2], g.c) + x2;
    how[cell] = (unsigned char)kept;
    const double ax0 = mc_dot(A00, A01, A02, x0, x1, x2), ax1 = mc_dot(A01, A11, A12, x0, x1, x2), ax2 = mc_dot(A02, A12, A22, x0, x1, x2);
    err[cell] = (mc_dot(ax0, ax1, ax2, x0, x1, x2) + 2.0 * mc_dot(B0, B1, B2, x0, x1, x2)) + E;
}

// ---- triangles --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_triangles_kernel(int V, int T, const int *__restrict__ triangles,
                                                              const int *__restrict__ rank, int C, long long *__restrict__ tri_key)
{
    const long long t = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (t >= T)
        return;
    const int i0 = triangles[3 * t + 0], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
    long long key = -1;
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const long long r0 = rank[i0], r1 = rank[i1], r2 = rank[i2];
        if (r0 >= 0 && r0 < C && r1 >= 0 && r1 < C && r2 >= 0 && r2 < C && r0 != r1 && r1 != r2 && r2 != r0) {
            // rotated so that the smallest rank comes first: the orientation stays
            const bool first0 = r0 < r1 && r0 < r2, first1 = !first0 && r1 < r2;
            const long long ra = first0 ? r0 : first1 ? r1 : r2, rb = first0 ? r1 : first1 ? r2 : r0, rc = first0 ? r2 : first1 ? r0 : r1;
            key = (((ra << MC_RANK_BITS) + rb) << MC_RANK_BITS) + rc;
        }
    }
    tri_key[t] = key;
}

static bool mc_grid_ok(double ox, double oy, double oz, double cell)
{
    return isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(cell) && cell > 0.0;
}

static const char *const MC_GRID_LIMITS = "the origin must be finite and the cell finite and positive";
static const char *const MC_ITEM_LIMITS = "outside the limits: 0 <= V, T < 2^31 / 3";
static const char *const MC_CELL_LIMITS = "outside the limits: 0 <= C <= 2^21";

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_mesh_cluster_keys(int V, const float *vertices, double ox, double oy, double oz, double cell, int nx,
                                            int ny, int nz, long long *key, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_mesh_cluster_keys";
    CLOUDAAE_REQUIRE(V >= 0 && V <= MC_MAX_ITEMS, name, MC_ITEM_LIMITS);
    CLOUDAAE_REQUIRE(mc_grid_ok(ox, oy, oz, cell), name, MC_GRID_LIMITS);
    CLOUDAAE_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= MC_MAX_DIM && ny <= MC_MAX_DIM && nz <= MC_MAX_DIM, name,
                     "outside the limits: 1 <= nx, ny, nz <= 2^20");
    CLOUDAAE_REQUIRE(V == 0 || (vertices && key), name, "null pointer");
    if (V == 0)
        return 0;
    hipLaunchKernelGGL(mc_keys_kernel, dim3((unsigned)ceil_div(V, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, V, vertices,
                       McGrid{ox, oy, oz, cell}, nx, ny, nz, key);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_mesh_cluster_sums(int V, int T, const float *vertices, const int *triangles, int C, const int *rank,
                                            const int *cell_grid, double ox, double oy, double oz, double cell,
                                            const int *vert_order, long long n_vert_order, const long long *vert_start,
                                            const int *corner_order, long long n_corner_order, const long long *corner_start,
                                            double *sums, int *counts, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_mesh_cluster_sums";
    CLOUDAAE_REQUIRE(V >= 0 && V <= MC_MAX_ITEMS && T >= 0 && T <= MC_MAX_ITEMS, name, MC_ITEM_LIMITS);
    CLOUDAAE_REQUIRE(C >= 0 && C <= MC_MAX_CELLS, name, MC_CELL_LIMITS);
    CLOUDAAE_REQUIRE(mc_grid_ok(ox, oy, oz, cell), name, MC_GRID_LIMITS);
    CLOUDAAE_REQUIRE(n_vert_order >= 0 && n_vert_order <= V && n_corner_order >= 0 && n_corner_order <= 3ll * T, name,
                     "the orders hold at most V vertices and 3 T corners");
    CLOUDAAE_REQUIRE(C == 0 || (cell_grid && vert_start && corner_start && sums && counts), name, "null pointer");
    CLOUDAAE_REQUIRE((V == 0 || (vertices && rank)) && (T == 0 || triangles) && (n_vert_order == 0 || vert_order) &&
                         (n_corner_order == 0 || corner_order),
                     name, "null pointer");
    if (C == 0)
        return 0;
    McSumsArgs a;
    a.V = V, a.T = T, a.C = C;
    a.vertices = vertices, a.triangles = triangles, a.rank = rank, a.cell_grid = cell_grid;
    a.g = McGrid{ox, oy, oz, cell};
    a.vert_order = vert_order, a.n_vert_order = n_vert_order, a.vert_start = vert_start;
    a.corner_order = corner_order, a.n_corner_order = n_corner_order, a.corner_start = corner_start;
    a.sums = sums, a.counts = counts;
    hipLaunchKernelGGL(mc_sums_kernel, dim3((unsigned)ceil_div(C, MC_WAVES)), dim3(MC_BLOCK), 0, (hipStream_t)stream, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_mesh_cluster_place(int C, const double *sums, const int *counts, const int *cell_grid, double ox,
                                             double oy, double oz, double cell, double eps, double *pos, uint8_t *how,
                                             double *err, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_mesh_cluster_place";
    CLOUDAAE_REQUIRE(C >= 0 && C <= MC_MAX_CELLS, name, MC_CELL_LIMITS);
    CLOUDAAE_REQUIRE(mc_grid_ok(ox, oy, oz, cell), name, MC_GRID_LIMITS);
    CLOUDAAE_REQUIRE(isfinite(eps) && eps > 0.0, name, "eps must be finite and > 0");
    CLOUDAAE_REQUIRE(C == 0 || (sums && counts && cell_grid && pos && how && err), name, "null pointer");
    if (C == 0)
        return 0;
    hipLaunchKernelGGL(mc_place_kernel, dim3((unsigned)ceil_div(C, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, C, sums, counts,
                       cell_grid, McGrid{ox, oy, oz, cell}, eps, pos, how, err);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_mesh_cluster_triangles(int V, int T, const int *triangles, const int *rank, int C, long long *tri_key,
                                                 cloudaae_stream_t stream)
{
    const char *name = "cloudaae_mesh_cluster_triangles";
    CLOUDAAE_REQUIRE(V >= 0 && V <= MC_MAX_ITEMS && T >= 0 && T <= MC_MAX_ITEMS, name, MC_ITEM_LIMITS);
    CLOUDAAE_REQUIRE(C >= 0 && C <= MC_MAX_CELLS, name, MC_CELL_LIMITS);
    CLOUDAAE_REQUIRE(T == 0 || (triangles && tri_key && (V == 0 || rank)), name, "null pointer");
    if (T == 0)
        return 0;
    hipLaunchKernelGGL(mc_triangles_kernel, dim3((unsigned)ceil_div(T, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, V, T,
                       triangles, rank, C, tri_key);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
