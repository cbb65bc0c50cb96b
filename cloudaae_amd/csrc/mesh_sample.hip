// mesh_sample.hip -- object models from triangle meshes on the GPU (gfx950): area weights as integers, their exact
// prefix sums, area-uniform surface samples with colours and face normals, and the row gather behind the model.
//
// DESIGN.md, "Mesh sampling", is the definition; tests/mesh_models_reference.py restates it in NumPy with Python
// integers.  Every index-valued result is integer arithmetic: a triangle's weight is floor(A2 / A2max * 2^32), the
// cumulative weights are a uint64 scan, and a draw is the high half of a 64 x 64 bit product searched in that scan --
// none depends on the order of a sum.  The floating-point part is fp64 on the widened fp32 coordinates, un-fused (the
// file is compiled with -ffp-contract=off) in the order written here.  A draw is a pure function of
// (seed, mesh id, global sample index) through philox4x32, stream 20.
//
//   cloudaae_mesh_weights      a memset and four launches: areas and the per-mesh maximum (integer atomic max on the
//                              bit pattern), weights and a block scan, the scan of the block sums (one workgroup, a
//                              carry across its rounds), the blocks' prefixes added and the mesh's base subtracted
//   cloudaae_mesh_sample       one launch, one lane per sample
//   cloudaae_mesh_gather_rows  one launch, one lane per output element
#include "common.h"
#include "philox.h"
#include "workspace.h"
#include "../../include/cloudaae_hip.h"
#include <math.h>

namespace cloudaae {

constexpr unsigned MS_STREAM = 20u;        // r0, r1 the triangle; r2 u; r3 v (synth.hip: 1-4 and 7; pose_sample.hip: 16-19)
constexpr int MS_SCAN_BLOCK = 256;         // B: triangles per block of the scan (tests/test_23_mesh_models_gpu.py names it)
constexpr long long MS_MAX_TOTAL = 1ll << 28;      // vertices, triangles and samples of one call
constexpr int MS_MAX_MESHES = 65535;
typedef unsigned long long u64;

// the mesh that holds packed triangle t: the last s with offsets[s] <= t (empty meshes are stepped over); s_count when
// t lies past the last mesh
__device__ __forceinline__ int ms_mesh_of(const int *__restrict__ offsets, int s_count, int t)
{
    int lo = 0, hi = s_count + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= t)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

// the three corners of packed triangle t of a mesh whose vertices are v0 .. v1 of `vertices`, widened; false when an
// index lies outside the mesh
__device__ __forceinline__ bool ms_corners(const int *__restrict__ triangles, int t, int v0, int v1, int ids[3])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = triangles[3 * (size_t)t + k];
        ok = ok && i >= 0 && i < v1 - v0;
        ids[k] = v0 + i;
    }
    return ok;
}

// n = e1 x e2, each component (p q) - (r s), and A2 = sqrt((nx^2 + ny^2) + nz^2), in double
__device__ __forceinline__ double ms_normal(const float *__restrict__ vertices, const int ids[3], double n[3])
{
    double a[3], e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)vertices[3 * (size_t)ids[0] + k];
        e1[k] = (double)vertices[3 * (size_t)ids[1] + k] - a[k];
        e2[k] = (double)vertices[3 * (size_t)ids[2] + k] - a[k];
    }
    n[0] = (e1[1] * e2[2]) - (e1[2] * e2[1]);
    n[1] = (e1[2] * e2[0]) - (e1[0] * e2[2]);
    n[2] = (e1[0] * e2[1]) - (e1[1] * e2[0]);
    return sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
}

// a mesh's ranges, taken as empty when the offsets do not describe ranges inside the packed arrays
__device__ __forceinline__ bool ms_ranges(const int *__restrict__ vert_offsets, const int *__restrict__ tri_offsets, int s, int nv,
                                  int nt, int &v0, int &v1, int &t0, int &t1)
{
    v0 = vert_offsets[s];
    v1 = vert_offsets[s + 1];
    t0 = tri_offsets[s];
    t1 = tri_offsets[s + 1];
    return v0 >= 0 && v0 <= v1 && v1 <= nv && t0 >= 0 && t0 <= t1 && t1 <= nt;
}

// pass 1, one lane per triangle: A2 -> a2 (0 for a triangle that gets no weight), the mesh's maximum, its invalid count
__global__ __launch_bounds__(MS_SCAN_BLOCK) void mesh_area_kernel(int s_count, const int *__restrict__ vert_offsets,
                                                          const int *__restrict__ tri_offsets, int nv, int nt,
                                                          const float *__restrict__ vertices,
                                                          const int *__restrict__ triangles, double *__restrict__ a2,
                                                          u64 *a2max, int *invalid)
{
    const int t = blockIdx.x * MS_SCAN_BLOCK + threadIdx.x;
    double area = 0.0;
    int s = -1;
    if (t < nt) {
        s = ms_mesh_of(tri_offsets, s_count, t);
        int v0, v1, t0, t1;
        if (s >= 0 && s < s_count && ms_ranges(vert_offsets, tri_offsets, s, nv, nt, v0, v1, t0, t1)) {
            int ids[3];
            double n[3];
            bool ok = ms_corners(triangles, t, v0, v1, ids);
            if (ok) {
                area = ms_normal(vertices, ids, n);
                ok = isfinite(area) && area > 0.0;
            }
            if (!ok) {
                area = 0.0;
                atomicAdd(invalid + s, 1);
            }
        } else {
            s = -1;
        }
        a2[t] = area;
    }
    // integer maximum on the bit pattern of a non-negative double: exact in any order.  A wave whose lanes all lie in
    // one mesh (lanes past the end aside: they bring 0) sends one atomic, the others one per lane; the plain read
    // before it only spares atomics: what it sees is never above the true maximum.
    u64 bits = (u64)__double_as_longlong(area);
    const unsigned long long in_mesh = __ballot(s >= 0);
    const int lead = __shfl(s, in_mesh ? __ffsll((long long)in_mesh) - 1 : 0, 64);      // (no such lane: -1, and bits are 0)
    if (__all(s < 0 || s == lead)) {
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = __shfl_xor(bits, off, 64);
            bits = o > bits ? o : bits;
        }
        if (lane_id() != 0)
            bits = 0;
        s = lead;
    }
    if (bits > 0 && bits > __atomic_load_n(a2max + s, __ATOMIC_RELAXED))
        atomicMax(a2max + s, bits);
}

// inclusive scan of one value per lane over the workgroup
__device__ __forceinline__ u64 ms_block_scan(u64 v, u64 (&buf)[2][MS_SCAN_BLOCK])
{
    const int i = threadIdx.x;
    int cur = 0;
    buf[0][i] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < MS_SCAN_BLOCK; off <<= 1) {
        buf[cur ^ 1][i] = buf[cur][i] + (i >= off ? buf[cur][i - off] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    const u64 r = buf[cur][i];
    __syncthreads();
    return r;
}

// pass 2: w = floor(A2 / A2max * 2^32), its scan inside the block of B packed triangles, the block's sum
__global__ __launch_bounds__(MS_SCAN_BLOCK) void mesh_weight_kernel(int s_count, const int *__restrict__ tri_offsets, int nt,
                                                            const double *__restrict__ a2,
                                                            const u64 *__restrict__ a2max, u64 *__restrict__ weights,
                                                            u64 *__restrict__ local, u64 *__restrict__ block_sum)
{
    __shared__ u64 buf[2][MS_SCAN_BLOCK];
    const int t = blockIdx.x * MS_SCAN_BLOCK + threadIdx.x;
    u64 w = 0;
    if (t < nt) {
        const double area = a2[t];
        if (area > 0.0) {                  // then t lies in a mesh and that mesh's maximum is >= area
            const int s = ms_mesh_of(tri_offsets, s_count, t);
            const double top = __longlong_as_double((long long)a2max[s]);
            w = (u64)((area / top) * 4294967296.0);
        }
        weights[t] = w;
    }
    const u64 incl = ms_block_scan(w, buf);
    if (t < nt)
        local[t] = incl;
    if (threadIdx.x == MS_SCAN_BLOCK - 1)
        block_sum[blockIdx.x] = incl;
}

// pass 3, one workgroup: block_prefix = the exclusive scan of the block sums, B at a time with a carry
__global__ __launch_bounds__(MS_SCAN_BLOCK) void mesh_block_prefix_kernel(int blocks, const u64 *__restrict__ block_sum,
                                                                  u64 *__restrict__ block_prefix)
{
    __shared__ u64 buf[2][MS_SCAN_BLOCK];
    __shared__ u64 carry_s;
    u64 carry = 0;
    for (int base = 0; base < blocks; base += MS_SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        const u64 v = i < blocks ? block_sum[i] : 0ull;
        const u64 incl = ms_block_scan(v, buf);
        if (i < blocks)
            block_prefix[i] = carry + (incl - v);
        if (threadIdx.x == MS_SCAN_BLOCK - 1)
            carry_s = carry + incl;
        __syncthreads();
        carry = carry_s;
        __syncthreads();
    }
}

// pass 4: cum[t] = (the packed scan at t) - (the packed scan before the mesh's first triangle)
__global__ __launch_bounds__(MS_SCAN_BLOCK) void mesh_cum_kernel(int s_count, const int *__restrict__ tri_offsets, int nt,
                                                         const u64 *__restrict__ local,
                                                         const u64 *__restrict__ block_prefix, u64 *__restrict__ cum)
{
    const int t = blockIdx.x * MS_SCAN_BLOCK + threadIdx.x;
    if (t >= nt)
        return;
    const int s = ms_mesh_of(tri_offsets, s_count, t);
    u64 base = 0;
    if (s >= 0 && s < s_count) {
        const int t0 = tri_offsets[s];
        if (t0 > 0 && t0 <= t)
            base = block_prefix[(t0 - 1) / MS_SCAN_BLOCK] + local[t0 - 1];
    }
    cum[t] = (block_prefix[t / MS_SCAN_BLOCK] + local[t]) - base;
}

// one lane per sample: sample j of mesh s
__global__ __launch_bounds__(64) void mesh_sample_kernel(int s_count, const int *__restrict__ vert_offsets,
                                                 const int *__restrict__ tri_offsets, int nv, int nt,
                                                 const float *__restrict__ vertices, const float *__restrict__ colors,
                                                 const int *__restrict__ triangles, const u64 *__restrict__ cum,
                                                 const int *__restrict__ mesh_ids, int n, u64 first, u64 seed,
                                                 float *__restrict__ xyzrgb, int *__restrict__ tri,
                                                 double *__restrict__ normal)
{
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long long)s_count * n)
        return;
    const int s = (int)(i / n), j = (int)(i - (long long)s * n);
    float out[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    double nrm[3] = {0.0, 0.0, 0.0};
    int picked = -1;
    int v0, v1, t0, t1;
    if (ms_ranges(vert_offsets, tri_offsets, s, nv, nt, v0, v1, t0, t1) && t1 > t0) {
        const u64 total = cum[t1 - 1];
        if (total > 0) {
            const u64 id = (u64)(mesh_ids ? mesh_ids[s] : s);
            unsigned r[4];
            philox4x32(seed, (id << 40) + (first + (u64)j), MS_STREAM, r);
            const u64 target = __umul64hi(((u64)r[0] << 32) | (u64)r[1], total);      // < total
            // the first t with cum[t] > target
            int lo = t0, hi = t1 - 1;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (cum[mid] > target)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            int ids[3];
            if (ms_corners(triangles, lo, v0, v1, ids)) {        // (always, with the weights of cloudaae_mesh_weights)
                picked = lo - t0;
                double u = (double)u01(r[2]), v = (double)u01(r[3]);
                if (u + v > 1.0) {
                    u = 1.0 - u;
                    v = 1.0 - v;
                }
                const double b0 = (1.0 - u) - v;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double a = (double)vertices[3 * (size_t)ids[0] + k], b = (double)vertices[3 * (size_t)ids[1] + k],
                                 c = (double)vertices[3 * (size_t)ids[2] + k];
                    out[k] = (float)((b0 * a + u * b) + v * c);
                    if (colors) {
                        const double ca = (double)colors[3 * (size_t)ids[0] + k], cb = (double)colors[3 * (size_t)ids[1] + k],
                                     cc = (double)colors[3 * (size_t)ids[2] + k];
                        out[3 + k] = (float)((b0 * ca + u * cb) + v * cc);
                    }
                }
                if (normal) {
                    double nn[3];
                    const double area = ms_normal(vertices, ids, nn);
                    if (isfinite(area) && area > 0.0) {
                        nrm[0] = nn[0] / area;
                        nrm[1] = nn[1] / area;
                        nrm[2] = nn[2] / area;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        xyzrgb[6 * (size_t)i + k] = out[k];
    tri[i] = picked;
    if (normal) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            normal[3 * (size_t)i + k] = nrm[k];
    }
}

// dst[set, j, c] = src[set, idx[set, j], c]; an index outside the set's rows gives zeros
template <typename T>
__global__ __launch_bounds__(256) void mesh_gather_rows_kernel(long long total, int k, int cols, const int *__restrict__ idx,
                                                       long long rows_per_set, const T *__restrict__ src,
                                                       long long src_row_stride, T *__restrict__ dst,
                                                       long long dst_row_stride)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total)
        return;
    const long long row = e / cols;
    const int c = (int)(e - row * cols);
    const long long set = row / k;
    const long long pick = idx ? (long long)idx[row] : row - set * k;
    T v = (T)0;
    if (pick >= 0 && pick < rows_per_set)
        v = src[(set * rows_per_set + pick) * src_row_stride + c];
    dst[row * dst_row_stride + c] = v;
}

// the workspace of cloudaae_mesh_weights (null: the size alone is asked for)
struct MsWorkspace {
    double *a2;                                    // [num_triangles]
    u64 *local, *block_sum, *block_prefix;         // [num_triangles], [blocks], [blocks]
    size_t bytes;
};

static MsWorkspace ms_workspace(long long num_triangles, void *workspace)
{
    const size_t blocks = (size_t)ceil_div(num_triangles, MS_SCAN_BLOCK);
    Carver ws(workspace);
    MsWorkspace L;
    L.a2 = ws.take<double>((size_t)num_triangles);
    L.local = ws.take<u64>((size_t)num_triangles);
    L.block_sum = ws.take<u64>(blocks);
    L.block_prefix = ws.take<u64>(blocks);
    L.bytes = ws.bytes();
    return L;
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API long long cloudaae_mesh_weights_workspace_bytes(long long num_triangles)
{
    if (num_triangles < 1 || num_triangles > MS_MAX_TOTAL)
        return -1;
    return (long long)ms_workspace(num_triangles, nullptr).bytes;
}

CLOUDAAE_API int cloudaae_mesh_weights(int s, const int *vert_offsets, const int *tri_offsets, long long num_vertices,
                                       long long num_triangles, const float *vertices, const int *triangles,
                                       unsigned long long *weights, unsigned long long *cum, double *a2max, int *invalid,
                                       void *workspace, long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_mesh_weights";
    CLOUDAAE_REQUIRE(s >= 1 && s <= MS_MAX_MESHES, name, "s must lie in [1, 65535]");
    CLOUDAAE_REQUIRE(num_vertices >= 1 && num_vertices <= MS_MAX_TOTAL, name, "num_vertices must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(num_triangles >= 1 && num_triangles <= MS_MAX_TOTAL, name, "num_triangles must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(vert_offsets && tri_offsets && vertices && triangles && weights && cum && a2max && invalid && workspace,
                     name, "null pointer");
    const MsWorkspace L = ms_workspace(num_triangles, workspace);
    CLOUDAAE_REQUIRE(workspace_bytes >= (long long)L.bytes, name, "workspace smaller than cloudaae_mesh_weights_workspace_bytes");
    const int nt = (int)num_triangles, blocks = ceil_div(num_triangles, MS_SCAN_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(a2max, 0, sizeof(double) * (size_t)s, st), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(invalid, 0, sizeof(int) * (size_t)s, st), name);
    hipLaunchKernelGGL(mesh_area_kernel, dim3(blocks), dim3(MS_SCAN_BLOCK), 0, st, s, vert_offsets, tri_offsets,
                       (int)num_vertices, nt, vertices, triangles, L.a2, (u64 *)a2max, invalid);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mesh_weight_kernel, dim3(blocks), dim3(MS_SCAN_BLOCK), 0, st, s, tri_offsets, nt, L.a2, (const u64 *)a2max,
                       (u64 *)weights, L.local, L.block_sum);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mesh_block_prefix_kernel, dim3(1), dim3(MS_SCAN_BLOCK), 0, st, blocks, L.block_sum, L.block_prefix);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mesh_cum_kernel, dim3(blocks), dim3(MS_SCAN_BLOCK), 0, st, s, tri_offsets, nt, L.local, L.block_prefix,
                       (u64 *)cum);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_mesh_sample(int s, const int *vert_offsets, const int *tri_offsets, long long num_vertices,
                                      long long num_triangles, const float *vertices, const float *colors,
                                      const int *triangles, const unsigned long long *cum, const int *mesh_ids, int n,
                                      unsigned long long first_index, unsigned long long seed, float *xyzrgb, int *tri,
                                      double *normal, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_mesh_sample";
    CLOUDAAE_REQUIRE(s >= 1 && s <= MS_MAX_MESHES, name, "s must lie in [1, 65535]");
    CLOUDAAE_REQUIRE(n >= 1 && (long long)s * n <= MS_MAX_TOTAL, name, "n must be >= 1 and s * n <= 2^28");
    CLOUDAAE_REQUIRE(num_vertices >= 1 && num_vertices <= MS_MAX_TOTAL, name, "num_vertices must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(num_triangles >= 1 && num_triangles <= MS_MAX_TOTAL, name, "num_triangles must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(first_index <= (1ull << 40) - (unsigned long long)n, name, "first_index + n above 2^40");
    CLOUDAAE_REQUIRE(vert_offsets && tri_offsets && vertices && triangles && cum && xyzrgb && tri, name, "null pointer");
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(ceil_div((long long)s * n, 64)), dim3(64), 0, (hipStream_t)stream, s,
                       vert_offsets, tri_offsets, (int)num_vertices, (int)num_triangles, vertices, colors, triangles,
                       (const u64 *)cum, mesh_ids, n, (u64)first_index, (u64)seed, xyzrgb, tri, normal);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_mesh_gather_rows(int s, int k, const int *idx, long long rows_per_set, const void *src,
                                           long long src_row_stride, int cols, int elem_bytes, void *dst,
                                           long long dst_row_stride, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_mesh_gather_rows";
    CLOUDAAE_REQUIRE(s >= 1 && k >= 1 && cols >= 1, name, "s, k and cols must be >= 1");
    CLOUDAAE_REQUIRE(rows_per_set >= 1 && (long long)s * rows_per_set <= MS_MAX_TOTAL, name,
                     "rows_per_set must be >= 1 and s * rows_per_set <= 2^28");
    CLOUDAAE_REQUIRE((long long)s * k <= MS_MAX_TOTAL && (long long)s * k * cols <= (1ll << 32), name,
                     "s * k above 2^28 or s * k * cols above 2^32");
    CLOUDAAE_REQUIRE(elem_bytes == 4 || elem_bytes == 8, name, "elem_bytes must be 4 or 8");
    CLOUDAAE_REQUIRE(src_row_stride >= cols && dst_row_stride >= cols, name, "a row stride below cols");
    CLOUDAAE_REQUIRE(idx != nullptr || k <= rows_per_set, name, "without idx, k must be <= rows_per_set");
    CLOUDAAE_REQUIRE(src && dst, name, "null pointer");
    const long long total = (long long)s * k * cols;
    if (elem_bytes == 4)
        hipLaunchKernelGGL(mesh_gather_rows_kernel<unsigned>, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, total,
                           k, cols, idx, rows_per_set, (const unsigned *)src, src_row_stride, (unsigned *)dst, dst_row_stride);
    else
        hipLaunchKernelGGL(mesh_gather_rows_kernel<u64>, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, total, k,
                           cols, idx, rows_per_set, (const u64 *)src, src_row_stride, (u64 *)dst, dst_row_stride);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
