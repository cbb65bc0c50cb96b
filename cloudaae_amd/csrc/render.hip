// render.hip -- depth and label frames of posed triangle meshes on the GPU (gfx950): a z-buffer rasteriser whose every
// output is an integer.
//
// DESIGN.md, "Rendered frames", is the definition; tests/render_reference.py restates it in NumPy with integer
// arithmetic.  Vertices go through the pose and the pinhole projection in fp64 on the widened fp32 inputs (un-fused:
// the file is compiled with -ffp-contract=off) and land on a fixed-point grid of 1/256 pixel.  Edge functions are
// int64 and exact inside the guard band, the depth of a sample is one fp64 expression, and the depth test is a 64-bit
// integer minimum on (quantised depth << 32 | draw rank): the result does not depend on the order of execution.
//
//   cloudaae_render_frames   four memsets and four launches: vertices (one lane per instance vertex); triangle setup
//                            with the small triangles rasterised by their lane and the large ones queued; the queue,
//                            one wave per triangle; the resolve, one lane per pixel
#include "common.h"
#include "depth_frame.h"
#include "pose_math.h"
#include "workspace.h"
#include "../../include/cloudaae_hip.h"
#include <math.h>

namespace cloudaae {

// a clamped box of at most this many samples is rasterised by the setup lane (tests/test_25_render_gpu.py reads the
// number; profiles/notes_render.md has the comparison, for which tools/bench_render.py takes libraries built with -D)
#ifndef CLOUDAAE_RN_SMALL
#define CLOUDAAE_RN_SMALL 16
#endif
constexpr int RN_SMALL = CLOUDAAE_RN_SMALL;
constexpr int RN_BLOCK = 256;
constexpr int RN_QUEUE_BLOCKS = 1024;      // the fixed grid that strides over the queue: 4096 waves
constexpr int RN_FRAC = 8;                 // fractional bits of a screen coordinate
constexpr double RN_GUARD = 16777216.0;    // |ix|, |iy| <= 2^24: differences below 2^26, edge values below 2^52
constexpr int RN_UNUSABLE = INT32_MIN;     // ix of a vertex that no triangle may use
constexpr long long RN_MAX_TOTAL = 1ll << 28;      // vertices and triangles of the packed meshes
constexpr long long RN_MAX_RANK = (1ll << 31) - 1; // instance triangles (and instance vertices) of a call
constexpr int RN_MAX_MESH_TRIANGLES = 1 << 24;
constexpr int RN_MAX_MESHES = 65535;
typedef unsigned long long u64;
constexpr u64 RN_EMPTY = ~0ull;

struct RenderArgs {
    int s, nv, nt;                         // the packed meshes
    const int *vert_offsets, *tri_offsets;
    const float *vertices;
    const int *triangles;
    int f, h, w;
    const float *intrinsics;
    const int *inst_offsets;
    int j;
    const int *inst_mesh, *inst_label;
    const double *inst_pose;
    const int *vert_base, *tri_base;       // [j+1]: exclusive prefix sums of the instances' vertex / triangle counts
    int sum_v, sum_t;
    double z_near;
    // workspace
    u64 *zbuf;
    int *vx, *vy;
    double *viz;
    int *queue, *queue_len;
    // outputs
    int *dropped, *degenerate;
};

// the last i in [0, n) with base[i] <= g (entries with an empty range are stepped over); -1 when there is none
__device__ __forceinline__ int rn_owner(const int *__restrict__ base, int n, int g)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (base[mid] <= g)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

// the ranges of instance j's mesh; false (an instance without vertices and triangles) when the mesh id or its offsets
// do not describe ranges inside the packed arrays
__device__ __forceinline__ bool rn_mesh(const RenderArgs &a, int j, int &v0, int &v1, int &t0, int &t1)
{
    const int m = a.inst_mesh[j];
    if (m < 0 || m >= a.s)
        return false;
    v0 = a.vert_offsets[m];
    v1 = a.vert_offsets[m + 1];
    t0 = a.tri_offsets[m];
    t1 = a.tri_offsets[m + 1];
    return v0 >= 0 && v0 <= v1 && v1 <= a.nv && t0 >= 0 && t0 <= t1 && t1 <= a.nt;
}

// one lane per (instance, vertex): the pose, the projection, the fixed-point grid
__global__ __launch_bounds__(RN_BLOCK) void render_vertex_kernel(RenderArgs a)
{
    const long long gl = (long long)blockIdx.x * RN_BLOCK + threadIdx.x;
    if (gl >= a.sum_v)
        return;
    const int g = (int)gl;
    int ix = RN_UNUSABLE, iy = 0;
    double iz = 0.0;
    const int j = rn_owner(a.vert_base, a.j, g);
    int v0, v1, t0, t1;
    if (j >= 0 && rn_mesh(a, j, v0, v1, t0, t1)) {
        const int v = g - a.vert_base[j];
        const int fr = rn_owner(a.inst_offsets, a.f + 1, j);
        if (v < v1 - v0 && fr >= 0 && fr < a.f) {
            const float *p = a.vertices + 3 * (size_t)(v0 + v);
            const float *k = a.intrinsics + 5 * (size_t)fr;
            double X, Y, Z;
            icp_apply(a.inst_pose + 16 * (size_t)j, (double)p[0], (double)p[1], (double)p[2], X, Y, Z);
            const double sx = ((double)k[0] * X) / Z + (double)k[2];
            const double sy = ((double)k[1] * Y) / Z + (double)k[3];
            const double fx = floor(sx * 256.0 + 0.5), fy = floor(sy * 256.0 + 0.5);
            // (a NaN fails every comparison: unusable)
            if (isfinite(Z) && Z >= a.z_near && fabs(fx) <= RN_GUARD && fabs(fy) <= RN_GUARD) {
                ix = (int)fx;
                iy = (int)fy;
                iz = 1.0 / Z;
            }
        }
    }
    a.vx[g] = ix;
    a.vy[g] = iy;
    a.viz[g] = iz;
}

struct RenderTri {
    long long ax, ay, bx, by, cx, cy, area2;
    double iza, izb, izc, factor;
    int u0, u1, v0, v1;                    // the clamped box of samples, inclusive; empty when u1 < u0 or v1 < v0
    int frame;
};

// the setup of draw rank g.  0: drawable (tri is filled in); 1: no such triangle; 2: dropped; 3: degenerate.  j is the
// instance (for the counts).
__device__ __forceinline__ int rn_setup(const RenderArgs &a, int g, RenderTri &tri, int &j)
{
    j = rn_owner(a.tri_base, a.j, g);
    int v0, v1, t0, t1;
    if (j < 0 || !rn_mesh(a, j, v0, v1, t0, t1))
        return 1;
    const int t = g - a.tri_base[j];
    const int fr = rn_owner(a.inst_offsets, a.f + 1, j);
    if (t >= t1 - t0 || fr < 0 || fr >= a.f)
        return 1;
    const long long vb = a.vert_base[j];
    int x[3], y[3];
    double z[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = a.triangles[3 * (size_t)(t0 + t) + k];
        if (i < 0 || i >= v1 - v0 || vb + i >= a.sum_v)
            return 2;
        x[k] = a.vx[vb + i];
        y[k] = a.vy[vb + i];
        z[k] = a.viz[vb + i];
        if (x[k] == RN_UNUSABLE)
            return 2;
    }
    long long area2 = (long long)(x[1] - x[0]) * (y[2] - y[0]) - (long long)(y[1] - y[0]) * (x[2] - x[0]);
    if (area2 == 0)
        return 3;
    int b = 1, c = 2;
    if (area2 < 0) {
        b = 2;
        c = 1;
        area2 = -area2;
    }
    tri.ax = x[0], tri.ay = y[0], tri.bx = x[b], tri.by = y[b], tri.cx = x[c], tri.cy = y[c];
    tri.area2 = area2;
    tri.iza = z[0], tri.izb = z[b], tri.izc = z[c];
    tri.factor = (double)a.intrinsics[5 * (size_t)fr + 4];
    tri.frame = fr;
    const int xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
    const int ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
    // samples lie at the multiples of 256: the first at or after the minimum, the last at or before the maximum
    tri.u0 = max((xmin + 255) >> RN_FRAC, 0);
    tri.u1 = min(xmax >> RN_FRAC, a.w - 1);
    tri.v0 = max((ymin + 255) >> RN_FRAC, 0);
    tri.v1 = min(ymax >> RN_FRAC, a.h - 1);
    return 0;
}

// one sample of one triangle: coverage, depth, the depth test
__device__ __forceinline__ void rn_sample(const RenderArgs &a, const RenderTri &t, int rank, int u, int v)
{
    const long long px = (long long)u << RN_FRAC, py = (long long)v << RN_FRAC;
    const long long wa = (t.cx - t.bx) * (py - t.by) - (t.cy - t.by) * (px - t.bx);
    const long long wb = (t.ax - t.cx) * (py - t.cy) - (t.ay - t.cy) * (px - t.cx);
    const long long wc = (t.bx - t.ax) * (py - t.ay) - (t.by - t.ay) * (px - t.ax);
    if (wa < 0 || wb < 0 || wc < 0)
        return;
    const double q = ((double)wa * t.iza + (double)wb * t.izb) + (double)wc * t.izc;
    const double z = (double)t.area2 / q;
    const double du = floor(z * t.factor + 0.5);
    if (!(du >= 1.0 && du <= 65535.0))
        return;
    const u64 key = ((u64)(unsigned)(int)du << 32) | (u64)(unsigned)rank;
    u64 *cell = a.zbuf + ((size_t)t.frame * a.h + v) * a.w + u;
    // the plain read only spares atomics: the cell never grows, so what it shows is never below the final minimum
    if (key < __atomic_load_n(cell, __ATOMIC_RELAXED))
        __hip_atomic_fetch_min(cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one lane per (instance, triangle) = per draw rank: the setup, the counts, the small boxes; the others are queued
__global__ __launch_bounds__(RN_BLOCK) void render_setup_kernel(RenderArgs a)
{
    const long long gl = (long long)blockIdx.x * RN_BLOCK + threadIdx.x;
    bool large = false;
    const int g = (int)gl;
    if (gl < a.sum_t) {
        RenderTri t;
        int j;
        const int what = rn_setup(a, g, t, j);
        if (what == 2)
            __hip_atomic_fetch_add(a.dropped + j, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (what == 3)
            __hip_atomic_fetch_add(a.degenerate + j, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (what == 0 && t.u1 >= t.u0 && t.v1 >= t.v0) {
            const long long count = (long long)(t.u1 - t.u0 + 1) * (t.v1 - t.v0 + 1);
            if (count <= RN_SMALL) {
                for (int v = t.v0; v <= t.v1; ++v)
                    for (int u = t.u0; u <= t.u1; ++u)
                        rn_sample(a, t, g, u, v);
            } else {
                large = true;
            }
        }
    }
    // wave-aggregated append: one integer atomic per wave, the lanes' slots by their position among the appending lanes
    const u64 mask = __builtin_amdgcn_ballot_w64(large);
    if (mask) {
        const int lane = lane_id();
        const int leader = __builtin_ctzll(mask);
        int first = 0;
        if (lane == leader)
            first = __hip_atomic_fetch_add(a.queue_len, __builtin_popcountll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        first = __builtin_amdgcn_readlane(first, leader);
        if (large) {
            const int slot = first + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
            if (slot < a.sum_t)                // (always: every rank is appended once at most)
                a.queue[slot] = g;
        }
    }
}

// a fixed grid of waves strides over the queue: one wave per triangle, its lanes tile the clamped box in 8 x 8 blocks
__global__ __launch_bounds__(RN_BLOCK) void render_queue_kernel(RenderArgs a)
{
    const int len = min(*a.queue_len, a.sum_t);
    const int waves = gridDim.x * (RN_BLOCK / 64);
    const int lane = lane_id(), lx = lane & 7, ly = lane >> 3;
    for (int q = blockIdx.x * (RN_BLOCK / 64) + (int)(threadIdx.x >> 6); q < len; q += waves) {
        const int g = a.queue[q];
        if (g < 0 || g >= a.sum_t)
            continue;
        RenderTri t;
        int j;
        if (rn_setup(a, g, t, j) != 0)
            continue;
        for (int vb = t.v0; vb <= t.v1; vb += 8)
            for (int ub = t.u0; ub <= t.u1; ub += 8) {
                const int u = ub + lx, v = vb + ly;
                if (u <= t.u1 && v <= t.v1)
                    rn_sample(a, t, g, u, v);
            }
    }
}

// one lane per pixel: key -> depth, label, rank
__global__ __launch_bounds__(RN_BLOCK) void render_resolve_kernel(long long pixels, const u64 *__restrict__ zbuf, int j,
                                                          const int *__restrict__ tri_base,
                                                          const int *__restrict__ inst_label,
                                                          unsigned short *__restrict__ depth,
                                                          unsigned char *__restrict__ label, int *__restrict__ tri)
{
    const long long p = (long long)blockIdx.x * RN_BLOCK + threadIdx.x;
    if (p >= pixels)
        return;
    const u64 key = zbuf[p];
    unsigned short d = 0;
    unsigned char l = 0;
    int r = -1;
    if (key != RN_EMPTY) {
        r = (int)(unsigned)(key & 0xffffffffull);
        const int i = rn_owner(tri_base, j, r);
        d = (unsigned short)(key >> 32);
        l = i >= 0 ? (unsigned char)inst_label[i] : 0;
    }
    depth[p] = d;
    label[p] = l;
    if (tri)
        tri[p] = r;
}

static bool rn_within_limits(long long f, long long h, long long w, long long j, long long sum_v, long long sum_t)
{
    return frame_within_limits(1, f, h, w) && j >= 1 && j <= RN_MAX_RANK && sum_v >= 0 && sum_v <= RN_MAX_RANK && sum_t >= 0 &&
           sum_t <= RN_MAX_RANK &&
           sum_t <= j * RN_MAX_MESH_TRIANGLES;     // (what the sums can show of "at most 2^24 triangles per mesh")
}

// the workspace pointers of a (null workspace: the size alone is asked for); returns the workspace's bytes
static size_t rn_carve(RenderArgs &a, size_t pixels, size_t sum_v, size_t sum_t, void *workspace)
{
    Carver ws(workspace);
    a.zbuf = ws.take<u64>(pixels);
    a.viz = ws.take<double>(sum_v);
    a.vx = ws.take<int>(sum_v);
    a.vy = ws.take<int>(sum_v);
    a.queue = ws.take<int>(sum_t);
    a.queue_len = ws.take<int>(1);
    return ws.bytes();
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API long long cloudaae_render_workspace_bytes(int f, int h, int w, int j, long long sum_inst_vertices,
                                                       long long sum_inst_triangles)
{
    if (!rn_within_limits(f, h, w, j, sum_inst_vertices, sum_inst_triangles))
        return 0;
    RenderArgs a;
    return (long long)rn_carve(a, (size_t)f * h * w, (size_t)sum_inst_vertices, (size_t)sum_inst_triangles, nullptr);
}

CLOUDAAE_API int cloudaae_render_frames(int s, const int *vert_offsets, const int *tri_offsets, long long num_vertices,
                                        long long num_triangles, const float *vertices, const int *triangles, int f, int h,
                                        int w, const float *intrinsics, const int *inst_offsets, int j, const int *inst_mesh,
                                        const int *inst_label, const double *inst_pose, const int *inst_vert_base,
                                        const int *inst_tri_base, long long sum_inst_vertices, long long sum_inst_triangles,
                                        double z_near, uint16_t *depth, uint8_t *label, int *tri, int *dropped,
                                        int *degenerate, void *workspace, long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_render_frames";
    CLOUDAAE_REQUIRE(s >= 1 && s <= RN_MAX_MESHES, name, "s must lie in [1, 65535]");
    CLOUDAAE_REQUIRE(num_vertices >= 1 && num_vertices <= RN_MAX_TOTAL, name, "num_vertices must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(num_triangles >= 1 && num_triangles <= RN_MAX_TOTAL, name, "num_triangles must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(rn_within_limits(f, h, w, j, sum_inst_vertices, sum_inst_triangles), name,
                     "outside the limits: f, h, w, j >= 1; h * w <= 2^24; f * h * w <= 2^28; instance vertices and triangles "
                     "(the draw ranks) below 2^31; at most 2^24 triangles per mesh");
    CLOUDAAE_REQUIRE(z_near > 0.0 && isfinite(z_near), name, "z_near must be positive and finite");
    CLOUDAAE_REQUIRE(vert_offsets && tri_offsets && vertices && triangles && intrinsics && inst_offsets && inst_mesh &&
                         inst_label && inst_pose && inst_vert_base && inst_tri_base && depth && label && dropped &&
                         degenerate && workspace,
                     name, "null pointer");
    const size_t pixels = (size_t)f * h * w, sv = (size_t)sum_inst_vertices, st = (size_t)sum_inst_triangles;
    RenderArgs a;
    CLOUDAAE_REQUIRE(workspace_bytes >= (long long)rn_carve(a, pixels, sv, st, workspace), name,
                     "workspace smaller than cloudaae_render_workspace_bytes");
    a.s = s, a.nv = (int)num_vertices, a.nt = (int)num_triangles;
    a.vert_offsets = vert_offsets, a.tri_offsets = tri_offsets, a.vertices = vertices, a.triangles = triangles;
    a.f = f, a.h = h, a.w = w, a.intrinsics = intrinsics, a.inst_offsets = inst_offsets;
    a.j = j, a.inst_mesh = inst_mesh, a.inst_label = inst_label, a.inst_pose = inst_pose;
    a.vert_base = inst_vert_base, a.tri_base = inst_tri_base, a.sum_v = (int)sv, a.sum_t = (int)st;
    a.z_near = z_near;
    a.dropped = dropped, a.degenerate = degenerate;
    hipStream_t sm = (hipStream_t)stream;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(a.zbuf, 0xFF, 8 * pixels, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(a.queue_len, 0, sizeof(int), sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(dropped, 0, sizeof(int) * (size_t)j, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(degenerate, 0, sizeof(int) * (size_t)j, sm), name);
    if (sv > 0 && st > 0) {
        hipLaunchKernelGGL(render_vertex_kernel, dim3(ceil_div((long long)sv, RN_BLOCK)), dim3(RN_BLOCK), 0, sm, a);
        CLOUDAAE_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(render_setup_kernel, dim3(ceil_div((long long)st, RN_BLOCK)), dim3(RN_BLOCK), 0, sm, a);
        CLOUDAAE_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(render_queue_kernel, dim3(RN_QUEUE_BLOCKS), dim3(RN_BLOCK), 0, sm, a);
        CLOUDAAE_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(render_resolve_kernel, dim3(ceil_div((long long)pixels, RN_BLOCK)), dim3(RN_BLOCK), 0, sm,
                       (long long)pixels, (const u64 *)a.zbuf, j, inst_tri_base, inst_label, (unsigned short *)depth,
                       (unsigned char *)label, tri);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
