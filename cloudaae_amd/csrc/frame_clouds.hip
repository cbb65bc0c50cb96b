// frame_clouds.hip -- fixed-size clouds drawn from the labelled pixels of depth / label frames on the GPU (gfx950): the
// step between cloudaae_render_frames / cloudaae_depth_sensor_noise and the training step, which takes [B,N,3] and
// [B,4N,3] clouds.  DESIGN.md, "Rendered training clouds", is the definition; tests/frame_clouds_reference.py restates it
// in NumPy.  Every output is a pure function of the frame's bytes and (seed, the cloud's global index g): ranks come
// from ballots and two prefix sums, there is no atomic of any kind, nothing is read back, and no workgroup waits for
// another.  The back-projection is that of segment.hip in fp32, un-fused (the file is compiled with -ffp-contract=off).
//
//   cloudaae_frame_clouds   four launches: the masked pixels per (cloud, tile of 1024 pixels); one workgroup per cloud
//                           that turns the tile counts into their exclusive prefix and writes n; the scatter (rank =
//                           tile prefix + the earlier waves of the tile + the earlier lanes of the wave; the lane decides
//                           for itself whether its pixel is a row, back-projects and writes); the rows that are re-draws
//                           or the fallback, one lane per (cloud, row)
#include "common.h"
#include "depth_frame.h"
#include "philox.h"
#include "workspace.h"
#include "../../include/cloudaae_hip.h"

namespace cloudaae {

typedef unsigned long long u64;

constexpr int FC_BLOCK = 256;
constexpr int FC_WAVES = FC_BLOCK / 64;
constexpr int FC_PASSES = 4;                       // pixels per lane
constexpr int FC_TILE = FC_BLOCK * FC_PASSES;      // pixels per workgroup, in pixel order: pass, wave, lane
constexpr unsigned FC_STREAM_STRATUM = 23u;        // r0 of counter g 2^24 + j: the pixel of stratum j (n >= rows)
constexpr unsigned FC_STREAM_REDRAW = 24u;         // r0 of counter g 2^24 + j: the source of row j >= n (n < rows)
constexpr long long FC_MAX_ROWS = 1ll << 20;
constexpr long long FC_MAX_INDEX = 1ll << 39;      // global cloud indices lie below
constexpr long long FC_MAX_GRID = (1ll << 31) - 1; // c * tiles and c * rows

struct FcArgs {
    int f, h, w, c, rows, tiles;
    const unsigned short *depth;
    const unsigned char *label;
    const float *intrinsics;
    const int *frame_of, *want;
    const long long *index;
    const float *fallback;                         // may be null: zeros
    u64 seed;
    int *tile_prefix;                              // workspace [c, tiles]: counts, then their exclusive prefix
    float *cloud;
    int *num_pixels;
    long long *num_distinct;
    int *row_src;
};

// the frame cloud c reads, or -1: a frame outside [0, f) or a global index outside [0, 2^39) makes the cloud the n = 0
// case, and nothing of the frames is read for it
__device__ __forceinline__ int fc_frame(const FcArgs &a, int c)
{
    const int fr = a.frame_of[c];
    const long long g = a.index[c];
    return (fr >= 0 && fr < a.f && g >= 0 && g < FC_MAX_INDEX) ? fr : -1;
}

// whether pixel p of the tile's pass belongs to the mask (p < h w is part of it)
__device__ __forceinline__ bool fc_masked(const FcArgs &a, int fr, int want, int p, unsigned short &d)
{
    d = 0;
    if (fr < 0 || p >= a.h * a.w)
        return false;
    const size_t i = (size_t)fr * ((size_t)a.h * a.w) + p;
    if ((int)a.label[i] != want)
        return false;
    d = a.depth[i];
    return d != 0;
}

// grid = c * tiles: workgroup b counts the masked pixels of tile b % tiles of cloud b / tiles
__global__ __launch_bounds__(FC_BLOCK) void frame_clouds_count_kernel(FcArgs a)
{
    __shared__ int red[FC_WAVES];
    const int c = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = fc_frame(a, c), want = a.want[c];
    int total = 0;
#pragma unroll
    for (int pass = 0; pass < FC_PASSES; ++pass) {
        unsigned short d;
        const bool m = fc_masked(a, fr, want, tile * FC_TILE + pass * FC_BLOCK + tid, d);
        total += __builtin_popcountll(__builtin_amdgcn_ballot_w64(m));
    }
    if (lane == 0)
        red[wv] = total;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
#pragma unroll
        for (int q = 0; q < FC_WAVES; ++q)
            sum += red[q];
        a.tile_prefix[(size_t)c * a.tiles + tile] = sum;
    }
}

// grid = c: one workgroup turns the cloud's tile counts into their exclusive prefix, 256 at a time (a Hillis-Steele
// scan in LDS), and writes n and num_distinct
__global__ __launch_bounds__(FC_BLOCK) void frame_clouds_scan_kernel(FcArgs a)
{
    __shared__ int buf[2][FC_BLOCK];
    const int c = blockIdx.x, tid = threadIdx.x;
    int *counts = a.tile_prefix + (size_t)c * a.tiles;
    int carry = 0;
    for (int base = 0; base < a.tiles; base += FC_BLOCK) {
        const int t = base + tid;
        const int mine = t < a.tiles ? counts[t] : 0;
        int cur = 0;
        buf[0][tid] = mine;
        __syncthreads();
#pragma unroll
        for (int off = 1; off < FC_BLOCK; off <<= 1) {
            const int v = buf[cur][tid] + (tid >= off ? buf[cur][tid - off] : 0);
            buf[cur ^ 1][tid] = v;
            cur ^= 1;
            __syncthreads();
        }
        if (t < a.tiles)
            counts[t] = carry + buf[cur][tid] - mine;
        carry += buf[cur][FC_BLOCK - 1];
        __syncthreads();                           // the next round writes buf[0]
    }
    if (tid == 0) {
        a.num_pixels[c] = carry;
        a.num_distinct[c] = carry >= a.rows ? (long long)a.rows : (carry >= 1 ? (long long)carry : 1ll);
    }
}

// row j of cloud c: the back-projection of pixel p with depth d
__device__ __forceinline__ void fc_write_row(const FcArgs &a, int c, int fr, int j, int p, unsigned short d)
{
    float q[3];
    backproject(pinhole<float>(a.intrinsics + 5 * (size_t)fr), p % a.w, p / a.w, d, q);
    const size_t o = (size_t)c * a.rows + j;
    a.cloud[3 * o + 0] = q[0];
    a.cloud[3 * o + 1] = q[1];
    a.cloud[3 * o + 2] = q[2];
    a.row_src[o] = j;
}

// grid = c * tiles, as the count: every masked lane forms its rank and decides whether its pixel is a row
__global__ __launch_bounds__(FC_BLOCK) void frame_clouds_scatter_kernel(FcArgs a)
{
    __shared__ int part[FC_PASSES * FC_WAVES];
    const int c = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = fc_frame(a, c);
    if (fr < 0)                                    // (the whole workgroup: before any barrier)
        return;
    const int want = a.want[c];
    const int n = a.num_pixels[c];
    bool m[FC_PASSES];
    unsigned short d[FC_PASSES];
    int before[FC_PASSES];                         // masked lanes of this wave and pass below this lane
#pragma unroll
    for (int pass = 0; pass < FC_PASSES; ++pass) {
        m[pass] = fc_masked(a, fr, want, tile * FC_TILE + pass * FC_BLOCK + tid, d[pass]);
        const u64 mask = __builtin_amdgcn_ballot_w64(m[pass]);
        before[pass] = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (lane == 0)
            part[pass * FC_WAVES + wv] = __builtin_popcountll(mask);
    }
    __syncthreads();
    int rank0 = a.tile_prefix[(size_t)c * a.tiles + tile];
    const u64 g = (u64)a.index[c];
    const long long rows = a.rows;
#pragma unroll
    for (int pass = 0; pass < FC_PASSES; ++pass) {
        int earlier = 0;                           // the pixels of the tile in front of this wave's pass
#pragma unroll
        for (int q = 0; q < FC_PASSES * FC_WAVES; ++q)
            earlier += q < pass * FC_WAVES + wv ? part[q] : 0;
        if (!m[pass])
            continue;
        const int r = rank0 + earlier + before[pass];
        const int p = tile * FC_TILE + pass * FC_BLOCK + tid;
        if (r >= n)                                // (never: n is the sum of the same counts)
            continue;
        if (n < a.rows) {
            fc_write_row(a, c, fr, r, p, d[pass]);
            continue;
        }
        // the stratum of rank r, its bounds, and the one rank of it that the draw picks
        const long long j = (((long long)r + 1) * rows - 1) / n;
        const long long s0 = (j * n) / rows, s1 = ((j + 1) * n) / rows;
        unsigned q4[4];
        philox4x32(a.seed, (g << 24) + (u64)j, FC_STREAM_STRATUM, q4);
        const long long pick = s0 + (long long)(((u64)q4[0] * (u64)(s1 - s0)) >> 32);
        if ((long long)r == pick && j < rows)
            fc_write_row(a, c, fr, (int)j, p, d[pass]);
    }
}

// one lane per (cloud, row): the fallback rows of an empty mask and the re-drawn rows j >= n of a small one
__global__ __launch_bounds__(FC_BLOCK) void frame_clouds_fill_kernel(FcArgs a)
{
    const long long gl = (long long)blockIdx.x * FC_BLOCK + threadIdx.x;
    if (gl >= (long long)a.c * a.rows)
        return;
    const int c = (int)(gl / a.rows), j = (int)(gl % a.rows);
    const int n = a.num_pixels[c];
    if (n >= a.rows || (n >= 1 && j < n))
        return;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    int src = 0;
    float *dst = a.cloud + 3 * (size_t)gl;
    if (n == 0) {
        if (a.fallback) {
            x = a.fallback[3 * (size_t)c + 0];
            y = a.fallback[3 * (size_t)c + 1];
            z = a.fallback[3 * (size_t)c + 2];
        }
    } else {
        unsigned q4[4];
        philox4x32(a.seed, ((u64)a.index[c] << 24) + (u64)j, FC_STREAM_REDRAW, q4);
        src = (int)(((u64)q4[0] * (u64)n) >> 32);
        const float *s = a.cloud + 3 * ((size_t)c * a.rows + src);      // a row below n: written by the scatter
        x = s[0], y = s[1], z = s[2];
    }
    dst[0] = x;
    dst[1] = y;
    dst[2] = z;
    a.row_src[gl] = src;
}

static int fc_tiles(long long h, long long w) { return (int)((h * w + FC_TILE - 1) / FC_TILE); }

static bool fc_within_limits(long long f, long long h, long long w, long long c, long long rows)
{
    return frame_within_limits(1, f, h, w) && c >= 1 && rows >= 1 && rows <= FC_MAX_ROWS && c * fc_tiles(h, w) <= FC_MAX_GRID &&
           c * rows <= FC_MAX_GRID;
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API long long cloudaae_frame_clouds_workspace_bytes(int f, int h, int w, int c, int rows)
{
    if (!fc_within_limits(f, h, w, c, rows))
        return 0;
    return (long long)workspace_pad((size_t)c * fc_tiles(h, w) * sizeof(int));
}

CLOUDAAE_API int cloudaae_frame_clouds(int f, int h, int w, const uint16_t *depth, const uint8_t *label, const float *intrinsics,
                                       int c, const int *frame_of, const int *want, const long long *index,
                                       const float *fallback, int rows, unsigned long long seed, float *cloud,
                                       int *num_pixels, long long *num_distinct, int *row_src, void *workspace,
                                       long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_frame_clouds";
    CLOUDAAE_REQUIRE(fc_within_limits(f, h, w, c, rows), name,
                     "outside the limits: f, h, w, c >= 1; h * w <= 2^24; f * h * w <= 2^28; 1 <= rows <= 2^20; c * rows and "
                     "c * ceil(h * w / 1024) below 2^31");
    CLOUDAAE_REQUIRE(depth && label && intrinsics && frame_of && want && index && cloud && num_pixels && num_distinct &&
                         row_src && workspace,
                     name, "null pointer");
    CLOUDAAE_REQUIRE(workspace_bytes >= cloudaae_frame_clouds_workspace_bytes(f, h, w, c, rows), name,
                     "workspace smaller than cloudaae_frame_clouds_workspace_bytes");
    FcArgs a;
    a.f = f, a.h = h, a.w = w, a.c = c, a.rows = rows, a.tiles = fc_tiles(h, w);
    a.depth = (const unsigned short *)depth, a.label = (const unsigned char *)label, a.intrinsics = intrinsics;
    a.frame_of = frame_of, a.want = want, a.index = index, a.fallback = fallback, a.seed = seed;
    a.tile_prefix = (int *)workspace;
    a.cloud = cloud, a.num_pixels = num_pixels, a.num_distinct = num_distinct, a.row_src = row_src;
    hipStream_t sm = (hipStream_t)stream;
    const unsigned tiles_grid = (unsigned)((long long)c * a.tiles);
    hipLaunchKernelGGL(frame_clouds_count_kernel, dim3(tiles_grid), dim3(FC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(frame_clouds_scan_kernel, dim3((unsigned)c), dim3(FC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(frame_clouds_scatter_kernel, dim3(tiles_grid), dim3(FC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(frame_clouds_fill_kernel, dim3(ceil_div((long long)c * rows, FC_BLOCK)), dim3(FC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
