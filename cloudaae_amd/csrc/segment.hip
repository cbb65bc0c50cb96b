// segment.hip -- evaluation inputs from RGB-D frames: the segment pipeline of the reference's evaluation
// (evaluate_cloudAAE_ycbv.py:164-271: back-projection, per-class mask, mean-distance filter, open3d's radius outlier
// removal, FPS_random).  The definition the kernels implement is written out in DESIGN.md ("Frame segments") and
// restated in NumPy by tests/segment_reference.py.  Every result is bit-reproducible and does not depend on the batch:
// integer counts only are combined with atomics, and the one floating-point sum (the segment mean) is taken in pixel
// order by one lane per coordinate.
//
//   cloudaae_frame_segments  (10 launches + a memset)  F frames -> S segments of filtered points, packed in segment order
//     fs_table      : (frame, class) -> segment (atomicMax: a pair named twice keeps its last segment)
//     fs_count      : per 256-pixel block, the number of masked pixels of each class (LDS integer atomics)
//     fs_seg_scan   : per segment, the exclusive scan of its block counts; one workgroup per segment
//     scan          : the masked segments' offsets (one workgroup)
//     fs_scatter    : masked points in pixel order: block offset + rank among the block's pixels of the class
//     fs_mean       : per segment and coordinate, the fp64 sum in pixel order, / count, rounded to fp32
//     filter + compact (compact_* below) -> the filtered points and their offsets
//   cloudaae_radius_outlier  (8 launches + a memset)
//     seg_fill      : the segment of each point
//     ro_grid       : per segment, a uniform grid of cells of edge >= r over its bounding box (counting sort in LDS)
//     ro_count      : per point, neighbours in the 27 cells, stopping once the count passes nb_points
//     inlier flags with the min_keep fallback + compact -> inlier points, local indices, counts
//   cloudaae_ragged_fps      (1 launch)  one workgroup per set; fp64 distances in registers, beyond a bound in memory
//
// Point counts are bounded by F*H*W (a pixel belongs to one segment at most), so every buffer is sized without
// reading a count back; grids are sized by that bound and blocks past the device-side total do nothing.
#include "common.h"
#include "depth_frame.h"
#include "workspace.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

using namespace cloudaae;

namespace {

constexpr int SEG_BLOCK = 256;             // pixels / points per block of the pixel and compaction passes
constexpr int SEG_CLASSES = 256;           // label values 1..255 -> classes 0..254
constexpr int SEG_SCAN_THREADS = 1024;
constexpr int RO_THREADS = 1024;
constexpr int RO_GRID_MAX = 32;            // cells per axis at most: 32^3 cell counts in LDS (128 KiB)
constexpr int RO_CELLS = RO_GRID_MAX * RO_GRID_MAX * RO_GRID_MAX;
constexpr int FPS_THREADS = 512;
constexpr int FPS_WAVES = FPS_THREADS / 64;
constexpr int FPS_PER_LANE = 24;           // points held in registers: 12288 per set; the rest in the workspace
constexpr int FPS_REG_POINTS = FPS_THREADS * FPS_PER_LANE;

// ---- one workgroup: exclusive scan of n ints in[i * stride] -> out[i], out[n] = total ------------------------------
__device__ void block_exclusive_scan(const int *in, long long stride, int n, int *out, int *lds /*[blockDim]*/)
{
    const int t = threadIdx.x, T = blockDim.x;
    const int chunk = (n + T - 1) / T;
    const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
    int sum = 0;
    for (int i = lo; i < hi; ++i)
        sum += in[(long long)i * stride];
    lds[t] = sum;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {
        const int v = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += v;
        __syncthreads();
    }
    int run = lds[t] - sum;
    for (int i = lo; i < hi; ++i) {
        const int v = in[(long long)i * stride];
        out[i] = run;
        run += v;
    }
    if (t == T - 1)
        out[n] = lds[T - 1];
    __syncthreads();
}

// rank of this lane among the active-flagged lanes below it, and the wave's count (wave64)
__device__ __forceinline__ int wave_rank(bool flag, int &wave_count)
{
    const unsigned long long m = __ballot(flag);
    wave_count = __popcll(m);
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long below = lane ? (m & ((~0ull) >> (64 - lane))) : 0ull;
    return __popcll(below);
}

// ---- frame segments ---------------------------------------------------------------------------------------------

__global__ void fs_table_kernel(int f, int s, const int *seg_frame, const int *seg_class, int *table)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s)
        return;
    const int fr = seg_frame[i], c = seg_class[i];
    if (fr >= 0 && fr < f && c >= 0 && c < SEG_CLASSES - 1)
        atomicMax(&table[fr * SEG_CLASSES + c], i);
}

// the segment of a pixel, or -1: label - 1 == class of a listed segment and depth != 0
__device__ __forceinline__ int fs_pixel_segment(const uint16_t *depth, const uint8_t *label, const int *table, int fr,
                                                long long p)
{
    const int c = (int)label[p] - 1;
    if (c < 0 || depth[p] == 0)
        return -1;
    return table[fr * SEG_CLASSES + c];
}

__global__ __launch_bounds__(SEG_BLOCK) void fs_count_kernel(int hw, int nblk, const uint16_t *depth,
                                                             const uint8_t *label, const int *table, int *blk_count)
{
    __shared__ int bins[SEG_CLASSES];
    const int fr = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    bins[t] = 0;
    __syncthreads();
    const int px = b * SEG_BLOCK + t;
    if (px < hw) {
        const long long p = (long long)fr * hw + px;
        if (fs_pixel_segment(depth, label, table, fr, p) >= 0)
            atomicAdd(&bins[(int)label[p] - 1], 1);
    }
    __syncthreads();
    blk_count[((long long)fr * nblk + b) * SEG_CLASSES + t] = bins[t];
}

// one workgroup per segment: offsets of its pixels in each block of its frame, and its size
__global__ __launch_bounds__(SEG_SCAN_THREADS) void fs_seg_scan_kernel(int f, int nblk, const int *seg_frame,
                                                                       const int *seg_class, const int *table,
                                                                       const int *blk_count, int *seg_blk_off,
                                                                       int *seg_size)
{
    __shared__ int lds[SEG_SCAN_THREADS];
    const int s = blockIdx.x;
    int *out = seg_blk_off + (long long)s * (nblk + 1);
    const int fr = seg_frame[s], c = seg_class[s];
    const bool owner = fr >= 0 && fr < f && c >= 0 && c < SEG_CLASSES - 1 && table[fr * SEG_CLASSES + c] == s;
    if (!owner) {                       // not a valid pair, or a duplicate that lost the table: an empty segment
        for (int i = threadIdx.x; i <= nblk; i += blockDim.x)
            out[i] = 0;
        if (threadIdx.x == 0)
            seg_size[s] = 0;
        return;
    }
    block_exclusive_scan(blk_count + (long long)fr * nblk * SEG_CLASSES + c, SEG_CLASSES, nblk, out, lds);
    if (threadIdx.x == 0)
        seg_size[s] = out[nblk];
}

__global__ __launch_bounds__(SEG_SCAN_THREADS) void scan_kernel(const int *in, int n, int *out)
{
    __shared__ int lds[SEG_SCAN_THREADS];
    block_exclusive_scan(in, 1, n, out, lds);
}

__global__ __launch_bounds__(SEG_BLOCK) void fs_scatter_kernel(
    int hw, int w, int nblk, const uint16_t *depth, const uint8_t *label, const float *intr, const int *table,
    const int *seg_blk_off, const int *mask_off, float *mxyz, int *mseg)
{
    __shared__ int segs[SEG_BLOCK];
    const int fr = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const int px = b * SEG_BLOCK + t;
    const long long p = (long long)fr * hw + px;
    const int s = px < hw ? fs_pixel_segment(depth, label, table, fr, p) : -1;
    segs[t] = s;
    __syncthreads();
    if (s < 0)
        return;
    int rank = 0;
    for (int j = 0; j < t; ++j)
        rank += segs[j] == s;
    float xyz[3];                                  // back-projection (:164-178) in fp32
    backproject(pinhole<float>(intr + 5 * fr), px % w, px / w, depth[p], xyz);
    const long long q = (long long)mask_off[s] + seg_blk_off[(long long)s * (nblk + 1) + b] + rank;
    mxyz[3 * q] = xyz[0];
    mxyz[3 * q + 1] = xyz[1];
    mxyz[3 * q + 2] = xyz[2];
    mseg[q] = s;
}

// one lane per (segment, coordinate): the fp64 sum in pixel order (loads batched ahead of the dependent adds)
__global__ void fs_mean_kernel(int s, const int *mask_off, const float *mxyz, float *mean)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * s)
        return;
    const int seg = i / 3, d = i % 3;
    const int lo = mask_off[seg], hi = mask_off[seg + 1];
    double sum = 0.0;
    int k = lo;
    for (; k + 8 <= hi; k += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            v[j] = mxyz[3 * (long long)(k + j) + d];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            sum += (double)v[j];
    }
    for (; k < hi; ++k)
        sum += (double)mxyz[3 * (long long)k + d];
    mean[i] = hi > lo ? (float)(sum / (double)(hi - lo)) : 0.0f;
}

// flag = sqrtf((dx^2 + dy^2) + dz^2) <= threshold in fp32 (:219-223); one count per block
__global__ __launch_bounds__(SEG_BLOCK) void fs_filter_flags_kernel(
    const int *total, long long m, const float *mxyz, const int *mseg, const float *mean, float threshold, uint8_t *flags,
    int *blk_count)
{
    __shared__ int wcount[SEG_BLOCK / 64];
    const long long i = (long long)blockIdx.x * SEG_BLOCK + threadIdx.x;
    bool keep = false;
    if (i < min((long long)*total, m)) {
        const int s = mseg[i];
        const float dx = mxyz[3 * i] - mean[3 * s], dy = mxyz[3 * i + 1] - mean[3 * s + 1];
        const float dz = mxyz[3 * i + 2] - mean[3 * s + 2];
        keep = sqrtf((dx * dx + dy * dy) + dz * dz) <= threshold;
        flags[i] = keep ? 1 : 0;
    }
    int wc;
    wave_rank(keep, wc);
    if ((threadIdx.x & 63) == 0)
        wcount[threadIdx.x >> 6] = wc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int k = 0; k < SEG_BLOCK / 64; ++k)
            c += wcount[k];
        blk_count[blockIdx.x] = c;
    }
}

// ---- compaction of flagged points, order kept (block offsets from scan_kernel) ----------------------------------

// out position = block offset + rank among the block's flagged points; carries the segment and, optionally, the
// point's index within its segment (local = i - src_off[seg])
__global__ __launch_bounds__(SEG_BLOCK) void compact_scatter_kernel(const int *total, long long m, const uint8_t *flags,
                                                                    const int *blk_off, const float *xyz,
                                                                    const int *seg, const int *src_off, float *out_xyz,
                                                                    int *out_seg, int *out_local)
{
    __shared__ int wcount[SEG_BLOCK / 64];
    const long long i = (long long)blockIdx.x * SEG_BLOCK + threadIdx.x;
    const bool keep = i < min((long long)*total, m) && flags[i];
    int wc;
    const int r = wave_rank(keep, wc);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        wcount[wv] = wc;
    __syncthreads();
    if (!keep)
        return;
    int base = blk_off[blockIdx.x];
    for (int k = 0; k < wv; ++k)
        base += wcount[k];
    const long long q = base + r;
    out_xyz[3 * q] = xyz[3 * i];
    out_xyz[3 * q + 1] = xyz[3 * i + 1];
    out_xyz[3 * q + 2] = xyz[3 * i + 2];
    const int s = seg[i];
    if (out_seg)
        out_seg[q] = s;
    if (out_local)
        out_local[q] = (int)(i - src_off[s]);
}

// out_off[s] = the number of flagged points before src_off[s] (s = 0..S; src_off[S] is the total)
__global__ void compact_offsets_kernel(int s, const int *src_off, const uint8_t *flags, const int *blk_off,
                                       int *out_off)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > s)
        return;
    const int b = src_off[i];
    int c = blk_off[b / SEG_BLOCK];
    for (int k = b - b % SEG_BLOCK; k < b; ++k)
        c += flags[k];
    out_off[i] = c;
}

// ---- radius outlier removal --------------------------------------------------------------------------------------

// The comparison of the definition: d^2 < r^2 in double, r the float radius widened (open3d takes the radius as
// the float32 tf.py_func hands it; DESIGN.md, "Frame segments").
__device__ __forceinline__ double ro_radius_sq(float radius)
{
    const double r = (double)radius;
    return r * r;
}

struct RoGrid {                            // per segment, in the workspace
    double ox, oy, oz, inv_h;
    int gx, gy, gz, pad;
};

__device__ __forceinline__ int ro_axis(float v, double o, double inv_h, int g)
{
    const int c = (int)floor(((double)v - o) * inv_h);
    return min(max(c, 0), g - 1);
}

// one workgroup per segment: bounding box, grid of cells of edge h = max(r (1 + 2^-10), extent / 31), counting sort
// of the points into cell order (order within a cell is free: only counts are read)
__global__ __launch_bounds__(RO_THREADS) void ro_grid_kernel(const int *off, long long m, const float *xyz, float radius,
                                                             RoGrid *grids, int *cell_start, float4 *sorted)
{
    extern __shared__ int cells[];                           // RO_CELLS counts, then cursors
    __shared__ float red[6][RO_THREADS / 64];
    __shared__ RoGrid g;
    const int s = blockIdx.x, t = threadIdx.x;
    const int lo = off[s], n = (int)min((long long)off[s + 1], m) - lo;
    int *start = cell_start + (long long)s * (RO_CELLS + 1);
    if (n <= 0)
        return;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = t; k < n; k += RO_THREADS)
        for (int d = 0; d < 3; ++d) {
            const float v = xyz[3 * (long long)(lo + k) + d];
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
    for (int c = t; c < RO_CELLS; c += RO_THREADS)
        cells[c] = 0;
    __syncthreads();
    if (t == 0) {
        double lo3[3], ext = 0.0;
        for (int d = 0; d < 3; ++d) {
            float a = red[d][0], b = red[3 + d][0];
            for (int k = 1; k < RO_THREADS / 64; ++k) {
                a = fminf(a, red[d][k]);
                b = fmaxf(b, red[3 + d][k]);
            }
            lo3[d] = (double)a;
            ext = fmax(ext, (double)b - (double)a);
        }
        const double h = fmax((double)radius * (1.0 + 1.0 / 1024.0), ext / (RO_GRID_MAX - 1));
        g.ox = lo3[0];
        g.oy = lo3[1];
        g.oz = lo3[2];
        g.inv_h = 1.0 / h;
        g.gx = g.gy = g.gz = RO_GRID_MAX;
        grids[s] = g;
    }
    __syncthreads();
    const RoGrid G = g;
    for (int k = t; k < n; k += RO_THREADS) {
        const float *p = xyz + 3 * (long long)(lo + k);
        const int c = (ro_axis(p[2], G.oz, G.inv_h, G.gz) * G.gy + ro_axis(p[1], G.oy, G.inv_h, G.gy)) * G.gx +
                      ro_axis(p[0], G.ox, G.inv_h, G.gx);
        atomicAdd(&cells[c], 1);
    }
    __syncthreads();
    // exclusive scan of the counts: RO_CELLS / RO_THREADS per thread, then across threads (red[0] reused as ints)
    constexpr int PER = RO_CELLS / RO_THREADS;
    __shared__ int part[RO_THREADS];
    int sum = 0;
    for (int k = 0; k < PER; ++k)
        sum += cells[t * PER + k];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < RO_THREADS; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int k = 0; k < PER; ++k) {
        const int v = cells[t * PER + k];
        start[t * PER + k] = run;
        cells[t * PER + k] = run;              // cursor
        run += v;
    }
    if (t == RO_THREADS - 1)
        start[RO_CELLS] = run;
    __syncthreads();
    for (int k = t; k < n; k += RO_THREADS) {
        const float *p = xyz + 3 * (long long)(lo + k);
        const int c = (ro_axis(p[2], G.oz, G.inv_h, G.gz) * G.gy + ro_axis(p[1], G.oy, G.inv_h, G.gy)) * G.gx +
                      ro_axis(p[0], G.ox, G.inv_h, G.gx);
        const int q = atomicAdd(&cells[c], 1);
        sorted[lo + q] = make_float4(p[0], p[1], p[2], 0.0f);
    }
}

// per point: neighbours (itself included) with d^2 < r^2, counted cell by cell until the count passes nb_points
__global__ __launch_bounds__(SEG_BLOCK) void ro_count_kernel(
    const int *total, long long m, const int *off, const int *seg, const float *xyz, const RoGrid *grids, const int *cell_start,
    const float4 *sorted, int nb_points, float radius, uint8_t *flags, int *seg_count)
{
    const long long i = (long long)blockIdx.x * SEG_BLOCK + threadIdx.x;
    const bool live = i < min((long long)*total, m);
    bool keep = false;
    int s = -1;
    if (live) {
        s = seg[i];
        const RoGrid G = grids[s];
        const int lo = off[s];
        const int *start = cell_start + (long long)s * (RO_CELLS + 1);
        const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
        const double x = px, y = py, z = pz, r2 = ro_radius_sq(radius);
        const int cx = ro_axis(px, G.ox, G.inv_h, G.gx), cy = ro_axis(py, G.oy, G.inv_h, G.gy);
        const int cz = ro_axis(pz, G.oz, G.inv_h, G.gz);
        int count = 0;
        for (int zz = max(cz - 1, 0); zz <= min(cz + 1, G.gz - 1) && count <= nb_points; ++zz)
            for (int yy = max(cy - 1, 0); yy <= min(cy + 1, G.gy - 1) && count <= nb_points; ++yy) {
                const int row = (zz * G.gy + yy) * G.gx;
                const int a = start[row + max(cx - 1, 0)], b = start[row + min(cx + 1, G.gx - 1) + 1];
                for (int k = a; k < b && count <= nb_points; ++k) {
                    const float4 q = sorted[lo + k];
                    const double dx = x - (double)q.x, dy = y - (double)q.y, dz = z - (double)q.z;
                    count += ((dx * dx + dy * dy) + dz * dz) < r2;
                }
            }
        keep = count > nb_points;
        flags[i] = keep ? 1 : 0;
    }
    // one integer add per wave when the wave lies in one segment
    const int s0 = __shfl(s, 0);
    const bool uniform = __ballot(s != s0) == 0ull;
    int wc;
    wave_rank(keep, wc);
    if (uniform) {
        if ((threadIdx.x & 63) == 0 && s0 >= 0 && wc)
            atomicAdd(&seg_count[s0], wc);
    } else if (keep) {
        atomicAdd(&seg_count[s], 1);
    }
}

// fewer than min_keep inliers: keep the whole segment (:255-256); one count per block for the compaction
__global__ __launch_bounds__(SEG_BLOCK) void ro_inlier_flags_kernel(const int *total, long long m, const int *seg,
                                                                    const int *seg_count, int min_keep,
                                                                    uint8_t *flags, int *blk_count)
{
    __shared__ int wcount[SEG_BLOCK / 64];
    const long long i = (long long)blockIdx.x * SEG_BLOCK + threadIdx.x;
    bool keep = false;
    if (i < min((long long)*total, m)) {
        keep = flags[i] || seg_count[seg[i]] < min_keep;
        flags[i] = keep ? 1 : 0;
    }
    int wc;
    wave_rank(keep, wc);
    if ((threadIdx.x & 63) == 0)
        wcount[threadIdx.x >> 6] = wc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int k = 0; k < SEG_BLOCK / 64; ++k)
            c += wcount[k];
        blk_count[blockIdx.x] = c;
    }
}

// count_nonzero(inlier_idx): the inliers of a segment minus one when its point 0 is among them (:280)
__global__ void ro_num_valid_kernel(int s, const int *off, const int *in_off, const uint8_t *flags, int *num_valid)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s)
        return;
    const int n = in_off[i + 1] - in_off[i];
    num_valid[i] = n - ((off[i + 1] > off[i] && flags[off[i]]) ? 1 : 0);
}

// ---- ragged FPS --------------------------------------------------------------------------------------------------

__device__ __forceinline__ double fps_d2(double x0, double y0, double z0, float x, float y, float z)
{
    const double dx = x0 - (double)x, dy = y0 - (double)y, dz = z0 - (double)z;
    return (dx * dx + dy * dy) + dz * dz;
}

// (d, k) beats (bd, bk): the larger distance, then the lower index (numpy's first argmax)
__device__ __forceinline__ void fps_better(double d, int k, double &bd, int &bk)
{
    if (d > bd || (d == bd && k < bk)) {
        bd = d;
        bk = k;
    }
}

// one workgroup per set: idx[0] = start, idx[j] = first argmax of dist, dist = min(dist, d(idx[j]))
__global__ __launch_bounds__(FPS_THREADS) void fps_ragged_kernel(
    const int *off, long long m, const float *xyz, int k, const int *starts, double *dist_ws, int *idx, float *out_xyz)
{
    __shared__ double cand_d[2][FPS_WAVES];
    __shared__ int cand_k[2][FPS_WAVES];
    const int s = blockIdx.x, t = threadIdx.x;
    const int lo = off[s], n = (int)min((long long)off[s + 1], m) - lo;
    const int st = starts[s];
    int *I = idx + (long long)s * k;
    float *O = out_xyz + (long long)s * k * 3;
    const float *P = xyz + 3 * (long long)lo;
    if (n <= 0 || st < 0 || st >= n) {          // no set, or no valid start: -1 and zeros
        for (int j = t; j < k; j += FPS_THREADS) {
            I[j] = -1;
            O[3 * j] = O[3 * j + 1] = O[3 * j + 2] = 0.0f;
        }
        return;
    }
    double *D = dist_ws + lo;
    float px[FPS_PER_LANE], py[FPS_PER_LANE], pz[FPS_PER_LANE];
    double run[FPS_PER_LANE];
    double x0 = P[3 * st], y0 = P[3 * st + 1], z0 = P[3 * st + 2];
#pragma unroll
    for (int p = 0; p < FPS_PER_LANE; ++p) {
        const int q = t + FPS_THREADS * p;
        const bool ok = q < n;
        px[p] = ok ? P[3 * q] : 0.0f;
        py[p] = ok ? P[3 * q + 1] : 0.0f;
        pz[p] = ok ? P[3 * q + 2] : 0.0f;
        run[p] = ok ? fps_d2(x0, y0, z0, px[p], py[p], pz[p]) : -1.0;
    }
    for (int q = FPS_REG_POINTS + t; q < n; q += FPS_THREADS)
        D[q] = fps_d2(x0, y0, z0, P[3 * q], P[3 * q + 1], P[3 * q + 2]);
    if (t == 0) {
        I[0] = st;
        O[0] = P[3 * st];
        O[1] = P[3 * st + 1];
        O[2] = P[3 * st + 2];
    }
    int buf = 0;
    for (int j = 1; j < k; ++j) {
        // argmax over this lane's points in index order, then the wave, then the waves
        double bd = -2.0;
        int bk = 0x7fffffff;
#pragma unroll
        for (int p = 0; p < FPS_PER_LANE; ++p)
            if (run[p] > bd) {
                bd = run[p];
                bk = t + FPS_THREADS * p;
            }
        for (int q = FPS_REG_POINTS + t; q < n; q += FPS_THREADS) {
            const double d = D[q];
            if (d > bd) {
                bd = d;
                bk = q;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o);
            const int ok = __shfl_xor(bk, o);
            fps_better(od, ok, bd, bk);
        }
        if ((t & 63) == 0) {
            cand_d[buf][t >> 6] = bd;
            cand_k[buf][t >> 6] = bk;
        }
        __syncthreads();
        bd = cand_d[buf][0];
        bk = cand_k[buf][0];
        for (int w = 1; w < FPS_WAVES; ++w)
            fps_better(cand_d[buf][w], cand_k[buf][w], bd, bk);
        buf ^= 1;
        const float wx = P[3 * bk], wy = P[3 * bk + 1], wz = P[3 * bk + 2];
        if (t == 0) {
            I[j] = bk;
            O[3 * j] = wx;
            O[3 * j + 1] = wy;
            O[3 * j + 2] = wz;
        }
        if (j + 1 == k)
            break;
        x0 = wx;
        y0 = wy;
        z0 = wz;
#pragma unroll
        for (int p = 0; p < FPS_PER_LANE; ++p)
            if (t + FPS_THREADS * p < n)
                run[p] = fmin(run[p], fps_d2(x0, y0, z0, px[p], py[p], pz[p]));
        for (int q = FPS_REG_POINTS + t; q < n; q += FPS_THREADS)
            D[q] = fmin(D[q], fps_d2(x0, y0, z0, P[3 * q], P[3 * q + 1], P[3 * q + 2]));
    }
}

// ---- workspace layouts: one function each, for the query (null workspace) and the launcher ---------------------------

struct FsWorkspace {
    int nblk, gblk;                            // 256-pixel blocks of a frame, 256-point blocks of all frames
    int *table, *blk_count, *seg_blk_off, *seg_size, *mask_off, *mseg, *fblk_count, *fblk_off;
    float *mxyz;
    uint8_t *flags;
    size_t bytes;
};

FsWorkspace fs_workspace(int f, int h, int w, int s, void *workspace)
{
    const long long hw = (long long)h * w, m = (long long)f * hw;
    const long long nblk = (hw + SEG_BLOCK - 1) / SEG_BLOCK, gblk = (m + SEG_BLOCK - 1) / SEG_BLOCK;
    Carver ws(workspace);
    FsWorkspace L;
    L.nblk = (int)nblk, L.gblk = (int)gblk;
    L.table = ws.take<int>((size_t)f * SEG_CLASSES);
    L.blk_count = ws.take<int>((size_t)f * nblk * SEG_CLASSES);
    L.seg_blk_off = ws.take<int>((size_t)s * (nblk + 1));
    L.seg_size = ws.take<int>((size_t)s);
    L.mask_off = ws.take<int>((size_t)(s + 1));
    L.mxyz = ws.take<float>(3 * (size_t)m);
    L.mseg = ws.take<int>((size_t)m);
    L.flags = ws.take<uint8_t>((size_t)m);
    L.fblk_count = ws.take<int>((size_t)gblk);
    L.fblk_off = ws.take<int>((size_t)(gblk + 1));
    L.bytes = ws.bytes();
    return L;
}

struct RoWorkspace {
    int gblk;                                  // 256-point blocks
    RoGrid *grids;
    int *cell_start, *seg, *seg_count, *blk_count, *blk_off;
    float4 *sorted;
    uint8_t *flags;
    size_t bytes;
};

RoWorkspace ro_workspace(int s, long long m, void *workspace)
{
    const long long gblk = (m + SEG_BLOCK - 1) / SEG_BLOCK;
    Carver ws(workspace);
    RoWorkspace L;
    L.gblk = (int)gblk;
    L.grids = ws.take<RoGrid>((size_t)s);
    L.cell_start = ws.take<int>((size_t)s * (RO_CELLS + 1));
    L.sorted = ws.take<float4>((size_t)m);
    L.seg = ws.take<int>((size_t)m);
    L.flags = ws.take<uint8_t>((size_t)m);
    L.seg_count = ws.take<int>((size_t)s);
    L.blk_count = ws.take<int>((size_t)gblk);
    L.blk_off = ws.take<int>((size_t)(gblk + 1));
    L.bytes = ws.bytes();
    return L;
}

constexpr long long SEG_MAX_POINTS = 1ll << 28;    // F*H*W (and max_points): int offsets, 3*m float indices

}  // namespace

// segment index of each point of a packed array (seg_of[off[s] .. off[s+1]) = s): a per-segment fill
__global__ void seg_fill_kernel(const int *off, long long m, int *seg)
{
    const int s = blockIdx.y;
    const int lo = off[s], hi = (int)min((long long)off[s + 1], m);
    for (int i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += gridDim.x * blockDim.x)
        seg[i] = s;
}

CLOUDAAE_API long long cloudaae_frame_segments_workspace_bytes(int f, int h, int w, int s)
{
    if (f < 1 || h < 1 || w < 1 || s < 0 || (long long)f * h * w > SEG_MAX_POINTS)
        return -1;
    return (long long)fs_workspace(f, h, w, s, nullptr).bytes;
}

CLOUDAAE_API int cloudaae_frame_segments(int f, int h, int w, const uint16_t *depth, const uint8_t *label,
                                         const float *intrinsics, int s, const int *seg_frame, const int *seg_class,
                                         float threshold, int *offsets, float *xyz, float *mean, void *workspace,
                                         long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_frame_segments";
    CLOUDAAE_REQUIRE(f >= 1 && h >= 1 && w >= 1, name, "f, h and w must be >= 1");
    CLOUDAAE_REQUIRE((long long)f * h * w <= SEG_MAX_POINTS, name, "f*h*w above the limit of 2^28 pixels");
    CLOUDAAE_REQUIRE(s >= 1, name, "s must be >= 1");
    CLOUDAAE_REQUIRE(threshold == threshold, name, "threshold must not be NaN");
    CLOUDAAE_REQUIRE(depth && label && intrinsics && seg_frame && seg_class && offsets && xyz && mean && workspace,
                     name, "null pointer");
    const FsWorkspace L = fs_workspace(f, h, w, s, workspace);
    CLOUDAAE_REQUIRE(workspace_bytes >= (long long)L.bytes, name,
                     "workspace smaller than cloudaae_frame_segments_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    const int hw = h * w, nblk = L.nblk, gblk = L.gblk;
    const long long m = (long long)f * hw;

    CLOUDAAE_CHECK_HIP(hipMemsetAsync(L.table, 0xff, sizeof(int) * (size_t)f * SEG_CLASSES, st), name);
    hipLaunchKernelGGL(fs_table_kernel, dim3(ceil_div(s, 256)), dim3(256), 0, st, f, s, seg_frame, seg_class, L.table);
    hipLaunchKernelGGL(fs_count_kernel, dim3(nblk, f), dim3(SEG_BLOCK), 0, st, hw, nblk, depth, label, L.table,
                       L.blk_count);
    hipLaunchKernelGGL(fs_seg_scan_kernel, dim3(s), dim3(SEG_SCAN_THREADS), 0, st, f, nblk, seg_frame, seg_class,
                       L.table, L.blk_count, L.seg_blk_off, L.seg_size);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SEG_SCAN_THREADS), 0, st, L.seg_size, s, L.mask_off);
    hipLaunchKernelGGL(fs_scatter_kernel, dim3(nblk, f), dim3(SEG_BLOCK), 0, st, hw, w, nblk, depth, label,
                       intrinsics, L.table, L.seg_blk_off, L.mask_off, L.mxyz, L.mseg);
    hipLaunchKernelGGL(fs_mean_kernel, dim3(ceil_div(3ll * s, 64)), dim3(64), 0, st, s, L.mask_off, L.mxyz, mean);
    hipLaunchKernelGGL(fs_filter_flags_kernel, dim3(gblk), dim3(SEG_BLOCK), 0, st, L.mask_off + s, m, L.mxyz, L.mseg, mean,
                       threshold, L.flags, L.fblk_count);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SEG_SCAN_THREADS), 0, st, L.fblk_count, gblk, L.fblk_off);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(gblk), dim3(SEG_BLOCK), 0, st, L.mask_off + s, m, L.flags, L.fblk_off, L.mxyz,
                       L.mseg, L.mask_off, xyz, (int *)nullptr, (int *)nullptr);
    hipLaunchKernelGGL(compact_offsets_kernel, dim3(ceil_div(s + 1, 256)), dim3(256), 0, st, s, L.mask_off, L.flags,
                       L.fblk_off, offsets);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API long long cloudaae_radius_outlier_workspace_bytes(int s, long long max_points)
{
    if (s < 1 || max_points < 0 || max_points > SEG_MAX_POINTS)
        return -1;
    return (long long)ro_workspace(s, max_points, nullptr).bytes;
}

CLOUDAAE_API int cloudaae_radius_outlier(int s, const int *offsets, const float *xyz, long long max_points,
                                         int nb_points, float radius, int min_keep, int *in_offsets, int *in_index,
                                         float *in_xyz, int *num_valid, void *workspace, long long workspace_bytes,
                                         cloudaae_stream_t stream)
{
    const char *name = "cloudaae_radius_outlier";
    CLOUDAAE_REQUIRE(s >= 1, name, "s must be >= 1");
    CLOUDAAE_REQUIRE(max_points >= 1 && max_points <= SEG_MAX_POINTS, name, "max_points must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(nb_points >= 0 && min_keep >= 0, name, "nb_points and min_keep must be >= 0");
    CLOUDAAE_REQUIRE(radius > 0.0f && isfinite(radius), name, "radius must be a finite number > 0");
    CLOUDAAE_REQUIRE(offsets && xyz && in_offsets && in_index && in_xyz && num_valid && workspace, name,
                     "null pointer");
    const RoWorkspace L = ro_workspace(s, max_points, workspace);
    CLOUDAAE_REQUIRE(workspace_bytes >= (long long)L.bytes, name,
                     "workspace smaller than cloudaae_radius_outlier_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    const int gblk = L.gblk;
    constexpr size_t lds = sizeof(int) * RO_CELLS;      // (the same for every launch)
    CLOUDAAE_CHECK_HIP(allow_dynamic_lds<ro_grid_kernel>(lds, lds), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(L.seg_count, 0, sizeof(int) * (size_t)s, st), name);
    hipLaunchKernelGGL(seg_fill_kernel, dim3(64, s), dim3(256), 0, st, offsets, max_points, L.seg);
    hipLaunchKernelGGL(ro_grid_kernel, dim3(s), dim3(RO_THREADS), lds, st, offsets, max_points, xyz, radius, L.grids, L.cell_start,
                       L.sorted);
    hipLaunchKernelGGL(ro_count_kernel, dim3(gblk), dim3(SEG_BLOCK), 0, st, offsets + s, max_points, offsets, L.seg, xyz, L.grids,
                       L.cell_start, L.sorted, nb_points, radius, L.flags, L.seg_count);
    hipLaunchKernelGGL(ro_inlier_flags_kernel, dim3(gblk), dim3(SEG_BLOCK), 0, st, offsets + s, max_points, L.seg, L.seg_count,
                       min_keep, L.flags, L.blk_count);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SEG_SCAN_THREADS), 0, st, L.blk_count, gblk, L.blk_off);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(gblk), dim3(SEG_BLOCK), 0, st, offsets + s, max_points, L.flags, L.blk_off, xyz,
                       L.seg, offsets, in_xyz, (int *)nullptr, in_index);
    hipLaunchKernelGGL(compact_offsets_kernel, dim3(ceil_div(s + 1, 256)), dim3(256), 0, st, s, offsets, L.flags,
                       L.blk_off, in_offsets);
    hipLaunchKernelGGL(ro_num_valid_kernel, dim3(ceil_div(s, 256)), dim3(256), 0, st, s, offsets, in_offsets, L.flags,
                       num_valid);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API long long cloudaae_ragged_fps_workspace_bytes(long long max_points)
{
    if (max_points < 0 || max_points > SEG_MAX_POINTS)
        return -1;
    return (long long)workspace_pad(sizeof(double) * (size_t)max_points);
}

CLOUDAAE_API int cloudaae_ragged_fps(int s, const int *offsets, const float *xyz, long long max_points, int k,
                                     const int *starts, int *idx, float *out_xyz, void *workspace,
                                     long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_ragged_fps";
    CLOUDAAE_REQUIRE(s >= 1, name, "s must be >= 1");
    CLOUDAAE_REQUIRE(k >= 1, name, "k must be >= 1");
    CLOUDAAE_REQUIRE(max_points >= 1 && max_points <= SEG_MAX_POINTS, name, "max_points must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(offsets && xyz && starts && idx && out_xyz && workspace, name, "null pointer");
    CLOUDAAE_REQUIRE(workspace_bytes >= cloudaae_ragged_fps_workspace_bytes(max_points), name,
                     "workspace smaller than cloudaae_ragged_fps_workspace_bytes");
    hipLaunchKernelGGL(fps_ragged_kernel, dim3(s), dim3(FPS_THREADS), 0, (hipStream_t)stream, offsets, max_points, xyz, k, starts,
                       (double *)workspace, idx, out_xyz);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
