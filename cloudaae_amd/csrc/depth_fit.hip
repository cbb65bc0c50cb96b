// depth_fit.hip -- the per-pixel agreement of rendered hypotheses with the depth the camera saw, counted over a window of
// wh x ww pixels per sample: window pixel (x, y) is frame pixel (u0 + x, v0 + y), a pixel outside the frame has t = 0 and
// no segment.  DESIGN.md, "Pose verification" ("Counts") and "Detections" ("Windowed counts"), is the definition;
// tests/pose_verify_reference.py and tests/detect_reference.py restate it in NumPy.  The counts are integer arithmetic on
// the uint16 depths widened to int, so nothing depends on the order of execution, the batch or the run.
//
//   cloudaae_depth_fit_counts_window   three memsets and one launch.  A workgroup of 256 threads takes a run of 2048 window
//                               pixels of one sample, eight CONSECUTIVE ones per thread: the test depth, the label and
//                               seg are read once and kept in registers, then the sample's hypotheses [wh, ww] are
//                               streamed against them.  A lane reads its eight test depths with one 16-byte load (the
//                               label: one 8-byte load) only where they lie in one window row, inside the frame, and the
//                               address is aligned; every other lane goes pixel by pixel under predicates.  The choice
//                               is the lane's, per array, from the address: neither W nor ww need be a multiple of
//                               anything.  A predicate is counted by ballot + popcount per wave, the four waves meet in
//                               LDS once per eight hypotheses, and one integer atomic per workgroup, hypothesis and
//                               non-zero counter adds into the zeroed outputs.  The next hypothesis' depths are loaded
//                               while the current ones are compared.  A wave whose part of a hypothesis is all zero
//                               skips the comparisons.
//   cloudaae_depth_fit_counts   the same launch over whole frames.  A frame [h, w] is contiguous, so it is counted as ONE
//                               window row of h w pixels at the origin of a frame of one row: every lane inside lies "in
//                               one row" whatever w is, and only the lanes of a run's tail and the arrays whose base is
//                               not aligned go pixel by pixel.
#include "common.h"
#include "depth_frame.h"
#include "depth_fit.h"
#include "../../include/cloudaae_hip.h"

namespace cloudaae {

typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));


constexpr int DF_BLOCK = 256;
constexpr int DF_WAVES = DF_BLOCK / 64;
constexpr int DF_PIX = 8;                          // consecutive window pixels of a thread: 16 bytes of depth
constexpr int DF_TILE = DF_BLOCK * DF_PIX;         // window pixels of a workgroup
constexpr int DF_SLOTS = DF_COUNTERS + 2;          // + seg_total (hypothesis 0 only) + the sum of |d - t|
constexpr int DF_CHUNK = 8;                        // hypotheses between two meetings of the workgroup
static_assert(DF_CHUNK * DF_SLOTS <= DF_BLOCK, "one thread per (hypothesis of a chunk, slot)");

struct DepthFitArgs {
    int f, h, w, p, wh, ww, tiles;
    const unsigned short *depth_test, *depth_hyp;
    const unsigned char *label;
    const int *frame_of, *want, *tau, *origin;     // origin null: (0, 0) for every sample
    int *counts, *seg_total;
    long long *abs_sum;
};

// the eight depths packed in one 16-byte word
__device__ __forceinline__ void df_unpack8(uint4v q, int v[DF_PIX])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = (int)(q[i] & 0xffffu);
        v[2 * i + 1] = (int)(q[i] >> 16);
    }
}

// the lane's eight depths from window pixel q0 of a hypothesis image of n pixels (contiguous): one 16-byte load where the
// lane lies inside and its address is aligned, else pixel by pixel with zeros past the end
__device__ __forceinline__ void df_load8(const unsigned short *img, int n, int q0, int v[DF_PIX])
{
    if (q0 + DF_PIX <= n && ((uintptr_t)(img + q0) & 15u) == 0) {
        df_unpack8(*reinterpret_cast<const uint4v *>(img + q0), v);
    } else {
#pragma unroll
        for (int i = 0; i < DF_PIX; ++i)
            v[i] = q0 + i < n ? (int)img[q0 + i] : 0;
    }
}

__global__ __launch_bounds__(DF_BLOCK) void depth_fit_counts_kernel(DepthFitArgs a)
{
    __shared__ int red[DF_CHUNK][DF_WAVES][DF_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f)                       // (the whole workgroup: no barrier has been reached)
        return;
    const int n = a.wh * a.ww;                     // window pixels of a sample
    const int q0 = tile * DF_TILE + tid * DF_PIX;  // the lane's first window pixel (may lie past n)
    const int tau = a.tau[s];
    long long u0 = 0, v0 = 0;
    if (a.origin)                                  // (the whole workgroup)
        u0 = a.origin[2 * s], v0 = a.origin[2 * s + 1];

    // once per pixel: t and seg.  The lane's pixels start at column x0 of window row y0.
    const int y0 = q0 / a.ww, x0 = q0 - y0 * a.ww;
    const long long fu = u0 + x0, fv = v0 + y0;    // the frame pixel of the lane's first window pixel
    const bool one_row = q0 + DF_PIX <= n && x0 + DF_PIX <= a.ww && fv >= 0 && fv < a.h && fu >= 0 && fu + DF_PIX <= a.w;
    const size_t frame_base = (size_t)fr * a.h * a.w;
    int t[DF_PIX];
    unsigned seg = 0;
    const int want = a.label ? a.want[s] : 0;
    const size_t first = one_row ? frame_base + (size_t)fv * a.w + (size_t)fu : 0;
    if (one_row && ((uintptr_t)(a.depth_test + first) & 15u) == 0) {
        df_unpack8(*reinterpret_cast<const uint4v *>(a.depth_test + first), t);
    } else {
        int x = x0;
        long long v = fv;
#pragma unroll
        for (int i = 0; i < DF_PIX; ++i) {
            const long long u = u0 + x;
            const bool in = q0 + i < n && v >= 0 && v < a.h && u >= 0 && u < a.w;
            t[i] = in ? (int)a.depth_test[frame_base + (size_t)v * a.w + (size_t)u] : 0;
            if (++x == a.ww)
                x = 0, ++v;
        }
    }
    if (a.label) {
        if (one_row && ((uintptr_t)(a.label + first) & 7u) == 0) {
            const uint2v q = *reinterpret_cast<const uint2v *>(a.label + first);
#pragma unroll
            for (int i = 0; i < DF_PIX; ++i)
                seg |= (unsigned)((int)((q[i >> 2] >> (8 * (i & 3))) & 0xffu) == want && t[i] != 0) << i;
        } else {
            int x = x0;
            long long v = fv;
#pragma unroll
            for (int i = 0; i < DF_PIX; ++i) {
                const long long u = u0 + x;
                const bool in = q0 + i < n && v >= 0 && v < a.h && u >= 0 && u < a.w;
                const int l = in ? (int)a.label[frame_base + (size_t)v * a.w + (size_t)u] : -1;
                seg |= (unsigned)(l == want && t[i] != 0) << i;
                if (++x == a.ww)
                    x = 0, ++v;
            }
        }
    }
    int n_seg = 0;
#pragma unroll
    for (int i = 0; i < DF_PIX; ++i)
        n_seg += wave_count((seg >> i) & 1u);

    // the hypotheses, DF_CHUNK at a time: a wave leaves its counts of each in LDS, and the workgroup meets once per chunk.
    // The depths of the next hypothesis are on their way while the current ones are compared.
    const unsigned short *hyp0 = a.depth_hyp + (size_t)s * a.p * n;
    int d[DF_PIX], nx[DF_PIX];
    df_load8(hyp0, n, q0, nx);
    for (int j0 = 0; j0 < a.p; j0 += DF_CHUNK) {
        const int nj = a.p - j0 < DF_CHUNK ? a.p - j0 : DF_CHUNK;
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
#pragma unroll
            for (int i = 0; i < DF_PIX; ++i)
                d[i] = nx[i];
            if (j + 1 < a.p)
                df_load8(hyp0 + (size_t)(j + 1) * n, n, q0, nx);
            int cnt[DF_COUNTERS] = {0, 0, 0, 0, 0, 0};
            int asum = 0;
            const bool any = ((d[0] | d[1]) | (d[2] | d[3])) | ((d[4] | d[5]) | (d[6] | d[7]));
            if (__builtin_amdgcn_ballot_w64(any)) {    // (wave-uniform) a wave whose part is all zero counts nothing
#pragma unroll
                for (int i = 0; i < DF_PIX; ++i) {
                    const bool rend = d[i] != 0, both = rend && t[i] != 0;
                    const int diff = d[i] - t[i], mag = diff < 0 ? -diff : diff;
                    const bool cons = both && mag <= tau;
                    cnt[0] += wave_count(rend);
                    cnt[1] += wave_count(cons);
                    cnt[2] += wave_count(both && -diff > tau);
                    cnt[3] += wave_count(both && diff > tau);
                    cnt[4] += wave_count(rend && t[i] == 0);
                    cnt[5] += wave_count(cons && ((seg >> i) & 1u));
                    asum += cons ? mag : 0;
                }
            }
            // at most 512 * 65535: an int holds the wave's and the workgroup's sum
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                asum += __builtin_amdgcn_ds_bpermute((lane ^ o) << 2, asum);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < DF_COUNTERS; ++k)
                    red[jj][wv][k] = cnt[k];
                red[jj][wv][DF_COUNTERS] = j == 0 ? n_seg : 0;
                red[jj][wv][DF_COUNTERS + 1] = asum;
            }
        }
        __syncthreads();
        if (tid < nj * DF_SLOTS) {                 // one thread per (hypothesis of the chunk, slot)
            const int jj = tid / DF_SLOTS, slot = tid % DF_SLOTS;
            const size_t sp = (size_t)s * a.p + (j0 + jj);
            int sum = 0;
#pragma unroll
            for (int q = 0; q < DF_WAVES; ++q)
                sum += red[jj][q][slot];
            if (sum != 0) {
                if (slot < DF_COUNTERS)
                    __hip_atomic_fetch_add(a.counts + sp * DF_COUNTERS + slot, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else if (slot == DF_COUNTERS)
                    __hip_atomic_fetch_add(a.seg_total + s, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else
                    __hip_atomic_fetch_add(a.abs_sum + sp, (long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();                           // red is written again for the next chunk
    }
}

// Both entry points: `name` and `window` say which one refuses.  Without `window` the caller passes wh = h, ww = w and no
// origin, and the frame is flattened into one row here, after its products have been checked as 64-bit numbers.
static int depth_fit_counts(const char *name, bool window, int f, int h, int w, const uint16_t *depth_test, const uint8_t *label,
                            int b, int p, const int *frame_of, const int *want, const int *origin, int wh, int ww,
                            const uint16_t *depth_hyp, const int *tau, int *counts, int *seg_total, long long *abs_sum,
                            cloudaae_stream_t stream)
{
    CLOUDAAE_REQUIRE(f >= 1 && h >= 1 && w >= 1 && b >= 1 && p >= 1 && wh >= 1 && ww >= 1, name,
                     window ? "f, h, w, b, p, wh and ww must be >= 1" : "f, h, w, b and p must be >= 1");
    CLOUDAAE_REQUIRE((long long)h * w <= FRAME_MAX_PIXELS, name, "h * w above 2^24");
    CLOUDAAE_REQUIRE((long long)wh * ww <= FRAME_MAX_PIXELS, name, "wh * ww above 2^24");
    CLOUDAAE_REQUIRE((long long)b * p <= FRAME_MAX_TOTAL && (long long)b * p * ((long long)wh * ww) <= FRAME_MAX_TOTAL, name,
                     window ? "b * p * wh * ww above 2^28" : "b * p * h * w above 2^28");
    CLOUDAAE_REQUIRE(depth_test && frame_of && (origin || !window) && depth_hyp && tau && counts && seg_total && abs_sum, name,
                     "null pointer");
    CLOUDAAE_REQUIRE(want || !label, name, "a label image needs want");
    DepthFitArgs a;
    a.f = f, a.p = p;
    if (window)
        a.h = h, a.w = w, a.wh = wh, a.ww = ww;
    else
        a.h = a.wh = 1, a.w = a.ww = h * w;
    a.tiles = ceil_div((long long)wh * ww, DF_TILE);
    a.depth_test = depth_test, a.depth_hyp = depth_hyp, a.label = label;
    a.frame_of = frame_of, a.want = want, a.tau = tau, a.origin = origin;
    a.counts = counts, a.seg_total = seg_total, a.abs_sum = abs_sum;
    hipStream_t sm = (hipStream_t)stream;
    const size_t bp = (size_t)b * p;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * bp * DF_COUNTERS, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(seg_total, 0, sizeof(int) * (size_t)b, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(abs_sum, 0, sizeof(long long) * bp, sm), name);
    // b * tiles <= 2^28 / 2048 + b: below the grid limit
    hipLaunchKernelGGL(depth_fit_counts_kernel, dim3((unsigned)((long long)b * a.tiles)), dim3(DF_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_depth_fit_counts(int f, int h, int w, const uint16_t *depth_test, const uint8_t *label, int b, int p,
                                           const int *frame_of, const int *want, const uint16_t *depth_hyp, const int *tau,
                                           int *counts, int *seg_total, long long *abs_sum, cloudaae_stream_t stream)
{
    return depth_fit_counts("cloudaae_depth_fit_counts", false, f, h, w, depth_test, label, b, p, frame_of, want, nullptr, h, w,
                            depth_hyp, tau, counts, seg_total, abs_sum, stream);
}

CLOUDAAE_API int cloudaae_depth_fit_counts_window(int f, int h, int w, const uint16_t *depth_test, const uint8_t *label, int b,
                                                  int p, const int *frame_of, const int *want, const int *origin, int wh, int ww,
                                                  const uint16_t *depth_hyp, const int *tau, int *counts, int *seg_total,
                                                  long long *abs_sum, cloudaae_stream_t stream)
{
    return depth_fit_counts("cloudaae_depth_fit_counts_window", true, f, h, w, depth_test, label, b, p, frame_of, want, origin,
                            wh, ww, depth_hyp, tau, counts, seg_total, abs_sum, stream);
}
