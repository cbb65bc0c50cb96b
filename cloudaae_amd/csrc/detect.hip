// detect.hip -- the device side of detection: which found depth component is which object, under which pose, or nothing.
// DESIGN.md, "Detections", is the definition; tests/detect_reference.py restates it in NumPy.  All arithmetic is integer
// (the float64 scores are single divisions of two integers), so nothing depends on the order of execution, the batch or
// the run.
//
//   cloudaae_depth_fit_counts_window   cloudaae_depth_fit_counts (pose_verify.hip) over a window of wh x ww pixels per
//                               sample: window pixel (x, y) is frame pixel (u0 + x, v0 + y), a pixel outside the frame
//                               has t = 0 and no segment.  The same shape as that kernel: a workgroup of 256 threads
//                               takes a run of 2048 window pixels of one sample, eight consecutive ones per thread; t
//                               and seg are read once and held in registers, the sample's hypotheses [wh, ww] are
//                               streamed against them with the next one in flight, a predicate is counted by ballot +
//                               popcount per wave, the waves meet in LDS once per eight hypotheses and one integer
//                               atomic per workgroup, hypothesis and non-zero counter adds into the zeroed outputs.
//                               A lane reads its eight test depths with one 16-byte load (the label: one 8-byte load)
//                               only where they lie in one window row, inside the frame, and the address is aligned;
//                               every other lane goes pixel by pixel under predicates.  The choice is the lane's, per
//                               array, from the address: neither W nor ww need be a multiple of anything.
//   cloudaae_detect_assign      one launch, one workgroup per frame: the best hypothesis of every (component, class)
//                               pair by cloudaae_select_pose's fraction and comparison, then at most n_components rounds
//                               of greedy assignment, each one exact argmax over the eligible pairs (a thread's own
//                               pairs, a wave by shuffles, the four waves through LDS).  No workgroup waits for another.
#include "common.h"
#include "../../include/cloudaae_hip.h"

namespace cloudaae {

typedef unsigned int dt_uint4v __attribute__((ext_vector_type(4)));
typedef unsigned int dt_uint2v __attribute__((ext_vector_type(2)));

constexpr long long DW_MAX_PIXELS = 1ll << 24;     // wh ww, h w
constexpr long long DW_MAX_TOTAL = 1ll << 28;      // b p wh ww, f k c p

// ---- cloudaae_depth_fit_counts_window --------------------------------------------------------------------------------
constexpr int DW_BLOCK = 256;
constexpr int DW_WAVES = DW_BLOCK / 64;
constexpr int DW_PIX = 8;                          // consecutive window pixels of a thread: 16 bytes of depth
constexpr int DW_TILE = DW_BLOCK * DW_PIX;         // window pixels of a workgroup
constexpr int DW_COUNTERS = 6;                     // rendered, consistent, in_front, behind, unknown, explained
constexpr int DW_SLOTS = DW_COUNTERS + 2;          // + seg_total (hypothesis 0 only) + the sum of |d - t|
constexpr int DW_CHUNK = 8;                        // hypotheses between two meetings of the workgroup
static_assert(DW_CHUNK * DW_SLOTS <= DW_BLOCK, "one thread per (hypothesis of a chunk, slot)");

struct WindowFitArgs {
    int f, h, w, b, p, wh, ww, tiles;
    const unsigned short *depth_test, *depth_hyp;
    const unsigned char *label;
    const int *frame_of, *want, *tau, *origin;
    int *counts, *seg_total;
    long long *abs_sum;
};

// the lane's eight depths from window pixel q0 of a hypothesis image of n pixels (contiguous): one 16-byte load where the
// lane lies inside and its address is aligned, else pixel by pixel with zeros past the end
__device__ __forceinline__ void dw_load_hyp(const unsigned short *img, int n, int q0, int v[DW_PIX])
{
    if (q0 + DW_PIX <= n && ((uintptr_t)(img + q0) & 15u) == 0) {
        const dt_uint4v q = *reinterpret_cast<const dt_uint4v *>(img + q0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = (int)(q[i] & 0xffffu);
            v[2 * i + 1] = (int)(q[i] >> 16);
        }
    } else {
#pragma unroll
        for (int i = 0; i < DW_PIX; ++i)
            v[i] = q0 + i < n ? (int)img[q0 + i] : 0;
    }
}

__global__ __launch_bounds__(DW_BLOCK) void depth_fit_counts_window_kernel(WindowFitArgs a)
{
    __shared__ int red[DW_CHUNK][DW_WAVES][DW_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const int fr = a.frame_of[s];
    if (fr < 0 || fr >= a.f)                       // (the whole workgroup: no barrier has been reached)
        return;
    const int n = a.wh * a.ww;                     // window pixels of a sample
    const int q0 = tile * DW_TILE + tid * DW_PIX;  // the lane's first window pixel (may lie past n)
    const int tau = a.tau[s];
    const long long u0 = a.origin[2 * s], v0 = a.origin[2 * s + 1];

    // once per pixel: t and seg.  The lane's pixels start at column x0 of window row y0.
    const int y0 = q0 / a.ww, x0 = q0 - y0 * a.ww;
    const long long fu = u0 + x0, fv = v0 + y0;    // the frame pixel of the lane's first window pixel
    const bool one_row = q0 + DW_PIX <= n && x0 + DW_PIX <= a.ww && fv >= 0 && fv < a.h && fu >= 0 && fu + DW_PIX <= a.w;
    const size_t frame_base = (size_t)fr * a.h * a.w;
    int t[DW_PIX];
    unsigned seg = 0;
    const int want = a.label ? a.want[s] : 0;
    const size_t first = one_row ? frame_base + (size_t)fv * a.w + (size_t)fu : 0;
    if (one_row && ((uintptr_t)(a.depth_test + first) & 15u) == 0) {
        const dt_uint4v q = *reinterpret_cast<const dt_uint4v *>(a.depth_test + first);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            t[2 * i] = (int)(q[i] & 0xffffu);
            t[2 * i + 1] = (int)(q[i] >> 16);
        }
    } else {
        int x = x0;
        long long v = fv;
#pragma unroll
        for (int i = 0; i < DW_PIX; ++i) {
            const long long u = u0 + x;
            const bool in = q0 + i < n && v >= 0 && v < a.h && u >= 0 && u < a.w;
            t[i] = in ? (int)a.depth_test[frame_base + (size_t)v * a.w + (size_t)u] : 0;
            if (++x == a.ww)
                x = 0, ++v;
        }
    }
    if (a.label) {
        if (one_row && ((uintptr_t)(a.label + first) & 7u) == 0) {
            const dt_uint2v q = *reinterpret_cast<const dt_uint2v *>(a.label + first);
#pragma unroll
            for (int i = 0; i < DW_PIX; ++i)
                seg |= (unsigned)((int)((q[i >> 2] >> (8 * (i & 3))) & 0xffu) == want && t[i] != 0) << i;
        } else {
            int x = x0;
            long long v = fv;
#pragma unroll
            for (int i = 0; i < DW_PIX; ++i) {
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
    for (int i = 0; i < DW_PIX; ++i)
        n_seg += wave_count((seg >> i) & 1u);

    // the hypotheses, DW_CHUNK at a time: a wave leaves its counts of each in LDS, and the workgroup meets once per chunk.
    // The depths of the next hypothesis are on their way while the current ones are compared.
    const unsigned short *hyp0 = a.depth_hyp + (size_t)s * a.p * n;
    int d[DW_PIX], nx[DW_PIX];
    dw_load_hyp(hyp0, n, q0, nx);
    for (int j0 = 0; j0 < a.p; j0 += DW_CHUNK) {
        const int nj = a.p - j0 < DW_CHUNK ? a.p - j0 : DW_CHUNK;
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
#pragma unroll
            for (int i = 0; i < DW_PIX; ++i)
                d[i] = nx[i];
            if (j + 1 < a.p)
                dw_load_hyp(hyp0 + (size_t)(j + 1) * n, n, q0, nx);
            int cnt[DW_COUNTERS] = {0, 0, 0, 0, 0, 0};
            int asum = 0;
            const bool any = ((d[0] | d[1]) | (d[2] | d[3])) | ((d[4] | d[5]) | (d[6] | d[7]));
            if (__builtin_amdgcn_ballot_w64(any)) {    // (wave-uniform) a wave whose part is all zero counts nothing
#pragma unroll
                for (int i = 0; i < DW_PIX; ++i) {
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
                for (int k = 0; k < DW_COUNTERS; ++k)
                    red[jj][wv][k] = cnt[k];
                red[jj][wv][DW_COUNTERS] = j == 0 ? n_seg : 0;
                red[jj][wv][DW_COUNTERS + 1] = asum;
            }
        }
        __syncthreads();
        if (tid < nj * DW_SLOTS) {                 // one thread per (hypothesis of the chunk, slot)
            const int jj = tid / DW_SLOTS, slot = tid % DW_SLOTS;
            const size_t sp = (size_t)s * a.p + (j0 + jj);
            int sum = 0;
#pragma unroll
            for (int q = 0; q < DW_WAVES; ++q)
                sum += red[jj][q][slot];
            if (sum != 0) {
                if (slot < DW_COUNTERS)
                    __hip_atomic_fetch_add(a.counts + sp * DW_COUNTERS + slot, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else if (slot == DW_COUNTERS)
                    __hip_atomic_fetch_add(a.seg_total + s, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else
                    __hip_atomic_fetch_add(a.abs_sum + sp, (long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();                           // red is written again for the next chunk
    }
}

// ---- cloudaae_detect_assign ------------------------------------------------------------------------------------------
constexpr int DA_BLOCK = 256;
constexpr int DA_WAVES = DA_BLOCK / 64;
constexpr int DA_MAX_K = 254, DA_MAX_C = 256, DA_MAX_P = 64;

struct AssignArgs {
    int f, k, c, p, mode, min_num, min_den, max_per_class;
    const int *counts, *seg_total, *valid, *n_components;
    const double *pose;
    int *pair_hyp, *pair_num, *pair_den;           // (written, then read back by the same launch: not __restrict__)
    double *pair_score;
    int *det_class, *det_hyp, *det_num, *det_den, *det_rank, *alt_class, *alt_num, *alt_den, *n_det;
    double *det_score, *det_pose;
};

// num and den of one hypothesis (0 / 1 for "no score"): cloudaae_select_pose's two rules
__device__ __forceinline__ void da_fraction(const int *c, int seg_total, bool usable, int mode, long long &num, long long &den)
{
    if (mode == 0) {
        num = c[5];
        den = (long long)seg_total + c[2];
    } else {
        num = c[1];
        den = ((long long)c[1] + c[2]) + c[3];
    }
    if (den <= 0 || num < 0 || !usable) {
        num = 0;
        den = 1;
    }
}

// a candidate of the argmax: a fraction and the pair's index (-1: none).  x beats y when it is there and y is not, its
// fraction is strictly larger, or the fractions are equal and its index is lower.
__device__ __forceinline__ bool da_beats(int xn, int xd, int xi, int yn, int yd, int yi)
{
    if (xi < 0 || yi < 0)
        return xi >= 0 && yi < 0;
    const long long l = (long long)xn * yd, r = (long long)yn * xd;
    return l > r || (l == r && xi < yi);
}

__global__ __launch_bounds__(DA_BLOCK) void detect_assign_kernel(AssignArgs a)
{
    __shared__ int sm_class[DA_MAX_K + 2], sm_rank[DA_MAX_K + 2], sm_used[DA_MAX_C];
    __shared__ int sm_best[DA_WAVES][3];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = blockIdx.x;
    const int kc = a.k * a.c;
    int nc = a.n_components[fr];
    nc = nc < 0 ? 0 : (nc > a.k ? a.k : nc);
    const size_t base = (size_t)fr * kc;

    // step 1: the best hypothesis of every pair
    for (int e = tid; e < kc; e += DA_BLOCK) {
        const int k = e / a.c;
        const size_t row = (base + e) * a.p;
        const int st = a.seg_total[base + e];
        int win = 0;
        long long wn = 0, wd = 1;
        for (int j = 0; j < a.p; ++j) {
            long long num, den;
            da_fraction(a.counts + (row + j) * DW_COUNTERS, st, k < nc && a.valid[row + j] != 0, a.mode, num, den);
            if (j == 0 || num * wd > wn * den)     // strictly larger: ties stay with the lower index
                win = j, wn = num, wd = den;
        }
        a.pair_hyp[base + e] = win;
        a.pair_num[base + e] = (int)wn;
        a.pair_den[base + e] = (int)wd;
        a.pair_score[base + e] = (double)wn / (double)wd;
    }
    for (int k = tid; k < DA_MAX_K + 2; k += DA_BLOCK)
        sm_class[k] = -1, sm_rank[k] = -1;
    for (int c = tid; c < DA_MAX_C; c += DA_BLOCK)
        sm_used[c] = 0;
    __syncthreads();                               // the pair tables are read by other threads from here on

    // step 2: greedy assignment.  Every thread sees the same winner, so the loop is uniform.
    int rounds = 0;
    for (; rounds < nc; ++rounds) {
        int bn = 0, bd = 1, bi = -1;
        for (int e = tid; e < nc * a.c; e += DA_BLOCK) {
            const int k = e / a.c, c = e - k * a.c;
            const int num = a.pair_num[base + e], den = a.pair_den[base + e];
            const bool eligible = sm_class[k] < 0 && sm_used[c] < a.max_per_class && num > 0 &&
                                  (long long)num * a.min_den >= (long long)a.min_num * den;
            if (eligible && da_beats(num, den, e, bn, bd, bi))
                bn = num, bd = den, bi = e;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int on = __shfl_xor(bn, o, 64), od = __shfl_xor(bd, o, 64), oi = __shfl_xor(bi, o, 64);
            if (da_beats(on, od, oi, bn, bd, bi))
                bn = on, bd = od, bi = oi;
        }
        if (lane == 0)
            sm_best[wv][0] = bn, sm_best[wv][1] = bd, sm_best[wv][2] = bi;
        __syncthreads();
        bn = sm_best[0][0], bd = sm_best[0][1], bi = sm_best[0][2];
#pragma unroll
        for (int q = 1; q < DA_WAVES; ++q)
            if (da_beats(sm_best[q][0], sm_best[q][1], sm_best[q][2], bn, bd, bi))
                bn = sm_best[q][0], bd = sm_best[q][1], bi = sm_best[q][2];
        __syncthreads();                           // sm_best is written again in the next round
        if (bi < 0)
            break;
        if (tid == 0) {
            const int k = bi / a.c, c = bi - k * a.c;
            sm_class[k] = c;
            sm_rank[k] = rounds;
            sm_used[c] += 1;
        }
        __syncthreads();
    }
    if (tid == 0)
        a.n_det[fr] = rounds;

    // the table, one thread per component
    for (int k = tid; k < a.k; k += DA_BLOCK) {
        const size_t o = (size_t)fr * a.k + k;
        const int c = sm_class[k];
        int hyp = -1, num = 0, den = 1;
        if (c >= 0) {
            const size_t e = base + (size_t)k * a.c + c;
            hyp = a.pair_hyp[e], num = a.pair_num[e], den = a.pair_den[e];
            const double *src = a.pose + 16 * (e * a.p + hyp);
            for (int i = 0; i < 16; ++i)
                a.det_pose[16 * o + i] = src[i];
        } else {
            for (int i = 0; i < 16; ++i)
                a.det_pose[16 * o + i] = 0.0;
        }
        a.det_class[o] = c;
        a.det_hyp[o] = hyp;
        a.det_num[o] = num;
        a.det_den[o] = den;
        a.det_score[o] = (double)num / (double)den;
        a.det_rank[o] = sm_rank[k];
        int an = 0, ad = 1, ac = -1;               // the best pair with another class, availability ignored
        for (int c2 = 0; c2 < a.c; ++c2) {
            if (c2 == c)
                continue;
            const size_t e = base + (size_t)k * a.c + c2;
            if (da_beats(a.pair_num[e], a.pair_den[e], c2, an, ad, ac))
                an = a.pair_num[e], ad = a.pair_den[e], ac = c2;
        }
        a.alt_class[o] = ac;
        a.alt_num[o] = an;
        a.alt_den[o] = ad;
    }
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_depth_fit_counts_window(int f, int h, int w, const uint16_t *depth_test, const uint8_t *label, int b,
                                                  int p, const int *frame_of, const int *want, const int *origin, int wh, int ww,
                                                  const uint16_t *depth_hyp, const int *tau, int *counts, int *seg_total,
                                                  long long *abs_sum, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_fit_counts_window";
    CLOUDAAE_REQUIRE(f >= 1 && h >= 1 && w >= 1 && b >= 1 && p >= 1 && wh >= 1 && ww >= 1, name,
                     "f, h, w, b, p, wh and ww must be >= 1");
    CLOUDAAE_REQUIRE((long long)h * w <= DW_MAX_PIXELS, name, "h * w above 2^24");
    CLOUDAAE_REQUIRE((long long)wh * ww <= DW_MAX_PIXELS, name, "wh * ww above 2^24");
    CLOUDAAE_REQUIRE((long long)b * p <= DW_MAX_TOTAL && (long long)b * p * ((long long)wh * ww) <= DW_MAX_TOTAL, name,
                     "b * p * wh * ww above 2^28");
    CLOUDAAE_REQUIRE(depth_test && frame_of && origin && depth_hyp && tau && counts && seg_total && abs_sum, name, "null pointer");
    CLOUDAAE_REQUIRE(want || !label, name, "a label image needs want");
    WindowFitArgs a;
    a.f = f, a.h = h, a.w = w, a.b = b, a.p = p, a.wh = wh, a.ww = ww;
    a.tiles = ceil_div((long long)wh * ww, DW_TILE);
    a.depth_test = depth_test, a.depth_hyp = depth_hyp, a.label = label;
    a.frame_of = frame_of, a.want = want, a.tau = tau, a.origin = origin;
    a.counts = counts, a.seg_total = seg_total, a.abs_sum = abs_sum;
    hipStream_t sm = (hipStream_t)stream;
    const size_t bp = (size_t)b * p;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * bp * DW_COUNTERS, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(seg_total, 0, sizeof(int) * (size_t)b, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(abs_sum, 0, sizeof(long long) * bp, sm), name);
    // b * tiles <= 2^28 / 2048 + b: below the grid limit
    hipLaunchKernelGGL(depth_fit_counts_window_kernel, dim3((unsigned)((long long)b * a.tiles)), dim3(DW_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_detect_assign(int f, int k, int c, int p, const int *counts, const int *seg_total, const int *valid,
                                        const double *pose, const int *n_components, int mode, int min_num, int min_den,
                                        int max_per_class, int *pair_hyp, int *pair_num, int *pair_den, double *pair_score,
                                        int *det_class, int *det_hyp, int *det_num, int *det_den, double *det_score,
                                        int *det_rank, double *det_pose, int *alt_class, int *alt_num, int *alt_den, int *n_det,
                                        cloudaae_stream_t stream)
{
    const char *name = "cloudaae_detect_assign";
    CLOUDAAE_REQUIRE(f >= 1 && k >= 1 && c >= 1 && p >= 1, name, "f, k, c and p must be >= 1");
    CLOUDAAE_REQUIRE(k <= DA_MAX_K && c <= DA_MAX_C && p <= DA_MAX_P, name, "k above 254, c above 256 or p above 64");
    CLOUDAAE_REQUIRE((long long)f * k * c * p <= DW_MAX_TOTAL, name, "f * k * c * p above 2^28");
    CLOUDAAE_REQUIRE(mode == 0 || mode == 1, name, "mode must be 0 (segment rule) or 1 (silhouette rule)");
    CLOUDAAE_REQUIRE(min_den >= 1 && min_den <= (1 << 20) && min_num >= 0 && min_num <= min_den, name,
                     "the threshold needs 0 <= min_num <= min_den and 1 <= min_den <= 2^20");
    CLOUDAAE_REQUIRE(max_per_class >= 1, name, "max_per_class must be >= 1");
    CLOUDAAE_REQUIRE(counts && seg_total && valid && pose && n_components && pair_hyp && pair_num && pair_den && pair_score &&
                         det_class && det_hyp && det_num && det_den && det_score && det_rank && det_pose && alt_class &&
                         alt_num && alt_den && n_det,
                     name, "null pointer");
    AssignArgs a;
    a.f = f, a.k = k, a.c = c, a.p = p, a.mode = mode, a.min_num = min_num, a.min_den = min_den, a.max_per_class = max_per_class;
    a.counts = counts, a.seg_total = seg_total, a.valid = valid, a.n_components = n_components, a.pose = pose;
    a.pair_hyp = pair_hyp, a.pair_num = pair_num, a.pair_den = pair_den, a.pair_score = pair_score;
    a.det_class = det_class, a.det_hyp = det_hyp, a.det_num = det_num, a.det_den = det_den, a.det_rank = det_rank;
    a.alt_class = alt_class, a.alt_num = alt_num, a.alt_den = alt_den, a.n_det = n_det;
    a.det_score = det_score, a.det_pose = det_pose;
    hipLaunchKernelGGL(detect_assign_kernel, dim3((unsigned)f), dim3(DA_BLOCK), 0, (hipStream_t)stream, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
