// detect.hip -- the device side of detection: which found depth component is which object, under which pose, or nothing,
// from the windowed counts of depth_fit.hip.  DESIGN.md, "Detections", is the definition; tests/detect_reference.py restates
// it in NumPy.  All arithmetic is integer (the float64 scores are single divisions of two integers), so nothing depends on
// the order of execution, the batch or the run.
//
//   cloudaae_detect_assign      one launch, one workgroup per frame: the best hypothesis of every (component, class)
//                               pair by cloudaae_select_pose's fraction (df_fraction of depth_fit.h) and comparison, then
//                               at most n_components rounds of greedy assignment, each one exact argmax over the eligible
//                               pairs (a thread's own pairs, a wave by shuffles, the four waves through LDS).  No
//                               workgroup waits for another.
#include "common.h"
#include "depth_fit.h"
#include "../../include/cloudaae_hip.h"

namespace cloudaae {

// ---- cloudaae_detect_assign ------------------------------------------------------------------------------------------
constexpr int DA_BLOCK = 256;
constexpr int DA_WAVES = DA_BLOCK / 64;
constexpr int DA_MAX_K = 254, DA_MAX_C = 256, DA_MAX_P = 64;
constexpr long long DA_MAX_TOTAL = 1ll << 28;      // f k c p

struct AssignArgs {
    int f, k, c, p, mode, min_num, min_den, max_per_class;
    const int *counts, *seg_total, *valid, *n_components;
    const double *pose;
    int *pair_hyp, *pair_num, *pair_den;           // (written, then read back by the same launch: not __restrict__)
    double *pair_score;
    int *det_class, *det_hyp, *det_num, *det_den, *det_rank, *alt_class, *alt_num, *alt_den, *n_det;
    double *det_score, *det_pose;
};

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
            df_fraction(a.counts + (row + j) * DF_COUNTERS, st, k < nc && a.valid[row + j] != 0, a.mode, num, den);
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
    CLOUDAAE_REQUIRE((long long)f * k * c * p <= DA_MAX_TOTAL, name, "f * k * c * p above 2^28");
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
