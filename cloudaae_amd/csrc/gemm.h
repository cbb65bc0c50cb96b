// gemm.h -- internal (not part of the C ABI): the GEMM launchers with folded-operand addressing,
// shared by gemm.hip / gemm_bf16.hip / gemm_b16.hip and edgeconv.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"

namespace cloudaae {

enum { EPI_STORE = 0, EPI_ACCUM = 1, EPI_ATOMIC = 2 };

// A row-major matrix whose logical columns are FOLDED into stacked row blocks: logical (r, c) lives
// at physical row (c >> shift) * rows + r, column c & (width - 1).  That is how the edge convolution's
// [2*cin, cout] kernel looks when it is used as [cin, 2*cout] = [W_centre | W_neighbour]: with it the
// P/Q products, their dX and their dW are ONE product each instead of two (edgeconv.hip).
// shift < 0: no folding.
struct Fold {
    int shift, rows;
};
__device__ __forceinline__ size_t fold_off(int r, int c, int ld, Fold f)
{
    if (f.shift < 0)
        return (size_t)r * ld + c;
    return (size_t)((c >> f.shift) * f.rows + r) * ld + (c & ((1 << f.shift) - 1));
}

// C[M,N] (+)= op(A) op(B) like cloudaae_gemm_f32 / cloudaae_gemm_bf16, plus:
// fold_b / fold_c = 0, or the power-of-two width at which the logical columns of B / C fold into stacked row
// blocks (see Fold); the folded matrix has leading dimension == width.
// colstats (optional): per row tile the column sums and sums of squares of C.
// ordered_ws (optional): room for splits * M * N floats; a product cut over K then keeps its slices apart and sums
// them in slice order (bit-reproducible) instead of adding them with atomics.
int gemm_f32_launch(const char *name, int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                    const float *B, int ldb, float *C, int ldc, const float *bias, int accumulate, int fold_b,
                    int fold_c, hipStream_t stream, double *colstats = nullptr, float *ordered_ws = nullptr);
int gemm_bf16_launch(const char *name, int trans_a, int trans_b, int M, int N, int K, const float *A, int lda,
                     const float *B, int ldb, float *C, int ldc, const float *bias, int accumulate, int fold_b,
                     int fold_c, hipStream_t stream, double *colstats = nullptr, float *ordered_ws = nullptr);
// C = (ws[0] + ws[1] + ...) + bias, the slices of a product cut over K summed in slice order into the (folded) output
int gemm_slices_sum(const char *name, int M, int N, int splits, const float *ws, float *C, int ldc, const float *bias,
                    hipStream_t stream, Fold fold);

// gemm_x3.hip: dx[M,N] = dy[M,K] P^T as cloudaae_gemm_bf16x3p, with dy formed from y[M,K] on its way into the matrix cores
// (bn_common.h: bn_bwd_dy_hoisted on the table `consts` of bn_dyc_floats(K, M / rows) floats) and stored to dy by the
// workgroups of the first column tile.  Served: a streamed product with 160-column tiles whose 128-row tiles lie inside one
// group of `rows` rows.
bool gemm_x3s_bnbwd_served(int M, int N, int K, int rows);
int gemm_x3s_bnbwd_launch(const char *name, int M, int N, int K, const float *y, int ldy, const void *planes, float *dx, int lddx,
                          const float *consts, int rows, int relu, float *dy, int lddy, hipStream_t stream);

// K slices for a product that asks for `want`: at most max_splits (K over the fewest k a slice may get), at least one,
// and above 8 a multiple of 8 -- whole slices per XCD (the kernels then keep a slice's tiles on one XCD)
inline int whole_xcd_splits(int want, int max_splits)
{
    int splits = want < max_splits ? want : max_splits;
    if (splits < 1)
        splits = 1;
    if (splits > 8)
        splits = splits / 8 * 8;
    return splits;
}

// Clears the fp32 output C[M, N] before K slices add into it with atomics; a folded output is one contiguous
// [N/width * M][width] block.
inline hipError_t gemm_zero_output(float *C, int M, int N, int ldc, bool folded, hipStream_t s)
{
    if (folded)
        return hipMemsetAsync(C, 0, sizeof(float) * (size_t)M * (size_t)N, s);
    return hipMemset2DAsync(C, sizeof(float) * (size_t)ldc, 0, sizeof(float) * (size_t)N, (size_t)M, s);
}

// ---- the host half of the fp32 (gemm.hip) and bf16-operand (gemm_bf16.hip) families ----------------------------------
// A Family supplies what differs between them:
//   BK                                  k per slab
//   plan(M, N, K, BM, BN, splits, ordered)  tile shape and K slices
//   fast(BM, BN, tb, args)              whether the predicate-free kernel serves this launch
//   kernel<BM, BN, WM, WN, TA, TB, FAST>(grid, stream, args)   launches one kernel
//   tiles(BM, BN, ta, tb, grid, stream, args)                   the tile shapes it is compiled for
//   ws_missing                          the refusal of an ordered product whose workspace does not cover the cut

// The cut of a product: tile shape, k per slice (whole slabs) and the slices that gives.  The launcher and every query
// derive it here, so a workspace sized by a query covers the launch that uses it.
struct GemmCut {
    int BM, BN, kchunk, splits;
};
template <class Family>
GemmCut gemm_cut(int M, int N, int K, bool ordered)
{
    GemmCut c;
    Family::plan(M, N, K, c.BM, c.BN, c.splits, ordered);
    c.kchunk = K > 0 ? ceil_div(ceil_div(K, c.splits), Family::BK) * Family::BK : Family::BK;
    c.splits = K > 0 ? ceil_div(K, c.kchunk) : 1;
    return c;
}

// the parameters of both families' kernels, in order
struct GemmArgs {
    int M, N, K;
    const float *A; int lda;
    const float *B; int ldb;
    float *C; int ldc;
    const float *bias;
    int epi, kchunk, vecA, vecB;
    Fold fb, fc;
    double *colstats;
    long long cslice;
};

template <class Family, int BM, int BN, int WM, int WN, bool FAST>
void gemm_launch_as(bool ta, bool tb, dim3 grid, hipStream_t s, const GemmArgs &g)
{
    if (!ta && !tb)
        Family::template kernel<BM, BN, WM, WN, false, false, FAST>(grid, s, g);
    else if (!ta && tb)
        Family::template kernel<BM, BN, WM, WN, false, true, FAST>(grid, s, g);
    else if (ta && !tb)
        Family::template kernel<BM, BN, WM, WN, true, false, FAST>(grid, s, g);
    else
        Family::template kernel<BM, BN, WM, WN, true, true, FAST>(grid, s, g);
}

template <class Family, int BM, int BN, int WM, int WN>
void gemm_launch_tile(bool ta, bool tb, dim3 grid, hipStream_t s, const GemmArgs &g)
{
    if (Family::fast(BM, BN, tb, g))
        gemm_launch_as<Family, BM, BN, WM, WN, true>(ta, tb, grid, s, g);
    else
        gemm_launch_as<Family, BM, BN, WM, WN, false>(ta, tb, grid, s, g);
}

// What gemm_f32_launch / gemm_bf16_launch do (declared above).
template <class Family>
int gemm_launch(const char *name, int trans_a, int trans_b, int M, int N, int K, const float *A, int lda, const float *B,
                int ldb, float *C, int ldc, const float *bias, int accumulate, int fold_b, int fold_c, hipStream_t s,
                double *colstats, float *ordered_ws)
{
    CLOUDAAE_REQUIRE(M >= 0 && N >= 0 && K >= 0, name, "negative size");
    if (M == 0 || N == 0)
        return 0;
    CLOUDAAE_REQUIRE(lda >= (trans_a ? M : K), name, "leading dimension too small");
    CLOUDAAE_REQUIRE(fold_b ? ldb == fold_b : ldb >= (trans_b ? K : N), name, "leading dimension too small");
    CLOUDAAE_REQUIRE(fold_c ? ldc == fold_c : ldc >= N, name, "leading dimension too small");
    CLOUDAAE_REQUIRE((fold_b & (fold_b - 1)) == 0 && (fold_c & (fold_c - 1)) == 0 && fold_b % 4 == 0 &&
                         fold_c % 4 == 0, name, "fold width must be a power of two >= 4");
    Fold fb = {-1, 0}, fc = {-1, 0};
    if (fold_b) {           // B's folded index: n for [K][N] storage, k for [N][K] storage
        fb.shift = __builtin_ctz((unsigned)fold_b);
        fb.rows = trans_b ? N : K;
    }
    if (fold_c) {
        fc.shift = __builtin_ctz((unsigned)fold_c);
        fc.rows = M;
    }

    const GemmCut cut = gemm_cut<Family>(M, N, K, ordered_ws != nullptr);
    const int tm = ceil_div(M, cut.BM), tn = ceil_div(N, cut.BN);
    CLOUDAAE_REQUIRE(tm <= 65535, name, "M too large");
    CLOUDAAE_REQUIRE(colstats == nullptr || (cut.splits == 1 && accumulate == 0 && !fold_c), name,
                     "column statistics need an unsplit, overwriting product");
    // accumulate: 0 = overwrite C, 1 = add to C, 2 = C is known to hold zeros (the caller cleared
    // a whole gradient buffer once): plain stores when K is not split, atomics WITHOUT the clear
    // pass when it is
    GemmArgs g = {M, N, K, A, lda, B, ldb, C, ldc, bias, accumulate == 1 ? EPI_ACCUM : EPI_STORE, cut.kchunk, 0, 0,
                  fb, fc, colstats, 0};
    // ordered_ws: a product cut over K keeps its slices apart -- slice s stores its [M, N] result at
    // ordered_ws + s M N -- and a second kernel sums them in slice order (bit-reproducible, unlike the atomics)
    const bool ordered = ordered_ws != nullptr && cut.splits > 1;
    CLOUDAAE_REQUIRE(ordered_ws == nullptr || (accumulate == 0 && colstats == nullptr), name,
                     "slice-ordered products overwrite their output");
    if (ordered) {
        g.C = ordered_ws;
        g.ldc = N;
        g.bias = nullptr;
        g.cslice = (long long)M * N;
        g.fc = Fold{-1, 0};             // the slices are plain [M, N] blocks; the sum kernel folds the output
    } else if (cut.splits > 1) {
        g.epi = EPI_ATOMIC;
        if (!accumulate)    // slices add into a zeroed output
            CLOUDAAE_CHECK_HIP(gemm_zero_output(C, M, N, ldc, fold_c != 0, s), name);
    }
    g.vecA = ((uintptr_t)A & 15) == 0 && lda % 4 == 0 ? 1 : 0;
    g.vecB = ((uintptr_t)B & 15) == 0 && ldb % 4 == 0 ? 1 : 0;
    Family::tiles(cut.BM, cut.BN, trans_a != 0, trans_b != 0, dim3(tn, tm, cut.splits), s, g);
    CLOUDAAE_CHECK_LAUNCH(name);
    if (ordered)
        return gemm_slices_sum(name, M, N, cut.splits, ordered_ws, C, ldc, bias, s, fc);
    return 0;
}

// The C-ABI queries and entry points of a family (cloudaae_gemm_{f32,bf16}_*).
template <class Family>
int gemm_splits(int M, int N, int K)
{
    return M <= 0 || N <= 0 || K <= 0 ? 1 : gemm_cut<Family>(M, N, K, false).splits;
}

template <class Family>
int gemm_colstats_parts(int M, int N, int K)
{
    if (M <= 0 || N <= 0 || K <= 0)
        return 0;
    const GemmCut c = gemm_cut<Family>(M, N, K, false);
    return c.splits == 1 ? ceil_div(M, c.BM) : 0;      // one row of sums per tile row
}

template <class Family>
long long gemm_ordered_workspace(int M, int N, int K)
{
    if (M <= 0 || N <= 0 || K <= 0)
        return 0;
    const GemmCut c = gemm_cut<Family>(M, N, K, true);
    return c.splits > 1 ? (long long)c.splits * M * N : 0;
}

// the slice-ordered product (cloudaae_gemm_*_ordered): the caller's workspace must cover the cut
template <class Family>
int gemm_ordered(const char *name, int trans_a, int trans_b, int M, int N, int K, const float *A,
                 int lda, const float *B, int ldb, float *C, int ldc, const float *bias, int fold_c, float *workspace,
                 long long workspace_floats, hipStream_t s)
{
    // (the cut is derived again at every launch, also from development knobs: a buffer sized by an earlier query must
    //  still cover it)
    const long long need = gemm_ordered_workspace<Family>(M, N, K);
    CLOUDAAE_REQUIRE(workspace != nullptr ? workspace_floats >= need : need == 0, name, Family::ws_missing);
    static float dummy_ws;      // (a product that stays whole never touches it; non-NULL selects the ordered plan)
    return gemm_launch<Family>(name, trans_a, trans_b, M, N, K, A, lda, B, ldb, C, ldc, bias, 0, 0, fold_c, s, nullptr,
                               workspace != nullptr ? workspace : &dummy_ws);
}

} // namespace cloudaae
