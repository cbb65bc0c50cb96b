// pose_verify.hip -- the device side of pose verification: hypotheses composed from a base pose, and the choice of the
// winner from the counts of depth_fit.hip (the per-pixel agreement of each rendered hypothesis with the depth the camera
// saw).  DESIGN.md, "Pose verification", is the definition; tests/pose_verify_reference.py restates it in NumPy.  The
// composition is fp64, un-fused (the file is compiled with -ffp-contract=off), products and sums in the written order; the
// winner is chosen by integer cross-multiplication, so nothing depends on the order of execution, the batch or the run.
//
//   cloudaae_pose_compose       one launch, one lane per (sample, hypothesis): base_i H_{c,j}, its log map
//                               (icp_log_map of pose_math.h) and the float translation.
//   cloudaae_select_pose        one launch, one lane per sample: the largest num / den (df_fraction of depth_fit.h) by
//                               int64 cross-multiplication.
#include "common.h"
#include "depth_fit.h"
#include "pose_math.h"
#include "../../include/cloudaae_hip.h"

#include <limits.h>
#include <math.h>

namespace cloudaae {

typedef unsigned long long u64;

constexpr long long PV_MAX_TOTAL = 1ll << 28;      // B P

// ---- cloudaae_pose_compose ---------------------------------------------------------------------------------------------
constexpr int PC_BLOCK = 64;

__global__ __launch_bounds__(PC_BLOCK) void pose_compose_kernel(int n, int p, const double *__restrict__ base,
                                                                const long long *__restrict__ class_id, int nclass,
                                                                const int *__restrict__ hyp_index, int n_total,
                                                                const double *__restrict__ hyp,
                                                                double *__restrict__ pose, double *__restrict__ rot_axag,
                                                                float *__restrict__ trans, int *__restrict__ valid)
{
    const int e = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (e >= n)
        return;
    const int i = e / p, j = e % p;
    // the class's members; anything that would leave the table is an empty set and is never followed
    int first = 0, count = 0;
    const long long cls = class_id[i];
    if (cls >= 0 && cls < nclass) {
        first = hyp_index[cls];
        count = hyp_index[cls + 1] - first;
        if (first < 0 || count < 0 || (long long)first + count > n_total)
            count = 0;
    }
    const bool ok = j < count;
    double H[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};       // an empty set: the identity
    if (count > 0) {
        const double *src = hyp + 16ll * (first + (ok ? j : 0));
        for (int k = 0; k < 12; ++k)
            H[k] = src[k];
    }
    const double *A = base + 16ll * i;
    double C[12], R[9], r[3];
    for (int row = 0; row < 3; ++row) {
        const double a0 = A[4 * row + 0], a1 = A[4 * row + 1], a2 = A[4 * row + 2], a3 = A[4 * row + 3];
        for (int c = 0; c < 3; ++c)
            C[4 * row + c] = (a0 * H[c] + a1 * H[4 + c]) + a2 * H[8 + c];
        C[4 * row + 3] = ((a0 * H[3] + a1 * H[7]) + a2 * H[11]) + a3;
    }
    for (int row = 0; row < 3; ++row)
        for (int c = 0; c < 3; ++c)
            R[3 * row + c] = C[4 * row + c];
    icp_log_map(R, r);
    double *out = pose + 16ll * e;
    for (int k = 0; k < 12; ++k)
        out[k] = C[k];
    out[12] = out[13] = out[14] = 0.0;
    out[15] = 1.0;
    for (int k = 0; k < 3; ++k) {
        rot_axag[3ll * e + k] = r[k];
        trans[3ll * e + k] = (float)C[4 * k + 3];
    }
    valid[e] = ok ? 1 : 0;
}

// ---- cloudaae_select_pose ----------------------------------------------------------------------------------------------
constexpr int SP_BLOCK = 64;

__global__ __launch_bounds__(SP_BLOCK) void select_pose_kernel(int b, int p, const int *__restrict__ counts,
                                                               const int *__restrict__ seg_total,
                                                               const int *__restrict__ valid,
                                                               const double *__restrict__ pose, int mode,
                                                               int *__restrict__ best, double *__restrict__ score,
                                                               double *__restrict__ pose_best, double *__restrict__ margin)
{
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= b)
        return;
    const int st = seg_total[i];
    const size_t row = (size_t)i * p;
    int win = 0, second = -1;
    long long wn = 0, wd = 1, rn = 0, rd = 1;      // the winner's and the runner-up's fraction
    for (int j = 0; j < p; ++j) {
        long long num, den;
        df_fraction(counts + (row + j) * DF_COUNTERS, st, valid[row + j] != 0, mode, num, den);
        score[row + j] = num == 0 ? 0.0 : (double)num / (double)den;
        if (j == 0) {
            wn = num, wd = den;
        } else if (num * wd > wn * den) {          // strictly larger: ties stay with the lower index
            second = win, rn = wn, rd = wd;
            win = j, wn = num, wd = den;
        } else if (second < 0 || num * rd > rn * den) {
            second = j, rn = num, rd = den;
        }
    }
    best[i] = win;
    const double ws = wn == 0 ? 0.0 : (double)wn / (double)wd, rs = rn == 0 ? 0.0 : (double)rn / (double)rd;
    margin[i] = second < 0 ? 0.0 : ws - rs;
    for (int k = 0; k < 16; ++k)
        pose_best[16ll * i + k] = pose[16ll * (row + win) + k];
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_pose_compose(int b, const double *base, const long long *class_id, int nclass, const int *hyp_index,
                                       int n_total, const double *hyp, int p, double *pose, double *rot_axag, float *trans,
                                       int *valid, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_pose_compose";
    CLOUDAAE_REQUIRE(b >= 1 && p >= 1 && (long long)b * p <= PV_MAX_TOTAL, name, "b and p must be >= 1 and b * p <= 2^28");
    CLOUDAAE_REQUIRE(nclass >= 1 && n_total >= 0 && n_total <= (1 << 24), name, "nclass must be >= 1 and n_total in [0, 2^24]");
    CLOUDAAE_REQUIRE(base && class_id && hyp_index && pose && rot_axag && trans && valid, name, "null pointer");
    CLOUDAAE_REQUIRE(hyp || n_total == 0, name, "hyp is null with n_total > 0");
    const int n = b * p;
    hipLaunchKernelGGL(pose_compose_kernel, dim3(ceil_div(n, PC_BLOCK)), dim3(PC_BLOCK), 0, (hipStream_t)stream, n, p, base,
                       class_id, nclass, hyp_index, n_total, hyp, pose, rot_axag, trans, valid);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_select_pose(int b, int p, const int *counts, const int *seg_total, const int *valid,
                                      const double *pose, int mode, int *best, double *score, double *pose_best,
                                      double *margin, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_select_pose";
    CLOUDAAE_REQUIRE(b >= 1 && p >= 1 && (long long)b * p <= PV_MAX_TOTAL, name, "b and p must be >= 1 and b * p <= 2^28");
    CLOUDAAE_REQUIRE(mode == 0 || mode == 1, name, "mode must be 0 (segment rule) or 1 (silhouette rule)");
    CLOUDAAE_REQUIRE(counts && seg_total && valid && pose && best && score && pose_best && margin, name, "null pointer");
    hipLaunchKernelGGL(select_pose_kernel, dim3(ceil_div(b, SP_BLOCK)), dim3(SP_BLOCK), 0, (hipStream_t)stream, b, p, counts,
                       seg_total, valid, pose, mode, best, score, pose_best, margin);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
