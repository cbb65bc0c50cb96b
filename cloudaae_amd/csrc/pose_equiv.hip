// pose_equiv.hip -- the nearest equivalent ground-truth pose of a symmetric object: of all label poses T_label o [S | c - S c]
// with S in the object's rotational symmetry set, the one whose rotation is closest to the predicted rotation.  DESIGN.md,
// "Equivalent poses", is the definition; tests/pose_equiv_reference.py restates it in NumPy.  All floating point is fp64,
// un-fused (the file is compiled with -ffp-contract=off), products and sums in the written order; the exponential map is
// exp_map of so3_dual.h on constant duals -- the op sequence of the loss -- and the log map is icp_log_map of pose_math.h.
//
//   cloudaae_nearest_equivalent_pose   one launch.  One wave64 per sample, four samples per workgroup of 256 lanes.  Every
//                                      lane forms Rp, Rl and M = Rp^T Rl (wave-uniform work, no exchange); lane j forms
//                                      the trace s_j = tr(M G_j) of member j of a finite set, lanes 0 and 1 the closed-form
//                                      maximum over the rotations about the axis of their coset.  The argmax is a butterfly
//                                      on (value, index), the lower index winning ties; lane 0 forms S*, the log map of
//                                      Rl S* and the shifted translation and writes the sample's five outputs.  No LDS, no
//                                      atomics, nothing waits on another wave; the only loop is the butterfly.
#include "common.h"
#include "pose_math.h"
#include "so3_dual.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

namespace cloudaae {

constexpr int PE_BLOCK = 256;
constexpr int PE_SAMPLES = PE_BLOCK / 64;          // one wave per sample
constexpr int PE_MAX_B = 1 << 24;
constexpr int PE_MAX_MEMBERS = CLOUDAAE_SYMMETRY_MAX_MEMBERS;
static_assert(PE_MAX_MEMBERS == 64, "one member of a finite set per lane of a wave");

// (value, index) of the largest value over the wave, the lowest index among equals: the same pair in every lane
__device__ __forceinline__ void wave_argmax(double &v, int &idx)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (ov > v || (ov == v && oi < idx)) {
            v = ov;
            idx = oi;
        }
    }
}

// C = A B, C[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]
__device__ __forceinline__ void pe_matmul(const double A[3][3], const double B[3][3], double C[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            C[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j];
}

__device__ __forceinline__ void pe_exp(double x, double y, double z, double R[3][3])
{
    const Dual ax[3] = {dconst(x), dconst(y), dconst(z)};
    Dual D[3][3];
    exp_map(ax, D);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[i][j] = D[i][j].v;
}

__global__ __launch_bounds__(PE_BLOCK) void nearest_equivalent_pose_kernel(
    int b, const void *__restrict__ rot_pred, int rot_pred_is_f64, const double *__restrict__ rot_label,
    const float *__restrict__ trans_label, const long long *__restrict__ class_id, int num_class,
    const int *__restrict__ sym_index, const double *__restrict__ sym_centre, const double *__restrict__ sym_axis, int num_rot,
    const double *__restrict__ sym_rot, double *__restrict__ rot_equiv, float *__restrict__ trans_equiv,
    int *__restrict__ member, double *__restrict__ phi, double *__restrict__ angle)
{
    const int lane = lane_id();
    const long long i = (long long)blockIdx.x * PE_SAMPLES + (threadIdx.x >> 6);
    if (i >= b)                         // the whole wave leaves
        return;

    // the class's entry; anything that would leave the table's arrays is `none` and is never followed
    int kind = CLOUDAAE_SYMMETRY_NONE, first = 0, count = 0;
    const long long cls = class_id[i];
    if (cls >= 0 && cls < num_class) {
        kind = sym_index[3 * cls + 0];
        first = sym_index[3 * cls + 1];
        count = sym_index[3 * cls + 2];
        const bool inside = first >= 0 && count >= 0 && (long long)first + count <= num_rot;
        if (kind == CLOUDAAE_SYMMETRY_FINITE) {
            if (!inside || count < 1 || count > PE_MAX_MEMBERS)
                kind = CLOUDAAE_SYMMETRY_NONE;
        } else if (kind == CLOUDAAE_SYMMETRY_AXIAL) {
            if (!inside || count > 1)
                kind = CLOUDAAE_SYMMETRY_NONE;
        } else {
            kind = CLOUDAAE_SYMMETRY_NONE;
        }
    }

    double Rp[3][3], Rl[3][3], M[3][3];
    if (rot_pred_is_f64) {
        const double *r = static_cast<const double *>(rot_pred) + 3 * i;
        pe_exp(r[0], r[1], r[2], Rp);
    } else {
        const float *r = static_cast<const float *>(rot_pred) + 3 * i;
        pe_exp((double)r[0], (double)r[1], (double)r[2], Rp);
    }
    pe_exp(rot_label[3 * i + 0], rot_label[3 * i + 1], rot_label[3 * i + 2], Rl);
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k)
            M[r][k] = (Rp[0][r] * Rl[0][k] + Rp[1][r] * Rl[1][k]) + Rp[2][r] * Rl[2][k];

    if (kind == CLOUDAAE_SYMMETRY_NONE) {
        // S* = I: the label itself, passed on bit for bit
        if (lane == 0) {
            const double t = ((M[0][0] + M[1][1]) + M[2][2] - 1.0) / 2.0;
            for (int k = 0; k < 3; ++k) {
                rot_equiv[3 * i + k] = rot_label[3 * i + k];
                trans_equiv[3 * i + k] = trans_label[3 * i + k];
            }
            member[i] = 0;
            phi[i] = 0.0;
            angle[i] = acos(fmin(fmax(t, -0.9999999), 0.9999999));
        }
        return;
    }

    double a[3] = {0.0, 0.0, 0.0};
    double s = -(double)INFINITY, ph = 0.0;
    int best = lane;
    if (kind == CLOUDAAE_SYMMETRY_FINITE) {
        if (lane < count) {
            const double *G = sym_rot + 9LL * (first + lane);
            s = 0.0;
            for (int r = 0; r < 3; ++r) {
                const double t = (M[r][0] * G[0 + r] + M[r][1] * G[3 + r]) + M[r][2] * G[6 + r];
                s = r == 0 ? t : s + t;
            }
        }
    } else {
        for (int k = 0; k < 3; ++k)
            a[k] = sym_axis[3 * cls + k];
        if (lane <= count) {            // coset 0 = the rotations about a, coset 1 = the half-turn F times them
            double N[3][3];
            if (lane == 0) {
                for (int r = 0; r < 3; ++r)
                    for (int k = 0; k < 3; ++k)
                        N[r][k] = M[r][k];
            } else {
                const double *Fp = sym_rot + 9LL * first;
                double F[3][3];
                for (int r = 0; r < 3; ++r)
                    for (int k = 0; k < 3; ++k)
                        F[r][k] = Fp[3 * r + k];
                pe_matmul(M, F, N);
            }
            double u[3];
            for (int r = 0; r < 3; ++r)
                u[r] = (N[r][0] * a[0] + N[r][1] * a[1]) + N[r][2] * a[2];
            const double alpha = (a[0] * u[0] + a[1] * u[1]) + a[2] * u[2];
            const double tau = (N[0][0] + N[1][1]) + N[2][2];
            const double beta = (a[0] * (N[1][2] - N[2][1]) + a[1] * (N[2][0] - N[0][2])) + a[2] * (N[0][1] - N[1][0]);
            const double d = tau - alpha;
            s = alpha + sqrt(d * d + beta * beta);
            ph = (d == 0.0 && beta == 0.0) ? 0.0 : atan2(beta, d);
        }
    }
    wave_argmax(s, best);
    ph = __shfl(ph, best, 64);
    if (lane != 0)
        return;

    // S* = G_best, or E_best R_a(phi)
    double S[3][3];
    if (kind == CLOUDAAE_SYMMETRY_FINITE) {
        const double *G = sym_rot + 9LL * (first + best);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k)
                S[r][k] = G[3 * r + k];
    } else {
        const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
        double K2[3][3], R[3][3];
        pe_matmul(K, K, K2);
        const double sn = sin(ph), vs = 1.0 - cos(ph);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k)
                R[r][k] = ((r == k ? 1.0 : 0.0) + sn * K[r][k]) + vs * K2[r][k];
        if (best == 0) {
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 3; ++k)
                    S[r][k] = R[r][k];
        } else {
            const double *Fp = sym_rot + 9LL * first;
            double F[3][3];
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 3; ++k)
                    F[r][k] = Fp[3 * r + k];
            pe_matmul(F, R, S);
        }
    }

    // S* = I exactly (member 0 of a finite set; no turn about the axis): the label itself, as for `none`
    bool identity = true;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k)
            identity = identity && S[r][k] == (r == k ? 1.0 : 0.0);
    if (identity) {
        for (int k = 0; k < 3; ++k) {
            rot_equiv[3 * i + k] = rot_label[3 * i + k];
            trans_equiv[3 * i + k] = trans_label[3 * i + k];
        }
        member[i] = best;
        phi[i] = ph;
        angle[i] = acos(fmin(fmax((s - 1.0) / 2.0, -0.9999999), 0.9999999));
        return;
    }

    double Q[3][3], Qf[9], r3[3], c[3], w[3];
    pe_matmul(Rl, S, Q);
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k)
            Qf[3 * r + k] = Q[r][k];
    icp_log_map(Qf, r3);
    for (int k = 0; k < 3; ++k)
        c[k] = sym_centre[3 * cls + k];
    for (int r = 0; r < 3; ++r)
        w[r] = c[r] - ((S[r][0] * c[0] + S[r][1] * c[1]) + S[r][2] * c[2]);
    for (int r = 0; r < 3; ++r) {
        const double v = (Rl[r][0] * w[0] + Rl[r][1] * w[1]) + Rl[r][2] * w[2];
        rot_equiv[3 * i + r] = r3[r];
        trans_equiv[3 * i + r] = (float)((double)trans_label[3 * i + r] + v);
    }
    member[i] = best;
    phi[i] = ph;
    angle[i] = acos(fmin(fmax((s - 1.0) / 2.0, -0.9999999), 0.9999999));
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_nearest_equivalent_pose(int b, const void *rot_pred, int rot_pred_is_f64, const double *rot_label,
                                                  const float *trans_label, const long long *class_id, int num_class,
                                                  const int *sym_index, const double *sym_centre, const double *sym_axis,
                                                  int num_rot, const double *sym_rot, double *rot_equiv, float *trans_equiv,
                                                  int *member, double *phi, double *angle, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_nearest_equivalent_pose";
    CLOUDAAE_REQUIRE(b >= 1 && b <= PE_MAX_B, name, "b must lie in [1, 2^24]");
    CLOUDAAE_REQUIRE(rot_pred_is_f64 == 0 || rot_pred_is_f64 == 1, name, "rot_pred_is_f64 must be 0 or 1");
    CLOUDAAE_REQUIRE(num_class >= 1, name, "num_class must be >= 1");
    CLOUDAAE_REQUIRE(num_rot >= 0 && num_rot <= (1 << 24), name, "num_rot must lie in [0, 2^24]");
    CLOUDAAE_REQUIRE(rot_pred && rot_label && trans_label && class_id && sym_index && sym_centre && sym_axis && rot_equiv &&
                         trans_equiv && member && phi && angle,
                     name, "null pointer");
    CLOUDAAE_REQUIRE(sym_rot || num_rot == 0, name, "sym_rot is null with num_rot > 0");
    hipLaunchKernelGGL(nearest_equivalent_pose_kernel, dim3(ceil_div(b, PE_SAMPLES)), dim3(PE_BLOCK), 0, (hipStream_t)stream, b,
                       rot_pred, rot_pred_is_f64, rot_label, trans_label, class_id, num_class, sym_index, sym_centre, sym_axis,
                       num_rot, sym_rot, rot_equiv, trans_equiv, member, phi, angle);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
