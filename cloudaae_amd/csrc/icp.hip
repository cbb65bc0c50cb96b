// icp.hip -- batched point-to-point ICP: the pose refinement of the reference's evaluation
// (evaluate_cloudAAE_ycbv.py:606-628: ten open3d registration_icp calls, correspondence radius 0.01 m times 0.9
// after each call).  The definition the kernel implements, in float64, is written out in DESIGN.md ("Pose
// refinement") and restated in NumPy by tests/icp_reference.py.
//
// One workgroup per cloud runs the whole schedule: no communication between workgroups, no spin-wait, every loop
// statically bounded (rounds x max_iteration updates, ICP_JACOBI_SWEEPS sweeps).  A cloud's result does not depend
// on the batch it sits in, and every sum is taken in a fixed order, so a launch is bit-reproducible.
//   - the target (scene) lives in LDS, sorted by a spatial hash of cubic cells of edge h = radius * (1 + 2^-20)
//     (counting sort, built once per launch).  A query probes the cell of p and those of its 26 neighbours that the
//     ball of radius rho can reach (with a margin of 1e-6 cell): any q with d < rho <= radius lies in them, and a
//     hash collision only adds candidates.  Distances are fp64 on the exact fp32 inputs: the correspondences are
//     those of the definition.
//   - the transformed source points sit in registers, ICP_PER_LANE per lane.  The 17 sums of an update (count,
//     sum p, sum q, sum q p^T, sum d^2) are taken per lane in point order, across the wave by a butterfly, across
//     the waves in wave order; the points are shifted by the initial translation first, so the cross moments do
//     not cancel.
//   - thread 0 solves the 3x3 orthogonal Procrustes problem by Horn's quaternion method (the proper rotation that
//     maximises tr(R^T Sigma): Umeyama's answer with the reflection fix) with a cyclic Jacobi eigen-solver on the
//     4x4 symmetric matrix, and broadcasts the update and the convergence decision through LDS.
//
// cloudaae_icp_point_to_plane is the same kernel template with another estimator (PLANE = true): the same hash grid,
// matching, tie rule, statistics and stopping rule; the sums of an update are the 21 + 6 entries of A = sum J J^T and
// b = sum J r (J = [p x n; n], r = (p - q) . n, n the matched target point's normal, read from global memory by the
// match's index), taken in the same order; thread 0 solves the 6x6 system by LDL^T.  The point-to-point instantiation
// keeps its arithmetic statement for statement.
#include "common.h"
#include "../../include/cloudaae_hip.h"
#include "pose_math.h"   // icp_rodrigues, icp_apply: shared with pose_score.hip; icp_log_map: with pose_equiv.hip

#include <math.h>

using namespace cloudaae;

namespace {

constexpr int ICP_THREADS = 512;
constexpr int ICP_WAVES = ICP_THREADS / 64;
constexpr int ICP_PER_LANE = 8;
constexpr int ICP_MAX_M = ICP_THREADS * ICP_PER_LANE;     // source points of a cloud (CLOUDAAE_ICP_MAX_POINTS)
constexpr int ICP_MAX_N = 4096;                           // target points of a cloud (CLOUDAAE_ICP_MAX_POINTS)
constexpr int ICP_SUMS = 17;                              // point to point: count, sum p, sum q, sum q p^T, sum d^2
constexpr int ICP_PLANE_SUMS = 29;                        // point to plane: count, sum d^2, A's upper triangle, b
constexpr int ICP_JACOBI_SWEEPS = 16;
constexpr double ICP_CELL_CLAMP = 268435456.0;            // 2^28: cell coordinates (and their neighbours) fit an int
constexpr double ICP_REACH_MARGIN = 1e-6;                 // cell units; rounding of p * (1/h) is far below it

// hash buckets: a power of two >= 2n, at least one per thread (the scan gives each thread a whole number of them)
static int icp_hash_bits(int n)
{
    int bits = 10;
    while ((1 << bits) < 2 * n)
        ++bits;
    return bits;
}

static size_t icp_lds_bytes(int n, int hbits, int sums)
{
    return sizeof(double) * (ICP_WAVES * sums + 64) + sizeof(float4) * (size_t)n +
           sizeof(int) * ((size_t)(1 << hbits) + 1 + ICP_WAVES);
}

__device__ __forceinline__ int icp_cell(double f)
{
    return (int)fmin(fmax(floor(f), -ICP_CELL_CLAMP), ICP_CELL_CLAMP);
}

__device__ __forceinline__ int icp_bucket(int cx, int cy, int cz, unsigned mask)
{
    return (int)((((unsigned)cx * 73856093u) ^ ((unsigned)cy * 19349663u) ^ ((unsigned)cz * 83492791u)) & mask);
}

}  // namespace

// ---- the 3x3 / 4x4 arithmetic of thread 0 (host-callable: it is plain fp64 code) ---------------------------------

// The rotation R (row-major 3x3) that maximises tr(R^T S) over SO(3), for S = Sigma = (1/n) sum (q - mq)(p - mp)^T:
// Horn's quaternion -- the eigenvector of the largest eigenvalue of the symmetric 4x4 matrix built from S -- by
// cyclic Jacobi rotations.  Any S (rank-deficient, zero) gives a unit quaternion, hence a finite proper rotation.
__host__ __device__ inline void icp_procrustes(const double *S, double *R)
{
    // Horn's S_ab = sum p_a q_b = Sigma_ba
    const double sxx = S[0], sxy = S[3], sxz = S[6];
    const double syx = S[1], syy = S[4], syz = S[7];
    const double szx = S[2], szy = S[5], szz = S[8];
    double A[4][4] = {{(sxx + syy) + szz, syz - szy, szx - sxz, sxy - syx},
                      {syz - szy, (sxx - syy) - szz, sxy + syx, szx + sxz},
                      {szx - sxz, sxy + syx, (syy - sxx) - szz, syz + szy},
                      {sxy - syx, szx + sxz, syz + szy, (szz - sxx) - syy}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < ICP_JACOBI_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (fabs(apq) <= 1e-300 || fabs(apq) <= 1e-18 * (fabs(A[p][p]) + fabs(A[q][q]))) {
                    A[p][q] = A[q][p] = 0.0;
                    continue;
                }
                rotated = true;
                const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r == p || r == q)
                        continue;
                    const double arp = A[r][p], arq = A[r][q];
                    A[r][p] = A[p][r] = c * arp - s * arq;
                    A[r][q] = A[q][r] = s * arp + c * arq;
                }
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
            }
        }
        if (!rotated)
            break;
    }
    // the largest eigenvalue's column (the first of equals), selected without indexing by a run-time value
    double w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0], top = A[0][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > top) {
            top = A[i][i];
            w = V[0][i];
            x = V[1][i];
            y = V[2][i];
            z = V[3][i];
        }
    const double qn = sqrt(((w * w + x * x) + y * y) + z * z);
    w /= qn;
    x /= qn;
    y /= qn;
    z /= qn;
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

namespace {

struct IcpShared {
    double *red;      // [ICP_WAVES][NS] per-wave partial sums
    double *bc;       // [0..11] T (3x4), [12..23] update U (3x4), [24] continue flag, [25] apply flag, [32..32+NS) sums
    float4 *tgt;      // [n] target points sorted by bucket, .w = the point's index (int bits)
    int *start;       // [H + 1] bucket starts
    int *wsum;        // [ICP_WAVES] scan totals
};

// Correspondences of this lane's points at rho and the workgroup's sums (thread 0 leaves them in L.bc[32..32+NS)):
// the 17 of the point-to-point update, or (PLANE, nrm = the cloud's target normals [n,3]) count, sum d^2, the upper
// triangle of sum J J^T row by row and sum J r.
template <bool PLANE>
__device__ __forceinline__ void icp_match(const IcpShared &L, const double (&P)[ICP_PER_LANE][3], int m, double rho2,
                                          double inv_h, double reach, unsigned mask, const double *ctr,
                                          const double *__restrict__ nrm)
{
    constexpr int NS = PLANE ? ICP_PLANE_SUMS : ICP_SUMS;
    const int tid = threadIdx.x;
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k)
        acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < ICP_PER_LANE; ++k) {
        if (k * ICP_THREADS + tid >= m)
            break;
        const double px = P[k][0], py = P[k][1], pz = P[k][2];
        const double fx = px * inv_h, fy = py * inv_h, fz = pz * inv_h;
        const int cx = icp_cell(fx), cy = icp_cell(fy), cz = icp_cell(fz);
        int x0 = -1, x1 = 1, y0 = -1, y1 = 1, z0 = -1, z1 = 1;
        if (fabs(fx) < 0.5 * ICP_CELL_CLAMP && fabs(fy) < 0.5 * ICP_CELL_CLAMP && fabs(fz) < 0.5 * ICP_CELL_CLAMP) {
            x0 = fx - (double)cx < reach ? -1 : 0;
            x1 = ((double)cx + 1.0) - fx < reach ? 1 : 0;
            y0 = fy - (double)cy < reach ? -1 : 0;
            y1 = ((double)cy + 1.0) - fy < reach ? 1 : 0;
            z0 = fz - (double)cz < reach ? -1 : 0;
            z1 = ((double)cz + 1.0) - fz < reach ? 1 : 0;
        }
        double best = 0.0;
        int bj = -1;
        float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int dz = z0; dz <= z1; ++dz)
            for (int dy = y0; dy <= y1; ++dy)
                for (int dx = x0; dx <= x1; ++dx) {
                    const int b = icp_bucket(cx + dx, cy + dy, cz + dz, mask);
                    const int e = L.start[b + 1];
                    for (int t = L.start[b]; t < e; ++t) {
                        const float4 q = L.tgt[t];
                        const double ex = px - (double)q.x, ey = py - (double)q.y, ez = pz - (double)q.z;
                        const double d2 = (ex * ex + ey * ey) + ez * ez;
                        const int j = __float_as_int(q.w);
                        if (d2 < rho2 && (bj < 0 || d2 < best || (d2 == best && j < bj))) {
                            best = d2;
                            bj = j;
                            bq = q;
                        }
                    }
                }
        if constexpr (PLANE) {
            if (bj >= 0) {
                const double *nq = nrm + 3LL * bj;
                const double n0 = nq[0], n1 = nq[1], n2 = nq[2];
                const double ex = px - (double)bq.x, ey = py - (double)bq.y, ez = pz - (double)bq.z;
                const double res = (ex * n0 + ey * n1) + ez * n2;
                const double J[6] = {py * n2 - pz * n1, pz * n0 - px * n2, px * n1 - py * n0, n0, n1, n2};
                acc[0] += 1.0;
                acc[1] += best;
                int t = 2;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b)
                        acc[t++] += J[a] * J[b];
#pragma unroll
                for (int a = 0; a < 6; ++a)
                    acc[23 + a] += J[a] * res;
            }
        } else if (bj >= 0) {
            const double ax = px - ctr[0], ay = py - ctr[1], az = pz - ctr[2];
            const double bx = (double)bq.x - ctr[0], by = (double)bq.y - ctr[1], bz = (double)bq.z - ctr[2];
            acc[0] += 1.0;
            acc[1] += ax;
            acc[2] += ay;
            acc[3] += az;
            acc[4] += bx;
            acc[5] += by;
            acc[6] += bz;
            acc[7] += bx * ax;
            acc[8] += bx * ay;
            acc[9] += bx * az;
            acc[10] += by * ax;
            acc[11] += by * ay;
            acc[12] += by * az;
            acc[13] += bz * ax;
            acc[14] += bz * ay;
            acc[15] += bz * az;
            acc[16] += best;
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k)
        acc[k] = wave_sum(acc[k]);
    const int w = tid >> 6;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k)
            L.red[w * NS + k] = acc[k];
    }
    __syncthreads();
    if (tid == 0) {
        #pragma unroll
        for (int k = 0; k < NS; ++k) {
            double v = L.red[k];
            for (int i = 1; i < ICP_WAVES; ++i)
                v += L.red[i * NS + k];
            L.bc[32 + k] = v;
        }
    }
}

// Thread 0: the update U (3x4) of Umeyama / Horn from the sums (count > 0).
__device__ inline void icp_update(const double *s, const double *ctr, double *U)
{
    const double n = s[0];
    const double mp[3] = {s[1] / n, s[2] / n, s[3] / n}, mq[3] = {s[4] / n, s[5] / n, s[6] / n};
    double S[9], R[9];
    #pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            S[3 * a + b] = s[7 + 3 * a + b] / n - mq[a] * mp[b];
    icp_procrustes(S, R);
    const double up[3] = {mp[0] + ctr[0], mp[1] + ctr[1], mp[2] + ctr[2]};
    #pragma unroll
    for (int a = 0; a < 3; ++a) {
        U[4 * a + 0] = R[3 * a + 0];
        U[4 * a + 1] = R[3 * a + 1];
        U[4 * a + 2] = R[3 * a + 2];
        U[4 * a + 3] = (mq[a] + ctr[a]) - ((R[3 * a] * up[0] + R[3 * a + 1] * up[1]) + R[3 * a + 2] * up[2]);
    }
}

// Thread 0: the point-to-plane update U (3x4) from the sums s = (count, sum d^2, A's upper triangle row by row, b).
// A x = -b by LDL^T; x = (alpha, beta, gamma, t); U = [Rz(gamma) Ry(beta) Rx(alpha) | t].  false (U = I: the caller
// leaves T and P alone) with fewer than six correspondences, a pivot that is not a finite number > 0, or a solution
// that is not finite.
__host__ __device__ inline bool icp_plane_update(const double *s, double *U)
{
    if (!(s[0] >= 6.0))
        return false;
    double A[6][6], Lm[6][6], d[6], x[6];
    int t = 2;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b)
            A[a][b] = A[b][a] = s[t++];
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
        for (int k = 0; k < j; ++k)
            dj -= (Lm[j][k] * Lm[j][k]) * d[k];
        if (!(dj > 0.0) || !isfinite(dj))
            return false;
        d[j] = dj;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k)
                v -= (Lm[i][k] * Lm[j][k]) * d[k];
            Lm[i][j] = v / dj;
        }
    }
    for (int i = 0; i < 6; ++i) {                      // L y = -b
        double v = -s[23 + i];
        for (int k = 0; k < i; ++k)
            v -= Lm[i][k] * x[k];
        x[i] = v;
    }
    for (int i = 0; i < 6; ++i)                        // D z = y
        x[i] = x[i] / d[i];
    for (int i = 5; i >= 0; --i) {                     // L^T x = z
        double v = x[i];
        for (int k = i + 1; k < 6; ++k)
            v -= Lm[k][i] * x[k];
        x[i] = v;
    }
    for (int i = 0; i < 6; ++i)
        if (!isfinite(x[i]))
            return false;
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    U[0] = cg * cb;
    U[1] = (cg * sb) * sa - sg * ca;
    U[2] = (cg * sb) * ca + sg * sa;
    U[3] = x[3];
    U[4] = sg * cb;
    U[5] = (sg * sb) * sa + cg * ca;
    U[6] = (sg * sb) * ca - cg * sa;
    U[7] = x[4];
    U[8] = -sb;
    U[9] = cb * sa;
    U[10] = cb * ca;
    U[11] = x[5];
    return true;
}

// T <- T^-1 for a rigid T (3x4): (R^T, -R^T t), the translation as -((R0i t0 + R1i t1) + R2i t2)
__host__ __device__ inline void icp_invert(double *T)
{
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, t[3] = {T[3], T[7], T[11]};
    for (int i = 0; i < 3; ++i) {
        T[4 * i] = R[i];
        T[4 * i + 1] = R[3 + i];
        T[4 * i + 2] = R[6 + i];
        T[4 * i + 3] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
    }
}

// T <- U T (both 3x4 with the implied last row 0 0 0 1): ((U_i0 T_0j + U_i1 T_1j) + U_i2 T_2j) + U_i3 T_3j
__device__ inline void icp_compose(const double *U, double *T)
{
    double N[12];
    #pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            N[4 * i + j] = ((U[4 * i] * T[j] + U[4 * i + 1] * T[4 + j]) + U[4 * i + 2] * T[8 + j]) +
                           U[4 * i + 3] * (j == 3 ? 1.0 : 0.0);
    #pragma unroll
    for (int k = 0; k < 12; ++k)
        T[k] = N[k];
}

// Thread 0: the estimator's update U from the sums; false = no update (U = I)
template <bool PLANE>
__device__ __forceinline__ bool icp_estimate(const double *sums, const double *ctr, double *U)
{
    if constexpr (PLANE) {
        return icp_plane_update(sums, U);
    } else {
        icp_update(sums, ctr, U);
        return true;
    }
}

// PLANE: nrm [b,n,3] = the target points' normals; inverse != 0: rot / trans and the results are the target -> source
// pose (inverted on entry and on exit).  Point to point takes nrm = nullptr, inverse = 0.
template <bool PLANE>
__global__ void __launch_bounds__(ICP_THREADS)
icp_kernel(const double *__restrict__ nrm_all, int inverse, int m, const float *__restrict__ src, int sps, long long scs, int n, const float *__restrict__ dst,
               int dps, long long dcs, const float *__restrict__ rot, const float *__restrict__ trans, double radius,
               double decay, int rounds, int max_it, double rel_fit, double rel_rmse, int hbits,
               double *__restrict__ T_out, double *__restrict__ rot_out, float *__restrict__ trans_out,
               double *__restrict__ fit_out, double *__restrict__ rmse_out, int *__restrict__ it_out)
{
    extern __shared__ double icp_lds[];
    constexpr int NS = PLANE ? ICP_PLANE_SUMS : ICP_SUMS;
    constexpr int D2 = PLANE ? 1 : 16;               // where the sums hold sum d^2
    const int H = 1 << hbits;
    IcpShared L;
    L.red = icp_lds;
    L.bc = L.red + ICP_WAVES * NS;
    L.tgt = reinterpret_cast<float4 *>(L.bc + 64);
    L.start = reinterpret_cast<int *>(L.tgt + n);
    L.wsum = L.start + H + 1;
    const int tid = threadIdx.x, c = blockIdx.x;
    const float *S = src + (long long)c * scs;
    const float *D = dst + (long long)c * dcs;
    const double *nrm = PLANE ? nrm_all + 3LL * (long long)c * n : nullptr;
    const double h = radius * (1.0 + 0x1p-20), inv_h = 1.0 / h;
    const unsigned mask = (unsigned)H - 1u;

    // ---- the target's spatial hash: count, scan, scatter ------------------------------------------------------
    for (int b = tid; b <= H; b += ICP_THREADS)
        L.start[b] = 0;
    __syncthreads();
    for (int j = tid; j < n; j += ICP_THREADS) {
        const float *q = D + (long long)j * dps;
        atomicAdd(&L.start[icp_bucket(icp_cell(q[0] * inv_h), icp_cell(q[1] * inv_h), icp_cell(q[2] * inv_h), mask)], 1);
    }
    __syncthreads();
    {
        const int per = H / ICP_THREADS;
        int run = 0;
        for (int i = 0; i < per; ++i)
            run += L.start[tid * per + i];
        int incl = run;                                   // inclusive scan of the per-thread totals in the wave
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            if ((tid & 63) >= off)
                incl += v;
        }
        if ((tid & 63) == 63)
            L.wsum[tid >> 6] = incl;
        __syncthreads();
        int base = 0;
        for (int w = 0; w < (tid >> 6); ++w)
            base += L.wsum[w];
        int acc = base + incl - run;
        for (int i = 0; i < per; ++i) {
            acc += L.start[tid * per + i];
            L.start[tid * per + i] = acc;                 // inclusive end of the bucket
        }
    }
    __syncthreads();
    for (int j = tid; j < n; j += ICP_THREADS) {
        const float *q = D + (long long)j * dps;
        const float x = q[0], y = q[1], z = q[2];
        const int b = icp_bucket(icp_cell(x * inv_h), icp_cell(y * inv_h), icp_cell(z * inv_h), mask);
        const int pos = atomicSub(&L.start[b], 1) - 1;     // ends -> starts; the order inside a bucket is free
        L.tgt[pos] = make_float4(x, y, z, __int_as_float(j));
    }
    __syncthreads();
    if (tid == 0) {
        L.start[H] = n;
        double R[9];
        icp_rodrigues((double)rot[3 * c], (double)rot[3 * c + 1], (double)rot[3 * c + 2], R);
        #pragma unroll
        for (int a = 0; a < 3; ++a) {
            L.bc[4 * a] = R[3 * a];
            L.bc[4 * a + 1] = R[3 * a + 1];
            L.bc[4 * a + 2] = R[3 * a + 2];
            L.bc[4 * a + 3] = (double)trans[3 * c + a];
        }
        if (PLANE && inverse)
            icp_invert(L.bc);
    }
    __syncthreads();

    // the sums are taken relative to the initial translation (the object's centre in the camera frame).  T lives in
    // L.bc: every thread reads it at a round's start, thread 0 changes it only after the round's first barrier.
    const double ctr[3] = {L.bc[3], L.bc[7], L.bc[11]};
    const double *sums = L.bc + 32;
    double P[ICP_PER_LANE][3] = {};
    double fit = 0.0, rmse = 0.0, rho = radius;      // fit, rmse: thread 0's
    const int nr = rounds > 0 ? rounds : 1;          // rounds = 0: the statistics of T0 at rho = radius
    for (int r = 0; r < nr; ++r) {
        const double rho2 = rho * rho, reach = rho * inv_h + ICP_REACH_MARGIN;
#pragma unroll
        for (int k = 0; k < ICP_PER_LANE; ++k) {
            const int i = k * ICP_THREADS + tid;
            if (i < m) {
                const float *x = S + (long long)i * sps;
                icp_apply(L.bc, (double)x[0], (double)x[1], (double)x[2], P[k][0], P[k][1], P[k][2]);
            }
        }
        // one pass = one matching, then thread 0's statistics and update; the first pass of a round is not an iteration
        int its = 0;
        auto pass = [&](bool first) __attribute__((always_inline)) {
            icp_match<PLANE>(L, P, m, rho2, inv_h, reach, mask, ctr, nrm);
            if (!first)
                ++its;
            if (tid == 0) {
                const double f = sums[0] / (double)m;
                const double e = sums[0] > 0.0 ? sqrt(sums[D2] / sums[0]) : 0.0;
                const bool converged = !first && fabs(fit - f) < rel_fit && fabs(rmse - e) < rel_rmse;
                fit = f;
                rmse = e;
                const bool cont = first ? rounds > 0 && max_it > 0 : !converged && its < max_it;
                L.bc[24] = cont ? 1.0 : 0.0;
                L.bc[25] = 0.0;
                if (cont && sums[0] > 0.0 && icp_estimate<PLANE>(sums, ctr, L.bc + 12)) {
                    icp_compose(L.bc + 12, L.bc);
                    L.bc[25] = 1.0;
                }
            }
            __syncthreads();
        };
        auto move = [&]() __attribute__((always_inline)) {
            if (L.bc[25] != 0.0) {
#pragma unroll
                for (int k = 0; k < ICP_PER_LANE; ++k)
                    icp_apply(L.bc + 12, P[k][0], P[k][1], P[k][2], P[k][0], P[k][1], P[k][2]);
            }
        };
        // The pass is expanded once for point to plane and twice for point to point, by measurement: the kernels are bound by
        // instruction fetch on one lane's path, and each is fastest in that form (profiles/notes_no_packed_fp32_build.md).
        if constexpr (PLANE) {
            for (bool first = true;; first = false) {
                pass(first);
                if (its >= max_it || L.bc[24] == 0.0)
                    break;
                move();
            }
        } else {
            pass(true);
            while (its < max_it && L.bc[24] != 0.0) {
                move();
                pass(false);
            }
        }
        if (tid == 0 && rounds > 0)
            it_out[(long long)c * rounds + r] = its;
        rho = rho * decay;
    }

    if (tid == 0) {
        double *To = T_out + 16LL * c;
        double T[12];
        if (PLANE && inverse)
            icp_invert(L.bc);
#pragma unroll
        for (int k = 0; k < 12; ++k)
            To[k] = T[k] = L.bc[k];
        To[12] = To[13] = To[14] = 0.0;
        To[15] = 1.0;
        const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
        icp_log_map(R, rot_out + 3LL * c);
        #pragma unroll
        for (int a = 0; a < 3; ++a)
            trans_out[3 * c + a] = (float)T[4 * a + 3];
        fit_out[c] = fit;
        rmse_out[c] = rmse;
    }
}

__global__ void f64_to_f32_kernel(long long n, const double *__restrict__ x, float *__restrict__ y)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        y[i] = (float)x[i];
}

}  // namespace

namespace {

// the argument checks and the launch shared by the two estimators
template <bool PLANE>
int icp_launch(const char *name, const double *tgt_normals, int inverse, int b, int m, const float *src,
               int src_point_stride, long long src_cloud_stride, int n, const float *dst, int dst_point_stride,
               long long dst_cloud_stride, const float *rot_axag, const float *trans, double radius, double decay,
               int rounds, int max_iteration, double relative_fitness, double relative_rmse, double *transform,
               double *rot_out, float *trans_out, double *fitness, double *rmse, int *iterations,
               cloudaae_stream_t stream)
{
    CLOUDAAE_REQUIRE(b >= 1 && m >= 1 && n >= 1, name, "b, m and n must be >= 1");
    CLOUDAAE_REQUIRE(m <= ICP_MAX_M, name, "m above the kernel's limit of 4096 source points per cloud");
    CLOUDAAE_REQUIRE(n <= ICP_MAX_N, name, "n above the kernel's limit of 4096 target points per cloud");
    CLOUDAAE_REQUIRE(rounds >= 0 && max_iteration >= 0, name, "rounds and max_iteration must be >= 0");
    CLOUDAAE_REQUIRE(radius > 0.0 && isfinite(radius), name, "radius must be a finite number > 0");
    CLOUDAAE_REQUIRE(decay > 0.0 && decay <= 1.0, name, "decay must lie in (0, 1]");
    CLOUDAAE_REQUIRE(relative_fitness == relative_fitness && relative_rmse == relative_rmse, name,
                     "relative_fitness and relative_rmse must not be NaN");
    CLOUDAAE_REQUIRE(src_point_stride >= 3 && dst_point_stride >= 3, name, "point strides must be >= 3 floats");
    CLOUDAAE_REQUIRE((b == 1 || src_cloud_stride >= (long long)(m - 1) * src_point_stride + 3) &&
                         (b == 1 || dst_cloud_stride >= (long long)(n - 1) * dst_point_stride + 3),
                     name, "cloud strides must not make clouds overlap");
    CLOUDAAE_REQUIRE(src && dst && rot_axag && trans && transform && rot_out && trans_out && fitness && rmse &&
                         (iterations || rounds == 0) && (tgt_normals || !PLANE),
                     name, "null pointer");
    constexpr int NS = PLANE ? ICP_PLANE_SUMS : ICP_SUMS;
    const int hbits = icp_hash_bits(n);
    const size_t lds = icp_lds_bytes(n, hbits, NS);
    const size_t max_lds = icp_lds_bytes(ICP_MAX_N, icp_hash_bits(ICP_MAX_N), NS);      // (n <= ICP_MAX_N: checked above)
    CLOUDAAE_CHECK_HIP(allow_dynamic_lds<icp_kernel<PLANE>>(lds, max_lds), name);
    hipLaunchKernelGGL(icp_kernel<PLANE>, dim3(b), dim3(ICP_THREADS), lds, (hipStream_t)stream, tgt_normals, inverse, m,
                       src, src_point_stride, src_cloud_stride, n, dst, dst_point_stride, dst_cloud_stride, rot_axag,
                       trans, radius, decay, rounds, max_iteration, relative_fitness, relative_rmse, hbits, transform,
                       rot_out, trans_out, fitness, rmse, iterations);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

CLOUDAAE_API int cloudaae_icp_point_to_point(int b, int m, const float *src, int src_point_stride,
                                             long long src_cloud_stride, int n, const float *dst, int dst_point_stride,
                                             long long dst_cloud_stride, const float *rot_axag, const float *trans,
                                             double radius, double decay, int rounds, int max_iteration,
                                             double relative_fitness, double relative_rmse, double *transform,
                                             double *rot_out, float *trans_out, double *fitness, double *rmse,
                                             int *iterations, cloudaae_stream_t stream)
{
    return icp_launch<false>("cloudaae_icp_point_to_point", nullptr, 0, b, m, src, src_point_stride, src_cloud_stride, n,
                             dst, dst_point_stride, dst_cloud_stride, rot_axag, trans, radius, decay, rounds,
                             max_iteration, relative_fitness, relative_rmse, transform, rot_out, trans_out, fitness,
                             rmse, iterations, stream);
}

CLOUDAAE_API int cloudaae_icp_point_to_plane(int b, int m, const float *src, int src_point_stride,
                                             long long src_cloud_stride, int n, const float *dst, int dst_point_stride,
                                             long long dst_cloud_stride, const double *tgt_normals,
                                             int pose_maps_target_to_source, const float *rot_axag, const float *trans,
                                             double radius, double decay, int rounds, int max_iteration,
                                             double relative_fitness, double relative_rmse, double *transform,
                                             double *rot_out, float *trans_out, double *fitness, double *rmse,
                                             int *iterations, cloudaae_stream_t stream)
{
    return icp_launch<true>("cloudaae_icp_point_to_plane", tgt_normals, pose_maps_target_to_source ? 1 : 0, b, m, src,
                            src_point_stride, src_cloud_stride, n, dst, dst_point_stride, dst_cloud_stride, rot_axag,
                            trans, radius, decay, rounds, max_iteration, relative_fitness, relative_rmse, transform,
                            rot_out, trans_out, fitness, rmse, iterations, stream);
}

CLOUDAAE_API int cloudaae_f64_to_f32(long long n, const double *x, float *y, cloudaae_stream_t stream)
{
    CLOUDAAE_REQUIRE(n >= 0, "cloudaae_f64_to_f32", "n must be >= 0");
    if (n == 0)
        return 0;
    CLOUDAAE_REQUIRE(x && y, "cloudaae_f64_to_f32", "null pointer");
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, n, x, y);
    CLOUDAAE_CHECK_LAUNCH("cloudaae_f64_to_f32");
    return 0;
}
