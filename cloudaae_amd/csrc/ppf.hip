// ppf.hip -- pose proposals by point-pair-feature voting: the pair table of the object models, the voting of a scene's
// point pairs for (model point, rotation about the normal) cells, and the greedy clustering of the voted poses.
// DESIGN.md, "Pose proposals", is the definition; tests/ppf_reference.py restates it in NumPy.  Everything is fp64 on
// fp32 points with + - * / sqrt only, un-fused (the library is compiled with -ffp-contract=off), products and sums in the
// written order.  No angle is formed: a quantity binned by angle is compared with a host-made table of bin-edge cosines,
// and the rotation of a peak comes from a host-made table of the bin centres' cosines and sines.  Votes are integers.
//
//   cloudaae_ppf_model_pairs   one launch, one wave per (set, reference point r): the key and the in-plane direction
//                              of every ordered pair (r, i) of the set.
//   cloudaae_ppf_vote          one launch, one workgroup of 256 threads per (sample, reference slot): an accumulator of
//                              m_max * n_alpha counters in dynamic LDS, one LDS atomic per (scene pair, table entry),
//                              then `peaks` block-wide maxima and their poses.  A wave deals the (point, entry) items
//                              of its 64 points to its lanes: buckets are too unequal for a lane to walk its own
//                              (profiles/notes_ppf.md).
//   cloudaae_ppf_cluster       one launch, one wave per sample: candidates in (votes, index) order join the first
//                              cluster near enough or found one; the `top` best clusters are written.
#include "common.h"
#include "pose_math.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

namespace cloudaae {

typedef unsigned long long u64;

constexpr int PPF_MAX_ANGLE = 64;                  // n_angle, and n_alpha / 2
constexpr int PPF_MAX_PEAKS = 4;
constexpr int PPF_MAX_TOP = 64;
constexpr int PPF_MAX_CANDIDATES = 4096;           // R * peaks of one sample in cloudaae_ppf_cluster
constexpr long long PPF_MAX_TOTAL = 1ll << 28;
// the accumulator's share of the 160 KiB of a workgroup; the rest holds the two edge tables and the reduction's slots
constexpr size_t PPF_VOTE_MAX_LDS = 158 * 1024;

// the bin of a cosine among n_edges + 1 equal angle bins over [0, pi]: how many of the (descending) edge cosines it does
// not exceed
__device__ __forceinline__ int ppf_bin(double c, const double *edges, int n_edges)
{
    int q = 0;
    for (int k = 0; k < n_edges; ++k)
        q += c <= edges[k] ? 1 : 0;
    return q;
}

// Q(n), row-major: the rotation that takes the unit vector n onto +x.  n_x >= 0: I + [v]x + [v]x^2 / (1 + n_x) with
// v = n x e_x, its first row written as n itself; n_x < 0: the half turn about z after Q(-n), so the divisor is never
// below 1.
__device__ __forceinline__ void ppf_frame(const double *n, double *Q)
{
    Q[0] = n[0];
    Q[1] = n[1];
    Q[2] = n[2];
    if (n[0] >= 0.0) {
        const double h = 1.0 + n[0], a = (n[1] * n[2]) / h;
        Q[3] = -n[1];
        Q[4] = 1.0 - (n[1] * n[1]) / h;
        Q[5] = -a;
        Q[6] = -n[2];
        Q[7] = -a;
        Q[8] = 1.0 - (n[2] * n[2]) / h;
    } else {
        const double h = 1.0 - n[0], a = (n[1] * n[2]) / h;
        Q[3] = -n[1];
        Q[4] = -(1.0 - (n[1] * n[1]) / h);
        Q[5] = a;
        Q[6] = n[2];
        Q[7] = -a;
        Q[8] = 1.0 - (n[2] * n[2]) / h;
    }
}

// The key of the oriented pair (p1, n1), (p2, n2), or -1 for a pair without one; d = p2 - p1 is left in d.
__device__ __forceinline__ int ppf_key(const double *p1, const double *n1, const double *p2, const double *n2, double dist_step,
                                       int n_dist, int n_angle, const double *edges, double *d)
{
    d[0] = p2[0] - p1[0];
    d[1] = p2[1] - p1[1];
    d[2] = p2[2] - p1[2];
    const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (!(len > 0.0))
        return -1;
    const double t = len / dist_step;
    if (!(t >= 0.0 && t < (double)n_dist))
        return -1;
    const int qd = (int)t;
    const double c1 = ((n1[0] * d[0] + n1[1] * d[1]) + n1[2] * d[2]) / len;
    const double c2 = ((n2[0] * d[0] + n2[1] * d[1]) + n2[2] * d[2]) / len;
    const double c3 = (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2];
    const int q1 = ppf_bin(c1, edges, n_angle - 1), q2 = ppf_bin(c2, edges, n_angle - 1), q3 = ppf_bin(c3, edges, n_angle - 1);
    return ((qd * n_angle + q1) * n_angle + q2) * n_angle + q3;
}

// the unit (y, z) part of Q d; false when it is zero
__device__ __forceinline__ bool ppf_direction(const double *Q, const double *d, double &uy, double &uz)
{
    const double y = (Q[3] * d[0] + Q[4] * d[1]) + Q[5] * d[2];
    const double z = (Q[6] * d[0] + Q[7] * d[1]) + Q[8] * d[2];
    const double r = sqrt(y * y + z * z);
    if (!(r > 0.0))
        return false;
    uy = y / r;
    uz = z / r;
    return true;
}

// ---- cloudaae_ppf_model_pairs ------------------------------------------------------------------------------------------
constexpr int MP_BLOCK = 64;

__global__ __launch_bounds__(MP_BLOCK) void ppf_model_pairs_kernel(int s, const int *__restrict__ offsets,
                                                                   const long long *__restrict__ pair_offsets, int m_total,
                                                                   long long n_pairs, const float *__restrict__ xyz,
                                                                   const double *__restrict__ normals,
                                                                   const double *__restrict__ dist_step, int n_dist, int n_angle,
                                                                   const double *__restrict__ cos_edges, int *__restrict__ key,
                                                                   int *__restrict__ ref, float *__restrict__ dir)
{
    __shared__ double edges[PPF_MAX_ANGLE];
    const int lane = threadIdx.x, g = blockIdx.x;
    if (lane < n_angle - 1)
        edges[lane] = cos_edges[lane];
    __syncthreads();
    // the set of point g: the last one that starts at or before it
    int lo = 0, hi = s;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    const int first = offsets[lo], last = offsets[lo + 1];
    if (first < 0 || last > m_total || g < first || g >= last)     // offsets that leave the points: nothing is written
        return;
    const int m = last - first, r = g - first;
    const long long base = pair_offsets[lo];
    if (base < 0 || base + (long long)m * m > n_pairs)
        return;
    const double step = dist_step[lo];
    double p1[3], n1[3], Q[9];
    for (int k = 0; k < 3; ++k) {
        p1[k] = (double)xyz[3ll * g + k];
        n1[k] = normals[3ll * g + k];
    }
    ppf_frame(n1, Q);
    for (int i = lane; i < m; i += MP_BLOCK) {
        const long long e = base + (long long)r * m + i;
        int k = -1;
        double uy = 0.0, uz = 0.0;
        if (i != r) {
            double p2[3], n2[3], d[3];
            for (int c = 0; c < 3; ++c) {
                p2[c] = (double)xyz[3ll * (first + i) + c];
                n2[c] = normals[3ll * (first + i) + c];
            }
            k = ppf_key(p1, n1, p2, n2, step, n_dist, n_angle, edges, d);
            if (k >= 0 && !ppf_direction(Q, d, uy, uz))
                k = -1;
            if (k < 0)
                uy = uz = 0.0;
        }
        key[e] = k;
        ref[e] = r;
        dir[2 * e] = (float)uy;
        dir[2 * e + 1] = (float)uz;
    }
}

// ---- cloudaae_ppf_vote -------------------------------------------------------------------------------------------------
constexpr int PV_BLOCK = 256;
constexpr int PV_WAVES = PV_BLOCK / 64;

struct PpfVoteArgs {
    int b, n, r_slots, ref_step, peaks, nclass, m_total, m_max, n_dist, n_angle, n_alpha, n_key;
    long long n_entries;
    const float *scene, *model_xyz, *entry_dir;
    const double *scene_normals, *model_normals, *dist_step, *cos_edges, *alpha_edges, *alpha_cs;
    const unsigned char *mask;
    const long long *class_id;
    const int *offsets, *bucket_start, *entry_ref;
    int *votes, *model_index, *bin, *acc;
    double *pose;
};

// one table entry's vote: the cell (its model point, the bin of alpha = alpha_scene - alpha_model)
__device__ __forceinline__ void ppf_cast(const PpfVoteArgs &a, int *acc, int m, long long e, double uy, double uz,
                                         const double *aedges, int half)
{
    const int rm = a.entry_ref[e];
    if ((unsigned)rm >= (unsigned)m)
        return;
    const double my = (double)a.entry_dir[2 * e], mz = (double)a.entry_dir[2 * e + 1];
    const double ca = uy * my + uz * mz, sa = uz * my - uy * mz;
    const int q = ppf_bin(ca, aedges, half - 1);
    const int bin = sa >= 0.0 ? half + q : half - 1 - q;
    __hip_atomic_fetch_add(acc + rm * a.n_alpha + bin, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The (point, entry) items of a wave's 64 points are numbered through by a prefix sum of the bucket lengths and dealt to
// the lanes 64 at a time, so a long bucket is walked by the whole wave and not by one lane while 63 wait; a lane finds its
// item's point by a binary search over the prefix sums (shuffles).
__global__ __launch_bounds__(PV_BLOCK) void ppf_vote_kernel(PpfVoteArgs a)
{
    extern __shared__ int acc[];
    __shared__ double edges[PPF_MAX_ANGLE], aedges[PPF_MAX_ANGLE];
    __shared__ u64 red[PV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int smp = blockIdx.x / a.r_slots, slot = blockIdx.x % a.r_slots;
    const int cells = a.m_max * a.n_alpha, half = a.n_alpha >> 1;
    for (int c = tid; c < cells; c += PV_BLOCK)
        acc[c] = 0;
    if (tid < a.n_angle - 1)
        edges[tid] = a.cos_edges[tid];
    if (tid < half - 1)
        aedges[tid] = a.alpha_edges[tid];

    // the class's model: anything that would leave the table is no model
    int first = 0, m = 0;
    const long long cls = a.class_id[smp];
    if (cls >= 0 && cls < a.nclass) {
        first = a.offsets[cls];
        const int last = a.offsets[cls + 1];
        m = last - first;
        if (first < 0 || last > a.m_total || m < 1 || m > a.m_max)
            m = 0;
    }
    // the reference point of this slot: usable point number slot * ref_step, counted by every wave for itself
    const unsigned char *mask = a.mask + (size_t)smp * a.n;
    const long long target = (long long)slot * a.ref_step;
    int ref_idx = -1;
    long long seen = 0;
    for (int base = 0; base < a.n; base += 64) {
        const int i = base + lane;
        const bool u = i < a.n && mask[i] != 0;
        const u64 bal = __ballot(u);
        const int c = __popcll(bal);
        if (target < seen + c) {
            const int rank = __popcll(bal & ((1ull << lane) - 1ull));
            const u64 hit = __ballot(u && rank == (int)(target - seen));
            ref_idx = base + (int)__ffsll((long long)hit) - 1;
            break;
        }
        seen += c;
    }
    __syncthreads();

    const float *scene = a.scene + (size_t)smp * a.n * 3;
    const double *snorm = a.scene_normals + (size_t)smp * a.n * 3;
    double pr[3] = {0.0, 0.0, 0.0}, nr[3] = {1.0, 0.0, 0.0}, Qs[9];
    const bool live = m > 0 && ref_idx >= 0;
    if (live) {
        for (int k = 0; k < 3; ++k) {
            pr[k] = (double)scene[3 * ref_idx + k];
            nr[k] = snorm[3 * ref_idx + k];
        }
    }
    ppf_frame(nr, Qs);
    if (live) {
        const double step = a.dist_step[cls];
        const int *bucket = a.bucket_start + (size_t)cls * (a.n_key + 1);
        for (int i0 = wv * 64; i0 < a.n; i0 += PV_BLOCK) {       // (wave-uniform) 64 points of the wave at a time
            const int i = i0 + lane;
            int lo = 0, len = 0;
            double uy = 0.0, uz = 0.0;
            if (i < a.n && i != ref_idx && mask[i] != 0) {
                double p2[3], n2[3], d[3];
                for (int k = 0; k < 3; ++k) {
                    p2[k] = (double)scene[3 * i + k];
                    n2[k] = snorm[3 * i + k];
                }
                const int key = ppf_key(pr, nr, p2, n2, step, a.n_dist, a.n_angle, edges, d);
                if (key >= 0 && ppf_direction(Qs, d, uy, uz)) {
                    // the bucket, clamped to the entry array
                    long long b0 = bucket[key], b1 = bucket[key + 1];
                    b0 = b0 < 0 ? 0 : b0;
                    b1 = b1 > a.n_entries ? a.n_entries : b1;
                    if (b1 > b0) {
                        lo = (int)b0;
                        len = (int)(b1 - b0);
                    }
                }
            }
            int inc = len;                                         // the inclusive prefix sum over the wave
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o, 64);
                if (lane >= o)
                    inc += t;
            }
            const int total = __shfl(inc, 63, 64), exc = inc - len;
            for (int base = 0; base < total; base += 64) {
                const int t = base + lane;
                int p = 0;                                         // the first lane whose inclusive sum exceeds t
#pragma unroll
                for (int s = 32; s > 0; s >>= 1)
                    if (__shfl(inc, p + s - 1, 64) <= t)
                        p += s;
                const int e = __shfl(lo, p, 64) + (t - __shfl(exc, p, 64));
                const double py = __shfl(uy, p, 64), pz = __shfl(uz, p, 64);
                if (t < total)
                    ppf_cast(a, acc, m, e, py, pz, aedges, half);
            }
        }
    }
    __syncthreads();
    if (a.acc) {
        int *out = a.acc + (size_t)blockIdx.x * cells;
        for (int c = tid; c < cells; c += PV_BLOCK)
            out[c] = acc[c];
    }
    // the peaks: the largest (votes, -cell) below the previous one, `peaks` times
    u64 prev = ~0ull;
    for (int k = 0; k < a.peaks; ++k) {
        u64 best = 0;
        for (int c = tid; c < cells; c += PV_BLOCK) {
            const u64 v = ((u64)(unsigned)acc[c] << 32) | (u64)(0xffffffffu - (unsigned)c);
            if (v < prev && v > best)
                best = v;
        }
        best = wave_max_u64(best);
        if (lane == 0)
            red[wv] = best;
        __syncthreads();
        best = red[0];
        for (int q = 1; q < PV_WAVES; ++q)
            best = red[q] > best ? red[q] : best;
        __syncthreads();                               // red is written again in the next round
        prev = best;
        if (tid == 0) {
            const size_t o = (size_t)blockIdx.x * a.peaks + k;
            const int v = (int)(best >> 32);
            const int cell = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
            double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
            int mi = -1, bn = -1;
            if (v > 0) {
                mi = cell / a.n_alpha;
                bn = cell % a.n_alpha;
                // T_s^-1 Rx(bin centre) T_m with T = [Q(n) | -Q(n) p]
                double pm[3], nm[3], Qm[9], A[9];
                for (int c = 0; c < 3; ++c) {
                    pm[c] = (double)a.model_xyz[3ll * (first + mi) + c];
                    nm[c] = a.model_normals[3ll * (first + mi) + c];
                }
                ppf_frame(nm, Qm);
                const double ca = a.alpha_cs[2 * bn], sa = a.alpha_cs[2 * bn + 1];
                for (int c = 0; c < 3; ++c) {
                    A[c] = Qm[c];
                    A[3 + c] = ca * Qm[3 + c] - sa * Qm[6 + c];
                    A[6 + c] = sa * Qm[3 + c] + ca * Qm[6 + c];
                }
                for (int i = 0; i < 3; ++i) {
                    for (int c = 0; c < 3; ++c)
                        T[4 * i + c] = (Qs[i] * A[c] + Qs[3 + i] * A[3 + c]) + Qs[6 + i] * A[6 + c];
                    T[4 * i + 3] = pr[i] - ((T[4 * i] * pm[0] + T[4 * i + 1] * pm[1]) + T[4 * i + 2] * pm[2]);
                }
            }
            a.votes[o] = v;
            a.model_index[o] = mi;
            a.bin[o] = bn;
            double *po = a.pose + 16 * o;
            for (int c = 0; c < 12; ++c)
                po[c] = T[c];
            po[12] = po[13] = po[14] = 0.0;
            po[15] = 1.0;
        }
    }
}

// ---- cloudaae_ppf_cluster ----------------------------------------------------------------------------------------------
constexpr int PC_BLOCK = 64;

__global__ __launch_bounds__(PC_BLOCK) void ppf_cluster_kernel(int c, const int *__restrict__ votes, const double *__restrict__ pose,
                                                               const long long *__restrict__ class_id, int nclass,
                                                               const double *__restrict__ trans_thresh2, double rot_bound, int top,
                                                               double *__restrict__ pose_out, double *__restrict__ rot_axag,
                                                               float *__restrict__ trans, int *__restrict__ score,
                                                               int *__restrict__ valid)
{
    __shared__ int s_votes[PPF_MAX_CANDIDATES], s_rep[PPF_MAX_CANDIDATES], s_score[PPF_MAX_CANDIDATES];
    const int lane = threadIdx.x, smp = blockIdx.x;
    const int *v_in = votes + (size_t)smp * c;
    const double *poses = pose + (size_t)smp * c * 16;
    for (int i = lane; i < c; i += PC_BLOCK)
        s_votes[i] = v_in[i];
    __syncthreads();
    const long long cls = class_id[smp];
    const bool known = cls >= 0 && cls < nclass;
    const double tt2 = known ? trans_thresh2[cls] : 0.0;
    int n_cl = 0;
    u64 prev = ~0ull;
    while (known) {
        // the next candidate by (votes descending, index ascending); one without votes ends the list
        u64 best = 0;
        for (int i = lane; i < c; i += PC_BLOCK) {
            const int v = s_votes[i];
            const u64 k = ((u64)(unsigned)(v > 0 ? v : 0) << 32) | (u64)(0xffffffffu - (unsigned)i);
            if (v > 0 && k < prev && k > best)
                best = k;
        }
        best = wave_max_u64(best);
        if (best == 0)
            break;
        prev = best;
        const int v = (int)(best >> 32), idx = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
        const double *Tb = poses + 16ll * idx;
        int found = -1;
        for (int base = 0; base < n_cl && found < 0; base += PC_BLOCK) {
            const int k = base + lane;
            bool ok = false;
            if (k < n_cl) {
                const double *Ta = poses + 16ll * s_rep[k];
                const double dx = Ta[3] - Tb[3], dy = Ta[7] - Tb[7], dz = Ta[11] - Tb[11];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const double r0 = (Ta[0] * Tb[0] + Ta[1] * Tb[1]) + Ta[2] * Tb[2];
                const double r1 = (Ta[4] * Tb[4] + Ta[5] * Tb[5]) + Ta[6] * Tb[6];
                const double r2 = (Ta[8] * Tb[8] + Ta[9] * Tb[9]) + Ta[10] * Tb[10];
                ok = d2 <= tt2 && (r0 + r1) + r2 >= rot_bound;
            }
            const u64 bal = __ballot(ok);
            if (bal)
                found = base + (int)__ffsll((long long)bal) - 1;
        }
        if (lane == 0) {
            if (found >= 0) {
                s_score[found] += v;
            } else {
                s_rep[n_cl] = idx;
                s_score[n_cl] = v;
            }
        }
        if (found < 0)
            ++n_cl;
        __syncthreads();
    }
    // the `top` best clusters by (score descending, founding order ascending)
    prev = ~0ull;
    for (int t = 0; t < top; ++t) {
        u64 best = 0;
        for (int k = lane; k < n_cl; k += PC_BLOCK) {
            const u64 key = ((u64)(unsigned)s_score[k] << 32) | (u64)(0xffffffffu - (unsigned)k);
            if (key < prev && key > best)
                best = key;
        }
        best = wave_max_u64(best);
        if (best != 0)
            prev = best;
        if (lane == 0) {
            const size_t o = (size_t)smp * top + t;
            double T[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
            int sc = 0;
            if (best != 0) {
                const int k = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
                sc = (int)(best >> 32);
                const double *src = poses + 16ll * s_rep[k];
                for (int q = 0; q < 16; ++q)
                    T[q] = src[q];
            }
            double R[9], r[3];
            for (int i = 0; i < 3; ++i)
                for (int q = 0; q < 3; ++q)
                    R[3 * i + q] = T[4 * i + q];
            icp_log_map(R, r);
            for (int q = 0; q < 16; ++q)
                pose_out[16 * o + q] = T[q];
            for (int q = 0; q < 3; ++q) {
                rot_axag[3 * o + q] = r[q];
                trans[3 * o + q] = (float)T[4 * q + 3];
            }
            score[o] = sc;
            valid[o] = best != 0 ? 1 : 0;
        }
    }
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_ppf_model_pairs(int s, const int *offsets, const long long *pair_offsets, int m_total, long long n_pairs,
                                          const float *xyz, const double *normals, const double *dist_step, int n_dist,
                                          int n_angle, const double *cos_edges, int *key, int *ref, float *dir,
                                          cloudaae_stream_t stream)
{
    const char *name = "cloudaae_ppf_model_pairs";
    CLOUDAAE_REQUIRE(s >= 1 && s <= (1 << 20) && m_total >= 1 && m_total <= (1 << 24), name,
                     "s must lie in [1, 2^20] and m_total in [1, 2^24]");
    CLOUDAAE_REQUIRE(n_pairs >= 1 && n_pairs <= PPF_MAX_TOTAL, name, "n_pairs must lie in [1, 2^28]");
    CLOUDAAE_REQUIRE(n_dist >= 1 && n_angle >= 1 && n_angle <= PPF_MAX_ANGLE &&
                     (long long)n_dist * n_angle * n_angle * n_angle <= (1ll << 24), name,
                     "n_dist >= 1, n_angle in [1, 64] and n_dist * n_angle^3 <= 2^24");
    CLOUDAAE_REQUIRE(offsets && pair_offsets && xyz && normals && dist_step && cos_edges && key && ref && dir, name, "null pointer");
    hipLaunchKernelGGL(ppf_model_pairs_kernel, dim3(m_total), dim3(MP_BLOCK), 0, (hipStream_t)stream, s, offsets, pair_offsets,
                       m_total, n_pairs, xyz, normals, dist_step, n_dist, n_angle, cos_edges, key, ref, dir);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_ppf_vote(int b, int n, const float *scene, const double *scene_normals, const uint8_t *mask,
                                   const long long *class_id, int ref_step, int peaks, int nclass, const int *offsets, int m_total,
                                   int m_max, const float *model_xyz, const double *model_normals, const double *dist_step,
                                   int n_dist, int n_angle, int n_alpha, const double *cos_edges, const double *alpha_edges,
                                   const double *alpha_cs, const int *bucket_start, long long n_entries, const int *entry_ref,
                                   const float *entry_dir, int *votes, int *model_index, int *bin, double *pose, int *acc,
                                   cloudaae_stream_t stream)
{
    const char *name = "cloudaae_ppf_vote";
    CLOUDAAE_REQUIRE(b >= 1 && n >= 2 && n <= (1 << 20) && ref_step >= 1 && ref_step <= n, name,
                     "b >= 1, n in [2, 2^20] and ref_step in [1, n]");
    CLOUDAAE_REQUIRE(peaks >= 1 && peaks <= PPF_MAX_PEAKS, name, "peaks must lie in [1, 4]");
    CLOUDAAE_REQUIRE(nclass >= 1 && m_total >= 1 && m_total <= (1 << 24) && m_max >= 1 && m_max <= m_total, name,
                     "nclass >= 1, m_total in [1, 2^24] and m_max in [1, m_total]");
    CLOUDAAE_REQUIRE(n_dist >= 1 && n_angle >= 1 && n_angle <= PPF_MAX_ANGLE &&
                     (long long)n_dist * n_angle * n_angle * n_angle <= (1ll << 24), name,
                     "n_dist >= 1, n_angle in [1, 64] and n_dist * n_angle^3 <= 2^24");
    CLOUDAAE_REQUIRE(n_alpha >= 2 && n_alpha % 2 == 0 && n_alpha <= 2 * PPF_MAX_ANGLE, name, "n_alpha must be even, in [2, 128]");
    CLOUDAAE_REQUIRE((long long)m_max * n_alpha >= peaks, name, "fewer cells than peaks");
    CLOUDAAE_REQUIRE(n_entries >= 0 && n_entries <= PPF_MAX_TOTAL, name, "n_entries must lie in [0, 2^28]");
    const int r_slots = ceil_div(n, ref_step);
    CLOUDAAE_REQUIRE((long long)b * r_slots <= (1ll << 24), name, "b * ceil(n / ref_step) above 2^24");
    CLOUDAAE_REQUIRE(scene && scene_normals && mask && class_id && offsets && model_xyz && model_normals && dist_step &&
                     cos_edges && alpha_edges && alpha_cs && bucket_start && votes && model_index && bin && pose, name,
                     "null pointer");
    CLOUDAAE_REQUIRE((entry_ref && entry_dir) || n_entries == 0, name, "the entries are null with n_entries > 0");
    const size_t lds = sizeof(int) * (size_t)m_max * n_alpha;
    CLOUDAAE_REQUIRE(lds <= PPF_VOTE_MAX_LDS, name,
                     "the accumulator of m_max * n_alpha counters does not fit the workgroup's LDS (158 KiB of the 160)");
    PpfVoteArgs a;
    a.b = b, a.n = n, a.r_slots = r_slots, a.ref_step = ref_step, a.peaks = peaks, a.nclass = nclass, a.m_total = m_total;
    a.m_max = m_max, a.n_dist = n_dist, a.n_angle = n_angle, a.n_alpha = n_alpha, a.n_key = n_dist * n_angle * n_angle * n_angle;
    a.n_entries = n_entries;
    a.scene = scene, a.model_xyz = model_xyz, a.entry_dir = entry_dir;
    a.scene_normals = scene_normals, a.model_normals = model_normals, a.dist_step = dist_step, a.cos_edges = cos_edges;
    a.alpha_edges = alpha_edges, a.alpha_cs = alpha_cs;
    a.mask = mask, a.class_id = class_id, a.offsets = offsets, a.bucket_start = bucket_start, a.entry_ref = entry_ref;
    a.votes = votes, a.model_index = model_index, a.bin = bin, a.acc = acc, a.pose = pose;
    CLOUDAAE_CHECK_HIP(allow_dynamic_lds<ppf_vote_kernel>(lds, PPF_VOTE_MAX_LDS), name);
    hipLaunchKernelGGL(ppf_vote_kernel, dim3((unsigned)(b * r_slots)), dim3(PV_BLOCK), lds, (hipStream_t)stream, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_ppf_cluster(int b, int c, const int *votes, const double *pose, const long long *class_id, int nclass,
                                      const double *trans_thresh2, double rot_bound, int top, double *pose_out, double *rot_axag,
                                      float *trans, int *score, int *valid, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_ppf_cluster";
    CLOUDAAE_REQUIRE(b >= 1 && b <= (1 << 24) && c >= 1 && c <= PPF_MAX_CANDIDATES, name,
                     "b must lie in [1, 2^24] and c (candidates per sample) in [1, 4096]");
    CLOUDAAE_REQUIRE(top >= 1 && top <= PPF_MAX_TOP && nclass >= 1, name, "top must lie in [1, 64] and nclass be >= 1");
    CLOUDAAE_REQUIRE(rot_bound == rot_bound, name, "rot_bound is not a number");
    CLOUDAAE_REQUIRE(votes && pose && class_id && trans_thresh2 && pose_out && rot_axag && trans && score && valid, name,
                     "null pointer");
    hipLaunchKernelGGL(ppf_cluster_kernel, dim3(b), dim3(PC_BLOCK), 0, (hipStream_t)stream, c, votes, pose, class_id, nclass,
                       trans_thresh2, rot_bound, top, pose_out, rot_axag, trans, score, valid);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
