// depth_components.hip -- object candidates from unlabelled depth frames on the GPU (gfx950): the dominant support plane
// by hypothesis voting, the foreground that stands on it, the connected components of the foreground in the depth image
// and their ordered table as a label image in the convention of segment.hip (0 = none, component k = value k + 1).
// DESIGN.md, "Depth components", is the definition; tests/depth_components_reference.py restates it in NumPy.  Every
// output is an integer, or a double copied from one hypothesis, and a pure function of the input: integer atomics only,
// and the launch boundaries are the only synchronisation between workgroups -- no kernel waits for another workgroup.
// The back-projection is that of segment.hip in fp32, un-fused (the file is compiled with -ffp-contract=off); everything
// after it is double with + - * in the written order.
//
//   cloudaae_depth_plane       a memset and two launches: the inlier counts (a workgroup takes a run of tested pixels and a
//                              block of hypotheses; ballot + popcount per wave, one atomic per workgroup and hypothesis),
//                              then one wave per frame that picks the winner and writes its plane
//   cloudaae_depth_foreground  one launch, one lane per pixel
//   cloudaae_depth_components  a memset and three launches: (a) a workgroup labels its 32 x 32 tile by union-find in LDS
//                              and writes each pixel's tile root as a frame pixel index; (b) one lane per joined pixel
//                              pair across a tile border unites the two roots in global memory (atomicMin union-find, every
//                              access of a label word an agent-scope atomic); (c) every pixel walks to its final root
//   cloudaae_component_labels  memsets and four launches: sizes (one atomic per run of equal roots in a wave), the list
//                              of candidates, one workgroup per frame that picks the first K by (size descending, root
//                              ascending), then the label image and the boxes (LDS atomics, then one global atomic per
//                              workgroup, component and box side)
//
// Every device loop has a bound: a walk along label words ends after as many steps as the tile or the frame has pixels
// (labels only ever decrease along a walk, so a correct walk is shorter) and sets a bit of the frame's status otherwise.
#include "common.h"
#include "depth_frame.h"
#include "philox.h"
#include "workspace.h"
#include "../../include/cloudaae_hip.h"

namespace cloudaae {

typedef unsigned long long u64;

constexpr int DC_BLOCK = 256;
constexpr int DC_WAVES = DC_BLOCK / 64;
constexpr unsigned DC_STREAM_PLANE = 25u;          // r0..r2 of counter ((first_frame + f) << 20) | h: the three pixels
constexpr int DC_MAX_HYP = 4096;
constexpr long long DC_MAX_FIRST_FRAME = 1ll << 40;
constexpr int DC_MAX_COMPONENTS = 254;
constexpr int DC_HB = 8;                           // hypotheses per workgroup of the count
constexpr int DC_PASSES = 4;                       // tested pixels per lane of the count
constexpr int DC_RUN = DC_BLOCK * DC_PASSES;       // tested pixels per workgroup of the count
constexpr int DC_TW = 32, DC_TH = 32;              // the tile of the component labelling
constexpr int DC_TILE = DC_TW * DC_TH;
constexpr int DC_TILE_PASSES = DC_TILE / DC_BLOCK;
constexpr int DC_STATUS_TILE = 1, DC_STATUS_SEAM = 2, DC_STATUS_FLATTEN = 4;

// pixel p of frame fr, back-projected in fp32 as the frame segments are, then widened
__device__ __forceinline__ void dc_point(const float *intrinsics, int fr, int w, int p, unsigned short d, double &x, double &y,
                                         double &z)
{
    float q[3];
    backproject(pinhole<float>(intrinsics + 5 * (size_t)fr), p % w, p / w, d, q);
    x = (double)q[0], y = (double)q[1], z = (double)q[2];
}

struct DcPlane {
    double nx, ny, nz, d, q;                       // q = -1 for a void hypothesis (n = d = 0): the count skips it
};

// hypothesis h of frame fr
__device__ __forceinline__ DcPlane dc_hypothesis(const unsigned short *depth, const float *intrinsics, int fr, int h, int w,
                                                 u64 seed, long long first_frame, int hyp)
{
    DcPlane pl;
    pl.nx = pl.ny = pl.nz = pl.d = 0.0;
    pl.q = -1.0;
    unsigned r[4];
    philox4x32(seed, ((u64)(first_frame + fr) << 20) | (u64)hyp, DC_STREAM_PLANE, r);
    const u64 hw = (u64)h * (u64)w;
    const unsigned short *df = depth + (size_t)fr * hw;
    double px[3], py[3], pz[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = (int)(((u64)r[k] * hw) >> 32);
        const unsigned short dv = df[p];
        ok = ok && dv != 0;
        dc_point(intrinsics, fr, w, p, dv, px[k], py[k], pz[k]);
    }
    if (!ok)
        return pl;
    const double e1x = px[1] - px[0], e1y = py[1] - py[0], e1z = pz[1] - pz[0];
    const double e2x = px[2] - px[0], e2y = py[2] - py[0], e2z = pz[2] - pz[0];
    double nx = e1y * e2z - e1z * e2y;
    double ny = e1z * e2x - e1x * e2z;
    double nz = e1x * e2y - e1y * e2x;
    const double q = (nx * nx + ny * ny) + nz * nz;
    if (!(q > 0.0))
        return pl;
    double d = -((nx * px[0] + ny * py[0]) + nz * pz[0]);
    if (d < 0.0)
        nx = -nx, ny = -ny, nz = -nz, d = -d;
    pl.nx = nx, pl.ny = ny, pl.nz = nz, pl.d = d, pl.q = q;
    return pl;
}

struct DpArgs {
    int f, h, w, n_hyp, stride, hs, ws, runs, hyp_blocks, min_plane_percent;
    const unsigned short *depth;
    const float *intrinsics;
    u64 seed;
    long long first_frame;
    double tol2;
    int *count, *tested, *plane_hyp;
    double *plane;
};

// grid = f * runs * hyp_blocks: workgroup b takes hypothesis block b % hyp_blocks and run (b / hyp_blocks) % runs of the
// tested pixels of frame b / (hyp_blocks * runs); the workgroups of hypothesis block 0 also count the tested pixels
__global__ __launch_bounds__(DC_BLOCK) void depth_plane_count_kernel(DpArgs a)
{
    __shared__ double hyp[DC_HB][5];
    __shared__ int total[DC_HB + 1];
    const int hb = blockIdx.x % a.hyp_blocks;
    const int run = (blockIdx.x / a.hyp_blocks) % a.runs;
    const int fr = blockIdx.x / (a.hyp_blocks * a.runs);
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < DC_HB) {
        const int hy = hb * DC_HB + tid;
        DcPlane pl;
        pl.nx = pl.ny = pl.nz = pl.d = 0.0, pl.q = -1.0;
        if (hy < a.n_hyp)
            pl = dc_hypothesis(a.depth, a.intrinsics, fr, a.h, a.w, a.seed, a.first_frame, hy);
        hyp[tid][0] = pl.nx, hyp[tid][1] = pl.ny, hyp[tid][2] = pl.nz, hyp[tid][3] = pl.d, hyp[tid][4] = pl.q;
    }
    if (tid <= DC_HB)
        total[tid] = 0;
    __syncthreads();
    double x[DC_PASSES], y[DC_PASSES], z[DC_PASSES];
    bool valid[DC_PASSES];
    int n_valid = 0;
    const int cells = a.hs * a.ws;
#pragma unroll
    for (int pass = 0; pass < DC_PASSES; ++pass) {
        const int c = run * DC_RUN + pass * DC_BLOCK + tid;
        valid[pass] = false;
        x[pass] = y[pass] = z[pass] = 0.0;
        if (c < cells) {
            const int p = (c / a.ws) * a.stride * a.w + (c % a.ws) * a.stride;   // v = (c / ws) stride < h, u < w
            const unsigned short dv = a.depth[(size_t)fr * ((size_t)a.h * a.w) + p];
            valid[pass] = dv != 0;
            dc_point(a.intrinsics, fr, a.w, p, dv, x[pass], y[pass], z[pass]);
        }
        n_valid += wave_count(valid[pass]);
    }
    if (hb == 0 && lane == 0 && n_valid)
        atomicAdd(&total[DC_HB], n_valid);
#pragma unroll 1
    for (int j = 0; j < DC_HB; ++j) {
        const double nx = hyp[j][0], ny = hyp[j][1], nz = hyp[j][2], d = hyp[j][3], bound = a.tol2 * hyp[j][4];
        const bool live = hyp[j][4] > 0.0;         // (not by the bound's sign: with tol = 0 a void one has 0 <= -0)
        int n = 0;
#pragma unroll
        for (int pass = 0; pass < DC_PASSES; ++pass) {
            const double s = ((nx * x[pass] + ny * y[pass]) + nz * z[pass]) + d;
            n += wave_count(live && valid[pass] && s * s <= bound);
        }
        if (lane == 0 && n)
            atomicAdd(&total[j], n);
    }
    __syncthreads();
    if (tid < DC_HB) {
        const int hy = hb * DC_HB + tid;
        if (hy < a.n_hyp && total[tid])
            atomicAdd(&a.count[(size_t)fr * a.n_hyp + hy], total[tid]);
    }
    if (tid == DC_HB && hb == 0 && total[DC_HB])
        atomicAdd(&a.tested[fr], total[DC_HB]);
}

// grid = f, one wave: the largest count, ties to the lowest hypothesis; the plane of the winner, formed again
__global__ __launch_bounds__(64) void depth_plane_winner_kernel(DpArgs a)
{
    const int fr = blockIdx.x, lane = threadIdx.x;
    u64 best = 0;                                  // (count << 12) | (4095 - h): the largest wins
    for (int hy = lane; hy < a.n_hyp; hy += 64) {
        const u64 key = ((u64)(unsigned)a.count[(size_t)fr * a.n_hyp + hy] << 12) | (u64)(DC_MAX_HYP - 1 - hy);
        best = key > best ? key : best;
    }
    best = wave_max_u64(best);
    if (lane != 0)
        return;
    const long long cnt = (long long)(best >> 12);
    const int hy = DC_MAX_HYP - 1 - (int)(best & (u64)(DC_MAX_HYP - 1));
    const long long tested = a.tested[fr];
    double *out = a.plane + 4 * (size_t)fr;
    if (cnt >= 3 && cnt * 100 >= (long long)a.min_plane_percent * tested) {
        const DcPlane pl = dc_hypothesis(a.depth, a.intrinsics, fr, a.h, a.w, a.seed, a.first_frame, hy);
        out[0] = pl.nx, out[1] = pl.ny, out[2] = pl.nz, out[3] = pl.d;
        a.plane_hyp[fr] = hy;
    } else {
        out[0] = out[1] = out[2] = out[3] = 0.0;
        a.plane_hyp[fr] = -1;
    }
}

// one lane per pixel of the batch
__global__ __launch_bounds__(DC_BLOCK) void depth_foreground_kernel(int f, int h, int w, const unsigned short *depth,
                                                                    const float *intrinsics, const double *plane,
                                                                    const int *plane_hyp, double tol2, double height2,
                                                                    unsigned char *fg)
{
    const long long hw = (long long)h * w;
    const long long g = (long long)blockIdx.x * DC_BLOCK + threadIdx.x;
    if (g >= (long long)f * hw)
        return;
    const int fr = (int)(g / hw), p = (int)(g % hw);
    const unsigned short dv = depth[g];
    bool on = dv != 0;
    if (on && plane_hyp[fr] >= 0) {
        const double nx = plane[4 * (size_t)fr], ny = plane[4 * (size_t)fr + 1], nz = plane[4 * (size_t)fr + 2];
        const double d = plane[4 * (size_t)fr + 3];
        const double q = (nx * nx + ny * ny) + nz * nz;
        double x, y, z;
        dc_point(intrinsics, fr, w, p, dv, x, y, z);
        const double s = ((nx * x + ny * y) + nz * z) + d;
        const double s2 = s * s;
        on = s > 0.0 && s2 > tol2 * q && s2 <= height2 * q;
    }
    fg[g] = on ? 1 : 0;
}

// ---- connected components ---------------------------------------------------------------------------------------------------

// Unites the sets of a and b in the label words lab (a word holds an index of its own set that is not above its own; a root
// holds itself).  The larger of the two is hung below the smaller with atomicMin; when it was no root any more, the union
// goes on from what it pointed to.  max(a, b) falls with every round, so a correct run ends within `bound` rounds; false
// when it did not.  Every access is an atomic of scope SCOPE: other lanes (LDS) or workgroups (global) write the words.
template <int SCOPE>
__device__ __forceinline__ bool dc_unite(int *lab, int a, int b, int bound)
{
    for (int step = 0; step <= bound; ++step) {
        if (a == b)
            return true;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a)
            return true;
        a = old;
    }
    return false;
}

// the root above a, at most `bound` steps away; -1 when the walk did not end
template <int SCOPE>
__device__ __forceinline__ int dc_find(int *lab, int a, int bound)
{
    for (int step = 0; step <= bound; ++step) {
        const int up = __hip_atomic_load(lab + a, __ATOMIC_RELAXED, SCOPE);
        if (up == a)
            return a;
        a = up;
    }
    return -1;
}

struct DccArgs {
    int f, h, w, tx, ty, nv, nh;                   // tiles across and down; seam pairs per frame, vertical and horizontal
    const unsigned short *depth;
    const unsigned char *fg;
    const int *jump_units;
    int *lab;                                      // workspace [f, h w]
    int *root, *status;
};

__device__ __forceinline__ bool dc_joined(int da, int db, int jump)
{
    const int diff = da > db ? da - db : db - da;
    return diff <= jump;
}

// grid = f * tx * ty: (a) the tile's components by union-find in LDS, written as frame pixel indices.  The tile order of
// two pixels is their frame order, so the smallest tile index of a component is its smallest frame index.
__global__ __launch_bounds__(DC_BLOCK) void depth_components_tile_kernel(DccArgs a)
{
    __shared__ int lab[DC_TILE];
    __shared__ unsigned short dep[DC_TILE];
    const int tiles = a.tx * a.ty;
    const int fr = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int x0 = (t % a.tx) * DC_TW, y0 = (t / a.tx) * DC_TH;
    const int tid = threadIdx.x;
    const size_t base = (size_t)fr * ((size_t)a.h * a.w);
    const int jump = a.jump_units[fr];
#pragma unroll
    for (int pass = 0; pass < DC_TILE_PASSES; ++pass) {
        const int l = pass * DC_BLOCK + tid;
        const int x = x0 + l % DC_TW, y = y0 + l / DC_TW;
        bool on = false;
        unsigned short dv = 0;
        if (x < a.w && y < a.h) {
            const size_t i = base + (size_t)y * a.w + x;
            on = a.fg[i] != 0;
            dv = a.depth[i];
        }
        lab[l] = on ? l : -1;
        dep[l] = dv;
    }
    __syncthreads();
    bool fine = true;
#pragma unroll
    for (int pass = 0; pass < DC_TILE_PASSES; ++pass) {
        const int l = pass * DC_BLOCK + tid;
        const int lx = l % DC_TW, ly = l / DC_TW;
        // (a pixel outside the frame is background: its word is -1 and never a partner)
        const bool on = __hip_atomic_load(lab + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0;
        if (!on)
            continue;
        if (lx + 1 < DC_TW && x0 + lx + 1 < a.w && y0 + ly < a.h &&
            __hip_atomic_load(lab + l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0 &&
            dc_joined(dep[l], dep[l + 1], jump))
            fine = dc_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l, l + 1, DC_TILE) && fine;
        if (ly + 1 < DC_TH && y0 + ly + 1 < a.h && x0 + lx < a.w &&
            __hip_atomic_load(lab + l + DC_TW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0 &&
            dc_joined(dep[l], dep[l + DC_TW], jump))
            fine = dc_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l, l + DC_TW, DC_TILE) && fine;
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < DC_TILE_PASSES; ++pass) {
        const int l = pass * DC_BLOCK + tid;
        const int x = x0 + l % DC_TW, y = y0 + l / DC_TW;
        if (x >= a.w || y >= a.h)
            continue;
        int out = -1;
        if (lab[l] >= 0) {
            int r = l;                             // (nothing writes lab any more: plain reads)
            int step = 0;
            for (; step <= DC_TILE && lab[r] != r; ++step)
                r = lab[r];
            if (step > DC_TILE)
                fine = false, r = l;
            out = (y0 + r / DC_TW) * a.w + x0 + r % DC_TW;
        }
        a.lab[base + (size_t)y * a.w + x] = out;
    }
    if (!fine)
        atomicOr(&a.status[fr], DC_STATUS_TILE);
}

// grid = ceil(f (nv + nh) / 256): (b) one lane per pixel pair across a tile border.  Pair s < nv of a frame is row s % h of
// vertical border s / h (between columns 32 (s / h + 1) - 1 and the next); the others are column (s - nv) % w of a
// horizontal border.  The label words are written by other workgroups meanwhile: agent-scope atomics only.
__global__ __launch_bounds__(DC_BLOCK) void depth_components_seam_kernel(DccArgs a)
{
    const long long per = (long long)a.nv + a.nh;
    const long long g = (long long)blockIdx.x * DC_BLOCK + threadIdx.x;
    if (g >= (long long)a.f * per)
        return;
    const int fr = (int)(g / per), s = (int)(g % per);
    int pa, pb;
    if (s < a.nv) {
        const int x = (s / a.h + 1) * DC_TW, y = s % a.h;          // 1 <= x <= (tx - 1) 32 < w
        pa = y * a.w + x - 1, pb = pa + 1;
    } else {
        const int y = ((s - a.nv) / a.w + 1) * DC_TH, x = (s - a.nv) % a.w;
        pa = (y - 1) * a.w + x, pb = pa + a.w;
    }
    const int hw = a.h * a.w;
    const size_t base = (size_t)fr * (size_t)hw;
    if (!a.fg[base + pa] || !a.fg[base + pb] || !dc_joined(a.depth[base + pa], a.depth[base + pb], a.jump_units[fr]))
        return;
    int *lab = a.lab + base;
    const int ra = dc_find<__HIP_MEMORY_SCOPE_AGENT>(lab, pa, hw);
    const int rb = dc_find<__HIP_MEMORY_SCOPE_AGENT>(lab, pb, hw);
    // (a word of a foreground pixel holds an index in [0, h w) of a foreground pixel: every walk stays inside the frame)
    if (ra < 0 || rb < 0 || !dc_unite<__HIP_MEMORY_SCOPE_AGENT>(lab, ra, rb, hw))
        atomicOr(&a.status[fr], DC_STATUS_SEAM);
}

// one lane per pixel of the batch: (c) the final root; the label words are read plainly, the launch before wrote them
__global__ __launch_bounds__(DC_BLOCK) void depth_components_flatten_kernel(DccArgs a)
{
    const int hw = a.h * a.w;
    const long long g = (long long)blockIdx.x * DC_BLOCK + threadIdx.x;
    if (g >= (long long)a.f * hw)
        return;
    const int fr = (int)(g / hw);
    const int *lab = a.lab + (size_t)fr * (size_t)hw;
    int r = lab[g % hw];
    if (r >= 0) {
        int step = 0;
        for (; step <= hw; ++step) {
            const int up = lab[r];
            if (up == r)
                break;
            r = up;
        }
        if (step > hw) {
            atomicOr(&a.status[fr], DC_STATUS_FLATTEN);
            r = (int)(g % hw);
        }
    }
    a.root[g] = r;
}

// ---- the component table --------------------------------------------------------------------------------------------------------

struct ClArgs {
    int f, h, w, min_pixels, max_components;
    const int *root;
    int *size, *rank, *cand, *ncand;               // workspace: [f, h w] each, [f]
    unsigned char *label;
    int *n_components, *n_candidates, *comp_root, *comp_size, *comp_box;
};

// a root the table may trust: a pixel of its own frame
__device__ __forceinline__ bool cl_root_ok(int r, int hw) { return r >= 0 && r < hw; }

// one lane per pixel: size[root] += 1, one atomic per run of equal roots among the consecutive pixels of a wave
__global__ __launch_bounds__(DC_BLOCK) void component_size_kernel(ClArgs a)
{
    const int hw = a.h * a.w;
    const long long total = (long long)a.f * hw;
    const long long g = (long long)blockIdx.x * DC_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    long long key = -1;                            // (frame, root) as one index into size, -1: none
    if (g < total) {
        const int r = a.root[g];
        if (cl_root_ok(r, hw))
            key = (g / hw) * hw + r;
    }
    const long long before = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || key != before;
    const u64 heads = __builtin_amdgcn_ballot_w64(head);
    if (head && key >= 0) {
        const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = above ? __builtin_ctzll(above) + 1 : 64 - lane;
        atomicAdd(&a.size[key], len);
    }
}

// one lane per pixel: the roots of at least min_pixels pixels, in no particular order
__global__ __launch_bounds__(DC_BLOCK) void component_candidates_kernel(ClArgs a)
{
    const int hw = a.h * a.w;
    const long long g = (long long)blockIdx.x * DC_BLOCK + threadIdx.x;
    if (g >= (long long)a.f * hw)
        return;
    const int fr = (int)(g / hw), p = (int)(g % hw);
    if (a.root[g] != p || a.size[g] < a.min_pixels)
        return;
    const int slot = atomicAdd(&a.ncand[fr], 1);   // < h w: a pixel is listed once
    a.cand[(size_t)fr * hw + slot] = p;
}

// grid = f: round k picks the best candidate below the one of round k - 1; key = (size << 24) | (2^24 - 1 - root)
__global__ __launch_bounds__(DC_BLOCK) void component_select_kernel(ClArgs a)
{
    __shared__ u64 red[DC_WAVES];
    const int fr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int hw = a.h * a.w;
    const size_t base = (size_t)fr * hw;
    const int n = min(max(a.ncand[fr], 0), hw);
    const int want = min(n, a.max_components);
    int keep = 0;
    u64 below = ~0ull;
    for (int k = 0; k < want; ++k) {
        u64 best = 0;
        for (int i = tid; i < n; i += DC_BLOCK) {
            const int r = a.cand[base + i];
            const u64 key = ((u64)(unsigned)a.size[base + r] << 24) | (u64)(FRAME_MAX_PIXELS - 1 - r);
            best = key < below && key > best ? key : best;
        }
        best = wave_max_u64(best);
        if (lane == 0)
            red[wv] = best;
        __syncthreads();
        best = 0;
#pragma unroll
        for (int q = 0; q < DC_WAVES; ++q)
            best = red[q] > best ? red[q] : best;
        __syncthreads();                           // the next round writes red
        if (best == 0)                             // (never: keys differ, and only k < n of them are taken; the same in
            break;                                 // every lane)
        below = best;
        keep = k + 1;
        if (tid == 0) {
            const int r = (int)(FRAME_MAX_PIXELS - 1 - (long long)(best & (u64)(FRAME_MAX_PIXELS - 1)));
            const size_t o = (size_t)fr * a.max_components + k;
            a.comp_root[o] = r;
            a.comp_size[o] = (int)(best >> 24);
            a.comp_box[4 * o + 0] = a.w, a.comp_box[4 * o + 1] = a.h;      // min sides start above, max sides below
            a.comp_box[4 * o + 2] = -1, a.comp_box[4 * o + 3] = -1;
            a.rank[base + r] = k + 1;
        }
    }
    for (int k = keep + tid; k < a.max_components; k += DC_BLOCK) {
        const size_t o = (size_t)fr * a.max_components + k;
        a.comp_root[o] = -1;
        a.comp_size[o] = -1;
        a.comp_box[4 * o + 0] = a.comp_box[4 * o + 1] = a.comp_box[4 * o + 2] = a.comp_box[4 * o + 3] = -1;
    }
    if (tid == 0) {
        a.n_components[fr] = keep;
        a.n_candidates[fr] = n;
    }
}

// grid = f * ceil(h w / 1024): the label of every pixel, and the boxes through LDS
__global__ __launch_bounds__(DC_BLOCK) void component_label_kernel(ClArgs a)
{
    __shared__ int box[DC_MAX_COMPONENTS][4];
    const int hw = a.h * a.w;
    const int chunks = (hw + DC_TILE - 1) / DC_TILE;
    const int fr = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int tid = threadIdx.x;
    const size_t base = (size_t)fr * hw;
    for (int k = tid; k < a.max_components; k += DC_BLOCK)
        box[k][0] = a.w, box[k][1] = a.h, box[k][2] = -1, box[k][3] = -1;
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < DC_TILE_PASSES; ++pass) {
        const int p = chunk * DC_TILE + pass * DC_BLOCK + tid;
        if (p >= hw)
            continue;
        const int r = a.root[base + p];
        int k = cl_root_ok(r, hw) ? a.rank[base + r] : 0;
        if (k < 0 || k > a.max_components)
            k = 0;
        a.label[base + p] = (unsigned char)k;
        if (k) {
            const int u = p % a.w, v = p / a.w;
            atomicMin(&box[k - 1][0], u);
            atomicMin(&box[k - 1][1], v);
            atomicMax(&box[k - 1][2], u);
            atomicMax(&box[k - 1][3], v);
        }
    }
    __syncthreads();
    for (int k = tid; k < a.max_components; k += DC_BLOCK) {
        if (box[k][2] < 0)
            continue;
        int *out = a.comp_box + 4 * ((size_t)fr * a.max_components + k);
        atomicMin(out + 0, box[k][0]);
        atomicMin(out + 1, box[k][1]);
        atomicMax(out + 2, box[k][2]);
        atomicMax(out + 3, box[k][3]);
    }
}

// The workspace of cloudaae_component_labels (null: the size alone is asked for): counts = size [m] | rank [m] | ncand [f]
// ints, which one memset of `cleared` bytes clears together, then cand [m] ints, written before it is read.  (The byte added
// to either region keeps the size above zero at f = 0.)
struct ClWorkspace {
    int *counts, *cand;
    size_t cleared, bytes;
};

static ClWorkspace cl_workspace(size_t m, size_t f, void *workspace)
{
    Carver ws(workspace);
    ClWorkspace L;
    L.cleared = sizeof(int) * (2 * m + f);
    L.counts = (int *)ws.take<char>(L.cleared + 1);
    L.cand = (int *)ws.take<char>(sizeof(int) * m + 1);
    L.bytes = ws.bytes();
    return L;
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_depth_plane(int f, int h, int w, const uint16_t *depth, const float *intrinsics,
                                      unsigned long long seed, long long first_frame, int n_hyp, int stride, double tol,
                                      int min_plane_percent, int *count, int *tested, double *plane, int *plane_hyp,
                                      cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_plane";
    CLOUDAAE_REQUIRE(frame_within_limits(0, f, h, w), name, CLOUDAAE_FRAME_LIMITS_F0);
    CLOUDAAE_REQUIRE(n_hyp >= 1 && n_hyp <= DC_MAX_HYP && stride >= 1 && first_frame >= 0 && first_frame <= DC_MAX_FIRST_FRAME &&
                         min_plane_percent >= 0 && min_plane_percent <= 100 && tol >= 0.0,
                     name, "outside the limits: 1 <= n_hyp <= 4096; stride >= 1; 0 <= first_frame <= 2^40; "
                           "0 <= min_plane_percent <= 100; tol >= 0");
    if (f == 0)
        return 0;
    CLOUDAAE_REQUIRE(depth && intrinsics && count && tested && plane && plane_hyp, name, "null pointer");
    DpArgs a;
    a.f = f, a.h = h, a.w = w, a.n_hyp = n_hyp, a.stride = stride, a.min_plane_percent = min_plane_percent;
    a.hs = (int)(((long long)h + stride - 1) / stride);
    a.ws = (int)(((long long)w + stride - 1) / stride);
    a.runs = ceil_div((long long)a.hs * a.ws, DC_RUN);
    a.hyp_blocks = ceil_div(n_hyp, DC_HB);
    a.depth = (const unsigned short *)depth, a.intrinsics = intrinsics, a.seed = seed, a.first_frame = first_frame;
    a.tol2 = tol * tol;
    a.count = count, a.tested = tested, a.plane = plane, a.plane_hyp = plane_hyp;
    // f * runs <= 2^28 / 1024 + f and hyp_blocks <= 512: the grid stays below 2^31 only with this check
    const long long grid = (long long)f * a.runs * a.hyp_blocks;
    CLOUDAAE_REQUIRE(grid <= (1ll << 31) - 1, name, "f * ceil(tested cells / 1024) * ceil(n_hyp / 8) must stay below 2^31");
    hipStream_t sm = (hipStream_t)stream;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int) * (size_t)f * n_hyp, sm), name);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(tested, 0, sizeof(int) * (size_t)f, sm), name);
    hipLaunchKernelGGL(depth_plane_count_kernel, dim3((unsigned)grid), dim3(DC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(depth_plane_winner_kernel, dim3((unsigned)f), dim3(64), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_depth_foreground(int f, int h, int w, const uint16_t *depth, const float *intrinsics,
                                           const double *plane, const int *plane_hyp, double tol, double max_height,
                                           uint8_t *fg, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_foreground";
    CLOUDAAE_REQUIRE(frame_within_limits(0, f, h, w), name, CLOUDAAE_FRAME_LIMITS_F0);
    CLOUDAAE_REQUIRE(tol >= 0.0 && max_height >= 0.0, name, "tol and max_height must be numbers >= 0");
    if (f == 0)
        return 0;
    CLOUDAAE_REQUIRE(depth && intrinsics && plane && plane_hyp && fg, name, "null pointer");
    hipLaunchKernelGGL(depth_foreground_kernel, dim3(ceil_div((long long)f * h * w, DC_BLOCK)), dim3(DC_BLOCK), 0,
                       (hipStream_t)stream, f, h, w, (const unsigned short *)depth, intrinsics, plane, plane_hyp, tol * tol,
                       max_height * max_height, (unsigned char *)fg);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API long long cloudaae_depth_components_workspace_bytes(int f, int h, int w)
{
    if (!frame_within_limits(0, f, h, w))
        return 0;
    return (long long)workspace_pad(sizeof(int) * (size_t)f * h * w + 1);
}

CLOUDAAE_API int cloudaae_depth_components(int f, int h, int w, const uint16_t *depth, const uint8_t *fg, const int *jump_units,
                                           int *root, int *status, void *workspace, long long workspace_bytes,
                                           cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_components";
    CLOUDAAE_REQUIRE(frame_within_limits(0, f, h, w), name, CLOUDAAE_FRAME_LIMITS_F0);
    if (f == 0)
        return 0;
    CLOUDAAE_REQUIRE(depth && fg && jump_units && root && status && workspace, name, "null pointer");
    CLOUDAAE_REQUIRE(workspace_bytes >= cloudaae_depth_components_workspace_bytes(f, h, w), name,
                     "workspace smaller than cloudaae_depth_components_workspace_bytes");
    DccArgs a;
    a.f = f, a.h = h, a.w = w;
    a.tx = (w + DC_TW - 1) / DC_TW, a.ty = (h + DC_TH - 1) / DC_TH;
    a.nv = (a.tx - 1) * h, a.nh = (a.ty - 1) * w;
    a.depth = (const unsigned short *)depth, a.fg = (const unsigned char *)fg, a.jump_units = jump_units;
    a.lab = (int *)workspace, a.root = root, a.status = status;
    hipStream_t sm = (hipStream_t)stream;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int) * (size_t)f, sm), name);
    // f tx ty <= f (h w / 1024 + h / 32 + w / 32 + 1): far below the grid limit
    hipLaunchKernelGGL(depth_components_tile_kernel, dim3((unsigned)((long long)f * a.tx * a.ty)), dim3(DC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    const long long pairs = (long long)f * ((long long)a.nv + a.nh);
    if (pairs > 0) {
        hipLaunchKernelGGL(depth_components_seam_kernel, dim3(ceil_div(pairs, DC_BLOCK)), dim3(DC_BLOCK), 0, sm, a);
        CLOUDAAE_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(depth_components_flatten_kernel, dim3(ceil_div((long long)f * h * w, DC_BLOCK)), dim3(DC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API long long cloudaae_component_labels_workspace_bytes(int f, int h, int w)
{
    if (!frame_within_limits(0, f, h, w))
        return 0;
    return (long long)cl_workspace((size_t)f * h * w, (size_t)f, nullptr).bytes;
}

CLOUDAAE_API int cloudaae_component_labels(int f, int h, int w, const int *root, int min_pixels, int max_components,
                                           uint8_t *label, int *n_components, int *n_candidates, int *comp_root, int *comp_size,
                                           int *comp_box, void *workspace, long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_component_labels";
    CLOUDAAE_REQUIRE(frame_within_limits(0, f, h, w), name, CLOUDAAE_FRAME_LIMITS_F0);
    CLOUDAAE_REQUIRE(min_pixels >= 1 && max_components >= 1 && max_components <= DC_MAX_COMPONENTS, name,
                     "outside the limits: min_pixels >= 1; 1 <= max_components <= 254");
    if (f == 0)
        return 0;
    CLOUDAAE_REQUIRE(root && label && n_components && n_candidates && comp_root && comp_size && comp_box && workspace, name,
                     "null pointer");
    const size_t m = (size_t)f * h * w;
    const ClWorkspace L = cl_workspace(m, (size_t)f, workspace);
    CLOUDAAE_REQUIRE(workspace_bytes >= (long long)L.bytes, name,
                     "workspace smaller than cloudaae_component_labels_workspace_bytes");
    ClArgs a;
    a.f = f, a.h = h, a.w = w, a.min_pixels = min_pixels, a.max_components = max_components;
    a.root = root;
    a.size = L.counts, a.rank = a.size + m, a.ncand = a.rank + m, a.cand = L.cand;
    a.label = (unsigned char *)label;
    a.n_components = n_components, a.n_candidates = n_candidates;
    a.comp_root = comp_root, a.comp_size = comp_size, a.comp_box = comp_box;
    hipStream_t sm = (hipStream_t)stream;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(L.counts, 0, L.cleared, sm), name);
    const dim3 pixels(ceil_div((long long)m, DC_BLOCK));
    hipLaunchKernelGGL(component_size_kernel, pixels, dim3(DC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(component_candidates_kernel, pixels, dim3(DC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(component_select_kernel, dim3((unsigned)f), dim3(DC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    const long long chunks = ((long long)h * w + DC_TILE - 1) / DC_TILE;
    hipLaunchKernelGGL(component_label_kernel, dim3((unsigned)((long long)f * chunks)), dim3(DC_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
