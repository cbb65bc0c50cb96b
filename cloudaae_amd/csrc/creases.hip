// creases.hip -- concave creases of the foreground of a depth frame on the GPU (gfx950), the cut that separates objects
// that touch before cloudaae_depth_components labels them.  DESIGN.md, "Creases", is the definition;
// tests/creases_reference.py restates it in NumPy.  Every output is an integer and a pure function of the input: the box
// sums are integer sums, the test is double with + - * / in the written order (the file is compiled with
// -ffp-contract=off and without packed fp32), and its result is a comparison.
//
//   cloudaae_depth_creases  a memset and two launches, both LDS-tiled stencils over 32 x 32 tiles, 256 lanes, four pixels
//                           per lane: (a) the tile and a halo of `smooth` pixels staged as one int per pixel (the depth, -1
//                           where the pixel is no foreground or outside the frame), then the box sum and count of every
//                           pixel packed into smooth_map; (b) the tile and a halo of `step` pixels staged as the raw depth
//                           and the smoothed point (three doubles, formed once per staged foreground pixel), then the
//                           four directions of every foreground pixel, the three images and one integer add per
//                           workgroup into n_crease
//
// Frame borders and partial tiles are predicates (a staged -1), never padding.  Every loop is bounded by smooth, step or
// the tile; no workgroup waits for another.
#include "common.h"
#include "depth_frame.h"
#include "workspace.h"
#include "../../include/cloudaae_hip.h"

namespace cloudaae {

constexpr int CR_BLOCK = 256;
constexpr int CR_WAVES = CR_BLOCK / 64;
constexpr int CR_TW = 32, CR_TH = 32;
constexpr int CR_TILE = CR_TW * CR_TH;
constexpr int CR_TILE_PASSES = CR_TILE / CR_BLOCK;
constexpr int CR_MAX_STEP = 8, CR_MAX_SMOOTH = 7;
constexpr int CR_SMOOTH_SIDE = CR_TW + 2 * CR_MAX_SMOOTH;          // 46: 46 x 46 ints = 8 464 bytes
constexpr size_t CR_CELL_BYTES = 3 * sizeof(double) + sizeof(int);   // a staged pixel of the test: its point, its raw depth
constexpr size_t CR_MAX_LDS = (size_t)(CR_TW + 2 * CR_MAX_STEP) * (CR_TH + 2 * CR_MAX_STEP) * CR_CELL_BYTES;

struct CrArgs {
    int f, h, w, tx, ty, step, smooth;
    const unsigned short *depth;
    const unsigned char *fg;
    const float *intrinsics;
    const int *jump_units;
    double cos2;
    unsigned *smooth_map;                          // workspace [f, h w]
    unsigned char *crease, *tested, *fg_cut;
    int *n_crease;
};

// the depth of frame pixel (x, y) as an int, -1 where it is outside the frame or no foreground: nothing is read there
__device__ __forceinline__ int cr_staged_depth(const CrArgs &a, size_t base, int x, int y)
{
    if (x < 0 || y < 0 || x >= a.w || y >= a.h)
        return -1;
    const size_t i = base + (size_t)y * a.w + x;
    return a.fg[i] != 0 ? (int)a.depth[i] : -1;
}

// grid = f * tx * ty: (a) smooth_map = (S << 8) | n over the members of each foreground pixel's box
__global__ __launch_bounds__(CR_BLOCK) void depth_creases_smooth_kernel(CrArgs a)
{
    __shared__ int dep[CR_SMOOTH_SIDE * CR_SMOOTH_SIDE];
    const int tiles = a.tx * a.ty;
    const int fr = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int x0 = (t % a.tx) * CR_TW, y0 = (t / a.tx) * CR_TH;
    const int tid = threadIdx.x;
    const int r = a.smooth, side = CR_TW + 2 * r;
    const size_t base = (size_t)fr * ((size_t)a.h * a.w);
    const int jump = a.jump_units[fr];
    for (int e = tid; e < side * side; e += CR_BLOCK)
        dep[e] = cr_staged_depth(a, base, x0 - r + e % side, y0 - r + e / side);
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < CR_TILE_PASSES; ++pass) {
        const int l = pass * CR_BLOCK + tid;
        const int lx = l % CR_TW, ly = l / CR_TW;
        if (x0 + lx >= a.w || y0 + ly >= a.h)
            continue;
        const int dc = dep[(ly + r) * side + lx + r];
        unsigned packed = 0;
        if (dc >= 0 && jump >= 0) {
            unsigned sum = 0, n = 0;               // sum <= 225 * 65535 < 2^24, n <= 225 < 2^8
            for (int dy = 0; dy <= 2 * r; ++dy)
                for (int dx = 0; dx <= 2 * r; ++dx) {
                    const int dq = dep[(ly + dy) * side + lx + dx];
                    const int diff = dq > dc ? dq - dc : dc - dq;
                    const bool member = dq >= 0 && diff <= jump;
                    sum += member ? (unsigned)dq : 0u;
                    n += member ? 1u : 0u;
                }
            packed = (sum << 8) | n;
        }
        a.smooth_map[base + (size_t)(y0 + ly) * a.w + x0 + lx] = packed;
    }
}

__device__ __forceinline__ double cr_dot(double ax, double ay, double az, double bx, double by, double bz)
{
    return (ax * bx + ay * by) + az * bz;
}

// grid = f * tx * ty, dynamic LDS = side^2 (3 doubles + 1 int), side = 32 + 2 step: (b) the crease test
__global__ __launch_bounds__(CR_BLOCK) void depth_creases_test_kernel(CrArgs a)
{
    extern __shared__ double cr_lds[];
    __shared__ int total[CR_WAVES];
    const int tiles = a.tx * a.ty;
    const int fr = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int x0 = (t % a.tx) * CR_TW, y0 = (t / a.tx) * CR_TH;
    const int tid = threadIdx.x;
    const int s = a.step, side = CR_TW + 2 * s, cells = side * side;
    double *px = cr_lds, *py = px + cells, *pz = py + cells;
    int *raw = (int *)(pz + cells);
    const size_t base = (size_t)fr * ((size_t)a.h * a.w);
    const Pinhole<double> cam = pinhole<double>(a.intrinsics + 5 * (size_t)fr);
    const long long reach = (long long)s * (long long)a.jump_units[fr];
    for (int e = tid; e < cells; e += CR_BLOCK) {
        const int x = x0 - s + e % side, y = y0 - s + e / side;
        const int d = cr_staged_depth(a, base, x, y);
        raw[e] = d;
        if (d < 0)
            continue;                              // no foreground: no float64 work, and its point is never read
        const unsigned word = a.smooth_map[base + (size_t)y * a.w + x];
        const unsigned n = word & 255u;
        double P[3] = {0.0, 0.0, 0.0};
        if (n)                                     // (n = 0 only in a frame with jump_units < 0, where nothing is tested)
            backproject_metres(cam, x, y, (double)(word >> 8) / ((double)n * cam.factor), P);
        px[e] = P[0], py[e] = P[1], pz[e] = P[2];
    }
    __syncthreads();
    int flagged = 0;
#pragma unroll
    for (int pass = 0; pass < CR_TILE_PASSES; ++pass) {
        const int l = pass * CR_BLOCK + tid;
        const int lx = l % CR_TW, ly = l / CR_TW;
        const bool inside = x0 + lx < a.w && y0 + ly < a.h;
        const int c = (ly + s) * side + lx + s;
        const int dc = inside ? raw[c] : -1;
        unsigned crease = 0, tested = 0;
        if (dc >= 0) {
            const double Cx = px[c], Cy = py[c], Cz = pz[c];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int du = b == 1 ? 0 : 1, dv = b == 0 ? 0 : (b == 3 ? -1 : 1);
                const int off = s * (dv * side + du);
                const int da = raw[c - off], db = raw[c + off];
                if (da < 0 || db < 0)
                    continue;
                const long long ga = da > dc ? da - dc : dc - da, gb = db > dc ? db - dc : dc - db;
                if (ga > reach || gb > reach)
                    continue;
                tested |= 1u << b;
                const double e1x = px[c - off] - Cx, e1y = py[c - off] - Cy, e1z = pz[c - off] - Cz;
                const double e2x = px[c + off] - Cx, e2y = py[c + off] - Cy, e2z = pz[c + off] - Cz;
                const double g = cr_dot(e1x, e1y, e1z, e2x, e2y, e2z);
                const double mx = e1x + e2x, my = e1y + e2y, mz = e1z + e2z;
                const double cc = cr_dot(mx, my, mz, Cx, Cy, Cz);
                const double q1 = cr_dot(e1x, e1y, e1z, e1x, e1y, e1z), q2 = cr_dot(e2x, e2y, e2z, e2x, e2y, e2z);
                if (cc < 0.0 && (g >= 0.0 || g * g < a.cos2 * (q1 * q2)))
                    crease |= 1u << b;
            }
        }
        if (inside) {
            const size_t i = base + (size_t)(y0 + ly) * a.w + x0 + lx;
            a.crease[i] = (unsigned char)crease;
            a.tested[i] = (unsigned char)tested;
            a.fg_cut[i] = dc >= 0 && crease == 0 ? 1 : 0;
        }
        flagged += wave_count(crease != 0);
    }
    if ((tid & 63) == 0)
        total[tid >> 6] = flagged;
    __syncthreads();
    if (tid == 0) {
        int n = 0;
#pragma unroll
        for (int q = 0; q < CR_WAVES; ++q)
            n += total[q];
        if (n)
            atomicAdd(&a.n_crease[fr], n);
    }
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API long long cloudaae_depth_creases_workspace_bytes(int f, int h, int w)
{
    if (!frame_within_limits(0, f, h, w))
        return 0;
    return (long long)workspace_pad(sizeof(unsigned) * (size_t)f * h * w + 1);
}

CLOUDAAE_API int cloudaae_depth_creases(int f, int h, int w, const uint16_t *depth, const uint8_t *fg, const float *intrinsics,
                                        const int *jump_units, int step, int smooth, double cos2, uint8_t *crease,
                                        uint8_t *tested, uint8_t *fg_cut, int *n_crease, void *workspace,
                                        long long workspace_bytes, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_creases";
    CLOUDAAE_REQUIRE(frame_within_limits(0, f, h, w), name, CLOUDAAE_FRAME_LIMITS_F0);
    CLOUDAAE_REQUIRE(step >= 1 && step <= CR_MAX_STEP && smooth >= 0 && smooth <= CR_MAX_SMOOTH && cos2 >= 0.0 && cos2 <= 1.0,
                     name, "outside the limits: 1 <= step <= 8; 0 <= smooth <= 7; cos2 a number in [0, 1]");
    if (f == 0)
        return 0;
    CLOUDAAE_REQUIRE(depth && fg && intrinsics && jump_units && crease && tested && fg_cut && n_crease && workspace, name,
                     "null pointer");
    CLOUDAAE_REQUIRE(workspace_bytes >= cloudaae_depth_creases_workspace_bytes(f, h, w), name,
                     "workspace smaller than cloudaae_depth_creases_workspace_bytes");
    CrArgs a;
    a.f = f, a.h = h, a.w = w, a.step = step, a.smooth = smooth, a.cos2 = cos2;
    a.tx = (w + CR_TW - 1) / CR_TW, a.ty = (h + CR_TH - 1) / CR_TH;
    a.depth = (const unsigned short *)depth, a.fg = (const unsigned char *)fg, a.intrinsics = intrinsics;
    a.jump_units = jump_units;
    a.smooth_map = (unsigned *)workspace;
    a.crease = (unsigned char *)crease, a.tested = (unsigned char *)tested, a.fg_cut = (unsigned char *)fg_cut;
    a.n_crease = n_crease;
    hipStream_t sm = (hipStream_t)stream;
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(n_crease, 0, sizeof(int) * (size_t)f, sm), name);
    // f tx ty <= f (h w / 1024 + h / 32 + w / 32 + 1): far below the grid limit
    const dim3 grid((unsigned)((long long)f * a.tx * a.ty));
    hipLaunchKernelGGL(depth_creases_smooth_kernel, grid, dim3(CR_BLOCK), 0, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    // 28 bytes per staged pixel: 40 432 at step 3, above 48 KiB from step 6 on, (32 + 16)^2 * 28 = 64 512 at step 8
    const int side = CR_TW + 2 * step;
    const size_t lds = (size_t)side * side * CR_CELL_BYTES;
    CLOUDAAE_CHECK_HIP(allow_dynamic_lds<depth_creases_test_kernel>(lds, CR_MAX_LDS), name);
    hipLaunchKernelGGL(depth_creases_test_kernel, grid, dim3(CR_BLOCK), lds, sm, a);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
