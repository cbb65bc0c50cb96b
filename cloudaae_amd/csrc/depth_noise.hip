// depth_noise.hip -- a structured-light depth sensor's noise on rendered depth / label frames, and the per-pixel normal
// map it is built on (gfx950).  DESIGN.md, "Sensor noise", is the definition; tests/depth_noise_reference.py restates it
// in NumPy.  The draws are u01 / normal2 of philox.h in fp32, widened; everything after them is fp64 on exactly widened
// fp32 or integer inputs, un-fused (the file is compiled with -ffp-contract=off), in the order written here.
//
//   cloudaae_depth_normals       a memset and one launch: the slope at every pixel (normal, angle to the viewing ray)
//   cloudaae_depth_sensor_noise  a memset and one launch: lateral jitter, axial noise, dropout, disparity steps and the
//                                quantisation, one lane per destination pixel
//
// Both kernels call dn_slope, so the two entries cannot drift apart.  A workgroup of 256 lanes takes 256 pixels of ONE
// frame (grid = frames x tiles); the five depth / label taps of a slope are plain loads -- neighbouring lanes share
// their cache lines.  A counter is a ballot + popcount per wave, the four waves meet in LDS, and one integer atomic per
// workgroup and counter (none for a zero) adds into the zeroed output, as in bop_score.hip.
#include "common.h"
#include "depth_frame.h"
#include "philox.h"
#include "../../include/cloudaae_hip.h"

#include <math.h>

namespace cloudaae {

typedef unsigned long long u64;

constexpr int DN_BLOCK = 256;
constexpr int DN_WAVES = DN_BLOCK / 64;
constexpr unsigned DN_STREAM_NORMALS = 21u;        // normal2(r0, r1) -> n_u, n_v; normal2(r2, r3) -> n_z, (unused)
constexpr unsigned DN_STREAM_DROP = 22u;           // r0: the dropout word
constexpr u64 DN_MAX_FRAME = 1ull << 40;           // global frame indices lie below
constexpr double DN_HALF_PI = 1.5707963267948966;  // the double nearest pi / 2

struct DnFrame {
    const unsigned short *depth;                   // this frame's [h, w]
    const unsigned char *label;
    int h, w;
    Pinhole<double> cam;
};

// adds the workgroup's totals of N per-lane predicates into dst[0 .. N): every lane of the workgroup must call it
template <int N>
__device__ __forceinline__ void dn_add_counts(const bool (&pred)[N], int *dst)
{
    __shared__ int red[DN_WAVES][N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int n = wave_count(pred[i]);
        if (lane == 0)
            red[wv][i] = n;
    }
    __syncthreads();
    if (tid < N) {
        int sum = 0;
#pragma unroll
        for (int q = 0; q < DN_WAVES; ++q)
            sum += red[q][tid];
        if (sum != 0)
            __hip_atomic_fetch_add(dst + tid, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the neighbour (u, v) of a pixel with label l: valid when inside the image, with depth and with that label
__device__ __forceinline__ bool dn_tap(const DnFrame &fr, int u, int v, unsigned char l, double (&p)[3])
{
    if (u < 0 || u >= fr.w || v < 0 || v >= fr.h)
        return false;
    const size_t i = (size_t)v * fr.w + u;
    const unsigned short d = fr.depth[i];
    if (d == 0 || fr.label[i] != l)
        return false;
    backproject(fr.cam, u, v, d, p);
    return true;
}

// the difference along one axis: central when both neighbours are valid, one-sided with the valid one, else none
__device__ __forceinline__ bool dn_axis(const DnFrame &fr, int u, int v, int du, int dv, unsigned char l,
                                       const double (&centre)[3], double (&g)[3])
{
    double lo[3], hi[3];
    const bool vlo = dn_tap(fr, u - du, v - dv, l, lo), vhi = dn_tap(fr, u + du, v + dv, l, hi);
    if (!vlo && !vhi)
        return false;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        g[k] = (vhi ? hi[k] : centre[k]) - (vlo ? lo[k] : centre[k]);
    return true;
}

__device__ __forceinline__ double dn_dot(const double (&a)[3], const double (&b)[3])
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// The slope at pixel (u, v), whose depth d is not 0.  false: the pixel is flat (normal zeros, theta 0).  Otherwise n is
// the unit normal turned towards the camera and theta its angle to the viewing ray, in [0, pi / 2].
__device__ __forceinline__ bool dn_slope(const DnFrame &fr, int u, int v, unsigned short d, double (&n)[3], double &theta)
{
    n[0] = n[1] = n[2] = 0.0;
    theta = 0.0;
    const unsigned char l = fr.label[(size_t)v * fr.w + u];
    double ray[3], gx[3], gy[3];
    backproject(fr.cam, u, v, d, ray);
    const bool hx = dn_axis(fr, u, v, 1, 0, l, ray, gx), hy = dn_axis(fr, u, v, 0, 1, l, ray, gy);
    if (!hx || !hy)
        return false;
    double c[3];
    c[0] = gx[1] * gy[2] - gx[2] * gy[1];
    c[1] = gx[2] * gy[0] - gx[0] * gy[2];
    c[2] = gx[0] * gy[1] - gx[1] * gy[0];
    const double nn = dn_dot(c, c), nr = dn_dot(c, ray), rr = dn_dot(ray, ray);
    if (!(nn > 0.0) || !isfinite(nn))              // (a NaN fails the first comparison)
        return false;
    const double len = sqrt(nn);
    const double cosine = fabs(nr) / (len * sqrt(rr));
    if (!(cosine >= 0.0))                          // not a number: flat
        return false;
    theta = acos(cosine < 1.0 ? cosine : 1.0);
    const double sign = nr > 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        n[k] = sign * (c[k] / len);
    return true;
}

__device__ __forceinline__ DnFrame dn_frame(int f, int h, int w, const unsigned short *depth, const unsigned char *label,
                                           const float *intrinsics)
{
    DnFrame fr;
    const size_t hw = (size_t)h * w;
    fr.depth = depth + (size_t)f * hw;
    fr.label = label + (size_t)f * hw;
    fr.h = h, fr.w = w;
    fr.cam = pinhole<double>(intrinsics + 5 * (size_t)f);
    return fr;
}

// grid = f * tiles: workgroup b takes pixels (b % tiles) * 256 .. of frame b / tiles
__global__ __launch_bounds__(DN_BLOCK) void depth_normals_kernel(int h, int w, int tiles,
                                                                const unsigned short *__restrict__ depth,
                                                                const unsigned char *__restrict__ label,
                                                                const float *__restrict__ intrinsics,
                                                                float *__restrict__ normals, float *__restrict__ theta_out,
                                                                int *__restrict__ flat_counts)
{
    const int f = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int hw = h * w;
    const int p = tile * DN_BLOCK + (int)threadIdx.x;
    bool flat[1] = {false};
    if (p < hw) {
        const DnFrame fr = dn_frame(f, h, w, depth, label, intrinsics);
        const unsigned short d = fr.depth[p];
        double n[3] = {0.0, 0.0, 0.0}, theta = 0.0;
        if (d != 0)
            flat[0] = !dn_slope(fr, p % w, p / w, d, n, theta);
        const size_t o = (size_t)f * hw + p;
        normals[3 * o + 0] = (float)n[0];
        normals[3 * o + 1] = (float)n[1];
        normals[3 * o + 2] = (float)n[2];
        if (theta_out)
            theta_out[o] = (float)theta;
    }
    dn_add_counts<1>(flat, flat_counts + f);
}

struct DnSensor {
    double sigma_l, a0, a1, z0, a2, theta_max, theta_drop, baseline, disparity_step;
    u64 drop_below;                                // floor(p_drop 2^32), in [0, 2^32]
    u64 seed, first_frame;
};

__global__ __launch_bounds__(DN_BLOCK) void depth_sensor_noise_kernel(int h, int w, int tiles,
                                                                     const unsigned short *__restrict__ depth,
                                                                     const unsigned char *__restrict__ label,
                                                                     const float *__restrict__ intrinsics, DnSensor s,
                                                                     unsigned short *__restrict__ depth_out,
                                                                     unsigned char *__restrict__ label_out,
                                                                     int *__restrict__ counts,
                                                                     double *__restrict__ z_noisy)
{
    const int f = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int hw = h * w;
    const int p = tile * DN_BLOCK + (int)threadIdx.x;
    bool what[4] = {false, false, false, false};   // input depth, dropped by angle, by chance, lost to range / disparity
    if (p < hw) {
        const DnFrame fr = dn_frame(f, h, w, depth, label, intrinsics);
        const int u = p % w, v = p / w;
        what[0] = fr.depth[p] != 0;
        const u64 ctr = ((s.first_frame + (u64)f) << 24) + (u64)p;
        unsigned r[4], q[4];
        philox4x32(s.seed, ctr, DN_STREAM_NORMALS, r);
        philox4x32(s.seed, ctr, DN_STREAM_DROP, q);
        float n_u, n_v, n_z, unused;
        normal2(r[0], r[1], n_u, n_v);
        normal2(r[2], r[3], n_z, unused);
        // 1. lateral jitter (the clamp in double: the offset of a large sigma_l does not fit an int)
        const double tu = (double)u + rint((double)n_u * s.sigma_l), tv = (double)v + rint((double)n_v * s.sigma_l);
        const int su = (int)fmin(fmax(tu, 0.0), (double)(w - 1)), sv = (int)fmin(fmax(tv, 0.0), (double)(h - 1));
        const size_t src = (size_t)sv * w + su;
        const unsigned short d = fr.depth[src];
        unsigned short out = 0;
        double zn = 0.0;
        if (d != 0) {
            // 2. axial noise
            double n[3], theta_raw;
            dn_slope(fr, su, sv, d, n, theta_raw);
            const double z = (double)d / fr.cam.factor;
            const double theta = theta_raw < s.theta_max ? theta_raw : s.theta_max;
            const double dz = z - s.z0, rest = DN_HALF_PI - theta;
            const double sigma_z = (s.a0 + s.a1 * (dz * dz)) + ((s.a2 / sqrt(z)) * (theta * theta)) / (rest * rest);
            zn = z + (double)n_z * sigma_z;
            // 3. dropout
            if (theta_raw > s.theta_drop) {
                what[1] = true;
            } else if ((u64)q[0] < s.drop_below) {
                what[2] = true;
            } else {
                // 4. disparity steps
                double zq = zn;
                bool lost = false;
                if (s.disparity_step > 0.0) {
                    const double fb = fr.cam.fx * s.baseline;
                    const double k = rint((fb / zn) / s.disparity_step);
                    lost = !(k >= 1.0);
                    zq = fb / (k * s.disparity_step);
                }
                // 5. quantisation (a NaN fails the comparisons)
                const double du = floor(zq * fr.cam.factor + 0.5);
                if (!lost && du >= 1.0 && du <= 65535.0)
                    out = (unsigned short)(int)du;
                else
                    what[3] = true;
            }
            if (!isfinite(zn))
                zn = 0.0;
        }
        const size_t o = (size_t)f * hw + p;
        depth_out[o] = out;
        label_out[o] = fr.label[src];
        if (z_noisy)
            z_noisy[o] = zn;
    }
    dn_add_counts<4>(what, counts + 4 * (size_t)f);
}

} // namespace cloudaae

using namespace cloudaae;

CLOUDAAE_API int cloudaae_depth_normals(int f, int h, int w, const uint16_t *depth, const uint8_t *label, const float *intrinsics,
                                        float *normals, float *theta, int *flat_counts, cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_normals";
    CLOUDAAE_REQUIRE(frame_within_limits(1, f, h, w), name, CLOUDAAE_FRAME_LIMITS);
    CLOUDAAE_REQUIRE(depth && label && intrinsics && normals && flat_counts, name, "null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const int tiles = ceil_div((long long)h * w, DN_BLOCK);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(flat_counts, 0, sizeof(int) * (size_t)f, sm), name);
    // f * tiles <= 2^28 / 256 + f: below the grid limit
    hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)((long long)f * tiles)), dim3(DN_BLOCK), 0, sm, h, w, tiles,
                       (const unsigned short *)depth, (const unsigned char *)label, intrinsics, normals, theta, flat_counts);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}

CLOUDAAE_API int cloudaae_depth_sensor_noise(int f, int h, int w, const uint16_t *depth, const uint8_t *label,
                                             const float *intrinsics, unsigned long long seed, unsigned long long first_frame,
                                             double sigma_l, double a0, double a1, double z0, double a2, double theta_max,
                                             double theta_drop, double p_drop, double baseline, double disparity_step,
                                             uint16_t *depth_out, uint8_t *label_out, int *counts, double *z_noisy,
                                             cloudaae_stream_t stream)
{
    const char *name = "cloudaae_depth_sensor_noise";
    CLOUDAAE_REQUIRE(frame_within_limits(1, f, h, w), name, CLOUDAAE_FRAME_LIMITS);
    CLOUDAAE_REQUIRE(first_frame < DN_MAX_FRAME && first_frame + (u64)f <= DN_MAX_FRAME, name,
                     "global frame indices (first_frame + f) must lie below 2^40");
    CLOUDAAE_REQUIRE(sigma_l >= 0.0 && isfinite(sigma_l), name, "sigma_l must be >= 0 and finite");
    CLOUDAAE_REQUIRE(theta_max >= 0.0 && theta_max < DN_HALF_PI, name, "theta_max must lie in [0, pi / 2)");
    CLOUDAAE_REQUIRE(p_drop >= 0.0 && p_drop <= 1.0, name, "p_drop must lie in [0, 1]");
    CLOUDAAE_REQUIRE(isfinite(a0) && isfinite(a1) && isfinite(z0) && isfinite(a2) && !isnan(theta_drop) && isfinite(baseline) &&
                         disparity_step >= 0.0 && isfinite(disparity_step),
                     name, "a0, a1, z0, a2 and baseline must be finite, theta_drop a number, disparity_step >= 0 and finite");
    CLOUDAAE_REQUIRE(depth && label && intrinsics && depth_out && label_out && counts, name, "null pointer");
    DnSensor s;
    s.sigma_l = sigma_l, s.a0 = a0, s.a1 = a1, s.z0 = z0, s.a2 = a2, s.theta_max = theta_max, s.theta_drop = theta_drop;
    s.baseline = baseline, s.disparity_step = disparity_step;
    s.drop_below = (u64)floor(p_drop * 4294967296.0);
    s.seed = seed, s.first_frame = first_frame;
    hipStream_t sm = (hipStream_t)stream;
    const int tiles = ceil_div((long long)h * w, DN_BLOCK);
    CLOUDAAE_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * 4 * (size_t)f, sm), name);
    hipLaunchKernelGGL(depth_sensor_noise_kernel, dim3((unsigned)((long long)f * tiles)), dim3(DN_BLOCK), 0, sm, h, w, tiles,
                       (const unsigned short *)depth, (const unsigned char *)label, intrinsics, s, (unsigned short *)depth_out,
                       (unsigned char *)label_out, counts, z_noisy);
    CLOUDAAE_CHECK_LAUNCH(name);
    return 0;
}
