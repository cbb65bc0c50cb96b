// tsdf_field.h -- the signed distance field of a fused volume, as the kernels that sample it between voxel centres read it:
// the raycast of tsdf.hip and the alignment step of tsdf_align.hip.  Here are the volume and its limits, the value of a
// voxel's state, the cell of a coordinate, the load of a cell's eight values and the trilinear form with its gradient.
// DESIGN.md, "Scanning" and "Scanning on the field", are the definitions.  Both includers are compiled un-fused
// (-ffp-contract=off) and without packed fp32, so this text gives the same bits in both.
#pragma once
#include "common.h"

#include <math.h>

namespace cloudaae {

constexpr int TSDF_MAX_DIM = 512;
constexpr long long TSDF_MAX_VOXELS = 1ll << 27;
constexpr double TSDF_QUANT = 4096.0;

#define TSDF_VOLUME_LIMITS "outside the limits: 2 <= nx, ny, nz <= 512; nx ny nz <= 2^27"
#define TSDF_FRAME_LIMITS "the origin must be finite and the voxel finite and positive"

struct TsdfVolume {
    int nx, ny, nz;
    double ox, oy, oz, s;
};

static inline bool tsdf_volume_ok(long long nx, long long ny, long long nz)
{
    return nx >= 2 && ny >= 2 && nz >= 2 && nx <= TSDF_MAX_DIM && ny <= TSDF_MAX_DIM && nz <= TSDF_MAX_DIM &&
           nx * ny * nz <= TSDF_MAX_VOXELS;
}

static inline bool tsdf_frame_ok(double ox, double oy, double oz, double voxel)
{
    return isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(voxel) && voxel > 0.0;
}

// tsdf_value of a state that is already in registers, without a branch: a sampler loads a cell's eight states at once and
// forms the values afterwards (through tsdf_value the compiler makes every corner's load wait for the corner before it)
__device__ __forceinline__ bool tsdf_value_of(const int4 s, int min_count, double &v)
{
    const bool near = s.y >= min_count, known = near || s.w >= 1;
    const double num = (double)(near ? s.x : s.z), den = (double)(near ? s.y : s.w);
    v = known ? num / den : 0.0;
    return known;
}

// the cell of a coordinate: clamp(floor(g), 0, n - 2), the clamp in float64 before the conversion
__device__ __forceinline__ int tsdf_ray_cell(double g, int n)
{
    const double fl = floor(g), top = (double)(n - 2);
    return (int)(fl >= 0.0 ? (fl <= top ? fl : top) : 0.0);
}

// the eight values of cell (i, j, k), corner c at voxel (i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)): the eight loads
// first, then the values; -> false when a corner is unknown
__device__ __forceinline__ bool tsdf_cell_values(const int4 *state, int nx, int ny, int i, int j, int k, int min_count,
                                                 double (&v)[8])
{
    int4 s[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
        s[c] = state[((size_t)(k + (c >> 2)) * ny + (size_t)(j + ((c >> 1) & 1))) * nx + (size_t)(i + (c & 1))];
    bool known = true;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        known = tsdf_value_of(s[c], min_count, v[c]) && known;
    return known;
}

// The trilinear form at the fractions (fx, fy, fz) of a cell: along x on the corner pairs (0,1), (2,3), (4,5), (6,7), then
// along y, then along z.  The four values after x and the two after y are kept: the gradient is formed of them.
struct TsdfTrilinear {
    double c00, c10, c01, c11, c0, c1, val;
};

__device__ __forceinline__ TsdfTrilinear tsdf_trilinear(const double (&v)[8], double fx, double fy, double fz)
{
    TsdfTrilinear t;
    t.c00 = v[0] + (v[1] - v[0]) * fx, t.c10 = v[2] + (v[3] - v[2]) * fx;
    t.c01 = v[4] + (v[5] - v[4]) * fx, t.c11 = v[6] + (v[7] - v[6]) * fx;
    t.c0 = t.c00 + (t.c10 - t.c00) * fy, t.c1 = t.c01 + (t.c11 - t.c01) * fy;
    t.val = t.c0 + (t.c1 - t.c0) * fz;
    return t;
}

// the derivative of that form by (fx, fy, fz), the same nesting differentiated: d/dfx blends the four x-differences by fy,
// then fz; d/dfy blends c10 - c00 with c11 - c01 by fz; d/dfz = c1 - c0
__device__ __forceinline__ void tsdf_trilinear_gradient(const double (&v)[8], const TsdfTrilinear &t, double fy, double fz,
                                                        double (&g)[3])
{
    const double d00 = v[1] - v[0], d10 = v[3] - v[2], d01 = v[5] - v[4], d11 = v[7] - v[6];
    const double gx0 = d00 + (d10 - d00) * fy, gx1 = d01 + (d11 - d01) * fy;
    const double e0 = t.c10 - t.c00, e1 = t.c11 - t.c01;
    g[0] = gx0 + (gx1 - gx0) * fz;
    g[1] = e0 + (e1 - e0) * fz;
    g[2] = t.c1 - t.c0;
}

} // namespace cloudaae
