// depth_frame.h -- what the kernels that read depth frames share: the limits of a batch of frames, the pinhole camera of an
// intrinsics row and the back-projection of a pixel ("Frame segments"; the frame clouds and the depth components
// are defined as that back-projection, tracking, the sensor model and the creases use it in float64).  Every includer is
// compiled un-fused (-ffp-contract=off) and without packed fp32 (none is in the Makefile's PK_OBJS), so this one text gives
// the same bits in all of them.
#pragma once
#include "common.h"

namespace cloudaae {

constexpr long long FRAME_MAX_PIXELS = 1ll << 24;  // h w of one frame (or window)
constexpr long long FRAME_MAX_TOTAL = 1ll << 28;   // f h w of one call

#define CLOUDAAE_FRAME_LIMITS "outside the limits: f, h, w >= 1; h * w <= 2^24; f * h * w <= 2^28"
#define CLOUDAAE_FRAME_LIMITS_F0 "outside the limits: f >= 0; h, w >= 1; h * w <= 2^24; f * h * w <= 2^28"

// the f, h, w part of an entry point's limits: min_f = 0 where an empty batch returns early, 1 where it is refused
static inline bool frame_within_limits(long long min_f, long long f, long long h, long long w)
{
    return f >= min_f && h >= 1 && w >= 1 && h * w <= FRAME_MAX_PIXELS && f * h * w <= FRAME_MAX_TOTAL;
}

// the camera of an intrinsics row (fx, fy, cx, cy, factor_depth), in the arithmetic T of its user
template <typename T>
struct Pinhole {
    T fx, fy, cx, cy, factor;
};

template <typename T>
__device__ __forceinline__ Pinhole<T> pinhole(const float *row)
{
    return Pinhole<T>{(T)row[0], (T)row[1], (T)row[2], (T)row[3], (T)row[4]};
}

// P = (((u - cx) dm) / fx, ((v - cy) dm) / fy, dm) of pixel (u, v) at dm metres: no fma, correctly rounded divisions
template <typename T>
__device__ __forceinline__ void backproject_metres(const Pinhole<T> &c, int u, int v, T dm, T (&p)[3])
{
    p[0] = (((T)u - c.cx) * dm) / c.fx;
    p[1] = (((T)v - c.cy) * dm) / c.fy;
    p[2] = dm;
}

// ... at depth d in the frame's units, an integer of the caller's type: dm = d / factor_depth
template <typename T, typename D>
__device__ __forceinline__ void backproject(const Pinhole<T> &c, int u, int v, D d, T (&p)[3])
{
    backproject_metres(c, u, v, (T)d / c.factor, p);
}

} // namespace cloudaae
