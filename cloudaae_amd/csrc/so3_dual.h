// so3_dual.h -- forward-mode duals and the exponential map of losses/angular_distance_taylor.py:30-66, shared by step.hip
// (rotation error and its gradient, cloudaae_exponential_map) and pose_sample.hip (the rotation of a drawn pose): ONE
// op sequence, so the matrix of a drawn axis-angle has the bits cloudaae_exponential_map gives for it.
#pragma once
#include <hip/hip_runtime.h>

namespace cloudaae {

// Forward-mode duals: a value and its derivative with respect to three inputs.  Carried through exactly the reference's
// op sequence they give what TF's autodiff of that graph yields (step.hip's rotation error); with dconst() inputs the
// derivative parts are dead code and only the value path remains (cloudaae_exponential_map, the pose sampler).
struct Dual {
    double v, d[3];
};
__device__ __forceinline__ Dual dconst(double c) { return Dual{c, {0.0, 0.0, 0.0}}; }
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return Dual{a.v + b.v, {a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2]}}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return Dual{a.v - b.v, {a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2]}}; }
__device__ __forceinline__ Dual operator-(Dual a) { return Dual{-a.v, {-a.d[0], -a.d[1], -a.d[2]}}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b)
{
    return Dual{a.v * b.v, {a.d[0] * b.v + a.v * b.d[0], a.d[1] * b.v + a.v * b.d[1], a.d[2] * b.v + a.v * b.d[2]}};
}
__device__ __forceinline__ Dual operator/(Dual a, Dual b)
{
    const double q = a.v / b.v;
    return Dual{q, {(a.d[0] - q * b.d[0]) / b.v, (a.d[1] - q * b.d[1]) / b.v, (a.d[2] - q * b.d[2]) / b.v}};
}
__device__ __forceinline__ Dual operator/(Dual a, double c) { return Dual{a.v / c, {a.d[0] / c, a.d[1] / c, a.d[2] / c}}; }
__device__ __forceinline__ Dual operator*(double c, Dual a) { return Dual{c * a.v, {c * a.d[0], c * a.d[1], c * a.d[2]}}; }
__device__ __forceinline__ Dual dsqrt(Dual a)
{
    const double r = sqrt(a.v), k = 0.5 / r;
    return Dual{r, {k * a.d[0], k * a.d[1], k * a.d[2]}};
}
__device__ __forceinline__ Dual dsin(Dual a)
{
    const double c = cos(a.v);
    return Dual{sin(a.v), {c * a.d[0], c * a.d[1], c * a.d[2]}};
}
__device__ __forceinline__ Dual dcos(Dual a)
{
    const double s = -sin(a.v);
    return Dual{cos(a.v), {s * a.d[0], s * a.d[1], s * a.d[2]}};
}

// exponential_map, angular_distance_taylor.py:30-66 (EPS = 1e-2 on theta^2)
__device__ inline void exp_map(const Dual ax[3], Dual R[3][3])
{
    const Dual zero = dconst(0.0);
    Dual ss[3][3] = {{zero, -ax[2], ax[1]}, {ax[2], zero, -ax[0]}, {-ax[1], ax[0], zero}};
    const Dual tsq = (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2];
    Dual t1, t2;
    if (tsq.v < 1e-2) {
        const Dual p4 = tsq * tsq, p6 = (tsq * tsq) * tsq, p8 = ((tsq * tsq) * tsq) * tsq;
        t1 = (((dconst(1.0) - (tsq / 6.0)) + (p4 / 120.0)) - (p6 / 5040.0)) + (p8 / 362880.0);
        t2 = (((dconst(0.5) - (tsq / 24.0)) + (p4 / 720.0)) - (p6 / 40320.0)) + (p8 / 3628800.0);
    } else {
        const Dual th = dsqrt(tsq);
        t1 = dsin(th) / th;
        t2 = (dconst(1.0) - dcos(th)) / tsq;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Dual sq = zero;
            for (int k = 0; k < 3; ++k)
                sq = sq + ss[i][k] * ss[k][j];
            R[i][j] = (dconst(i == j ? 1.0 : 0.0) + t1 * ss[i][j]) + t2 * sq;
        }
}

} // namespace cloudaae
