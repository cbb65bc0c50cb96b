// pose_math.h -- the fp64 pose arithmetic shared by icp.hip and pose_score.hip (plain code, host-callable).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// axangle2mat of transforms3d: theta = |r|, axis = r / theta normalised again, R = the Rodrigues form; theta = 0
// gives I (transforms3d divides by zero there).
__host__ __device__ inline void icp_rodrigues(double rx, double ry, double rz, double *R)
{
    const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
    if (!(theta > 0.0)) {
        for (int i = 0; i < 9; ++i)
            R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double x = rx / theta, y = ry / theta, z = rz / theta;
    const double nrm = sqrt((x * x + y * y) + z * z);
    x = x / nrm;
    y = y / nrm;
    z = z / nrm;
    const double c = cos(theta), s = sin(theta), C = 1.0 - c;
    const double xs = x * s, ys = y * s, zs = z * s;
    const double xC = x * C, yC = y * C, zC = z * C;
    const double xyC = x * yC, yzC = y * zC, zxC = z * xC;
    R[0] = x * xC + c;
    R[1] = xyC - zs;
    R[2] = zxC + ys;
    R[3] = xyC + zs;
    R[4] = y * yC + c;
    R[5] = yzC - xs;
    R[6] = zxC - ys;
    R[7] = yzC + xs;
    R[8] = z * zC + c;
}

// p = ((A00 x + A01 y) + A02 z) + A03, row by row (A is 3x4 row-major): the order of the definitions, no fma
__device__ __forceinline__ void icp_apply(const double *A, double x, double y, double z, double &px, double &py,
                                          double &pz)
{
    px = ((A[0] * x + A[1] * y) + A[2] * z) + A[3];
    py = ((A[4] * x + A[5] * y) + A[6] * z) + A[7];
    pz = ((A[8] * x + A[9] * y) + A[10] * z) + A[11];
}
