// pose_math.h -- the fp64 pose arithmetic shared by icp.hip, pose_score.hip and pose_equiv.hip (plain code,
// host-callable).
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

// Axis-angle of a rotation matrix, theta in [0, pi].  theta = atan2(|v|, tr - 1) with v the skew part (|v| = 2 sin,
// tr - 1 = 2 cos): accurate at both ends.  Away from pi the axis is v / |v| (rot = v * theta / |v|, which tends to v / 2
// as theta -> 0); near pi (cos < -0.5) it is the largest column of the symmetric part (R + R^T) / 2 - cos I =
// (1 - cos) a a^T, signed to agree with v.
__host__ __device__ inline void icp_log_map(const double *R, double *r)
{
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double tr1 = (R[0] + R[4] + R[8]) - 1.0;
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    const double theta = atan2(vn, tr1);
    if (tr1 > -1.0) {                       // cos theta > -0.5
        const double f = vn > 0.0 ? theta / vn : 0.5;
        r[0] = vx * f;
        r[1] = vy * f;
        r[2] = vz * f;
        return;
    }
    const double cs = 0.5 * tr1;
    const double b01 = 0.5 * (R[1] + R[3]), b02 = 0.5 * (R[2] + R[6]), b12 = 0.5 * (R[5] + R[7]);
    const double b00 = R[0] - cs, b11 = R[4] - cs, b22 = R[8] - cs;
    double ax = b00, ay = b01, az = b02;
    if (b11 > b00 && b11 >= b22) {
        ax = b01;
        ay = b11;
        az = b12;
    } else if (b22 > b00 && b22 > b11) {
        ax = b02;
        ay = b12;
        az = b22;
    }
    const double an = sqrt((ax * ax + ay * ay) + az * az);
    if (!(an > 0.0)) {
        ax = 1.0;
        ay = az = 0.0;
    } else {
        ax /= an;
        ay /= an;
        az /= an;
    }
    if ((ax * vx + ay * vy) + az * vz < 0.0) {
        ax = -ax;
        ay = -ay;
        az = -az;
    }
    r[0] = ax * theta;
    r[1] = ay * theta;
    r[2] = az * theta;
}
