// depth_fit.h -- what the counting kernel (depth_fit.hip) shares with the kernels that read its counters
// (select_pose_kernel of pose_verify.hip, detect_assign_kernel of detect.hip): the layout of counts [.., 6] and the score
// formed from it.  DESIGN.md, "Pose verification": "Counts" and "Selection".
#pragma once

namespace cloudaae {

constexpr int DF_COUNTERS = 6;                     // rendered, consistent, in_front, behind, unknown, explained

// num and den of one hypothesis from its counters c (0 / 1 for "no score", and for a hypothesis that is not usable): the
// segment rule (mode 0) or the silhouette rule (mode 1)
__device__ __forceinline__ void df_fraction(const int *c, int seg_total, bool usable, int mode, long long &num, long long &den)
{
    if (mode == 0) {
        num = c[5];
        den = (long long)seg_total + c[2];
    } else {
        num = c[1];
        den = ((long long)c[1] + c[2]) + c[3];
    }
    if (den <= 0 || num < 0 || !usable) {
        num = 0;
        den = 1;
    }
}

} // namespace cloudaae
