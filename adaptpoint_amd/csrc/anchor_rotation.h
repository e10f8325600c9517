// anchor_rotation.h -- the per-anchor rotation shared by the AdaptPoint augmentor (augment.hip) and PointWOLF
// (online_aug.hip): both compose R from the sines and cosines of three angles exactly as the reference does
// (generator_component4_15.py:288-290, pointwolf.py:142-144; its centre entry is sz sy sx + cz cy).
#pragma once
#include <hip/hip_runtime.h>

namespace apn {

struct AnchorTerms {
    float th[3], sg[3], tt[3];       // tanh(p0..2), sigmoid(p3..5), tanh(p6..8)
    float sn[3], cs[3];              // sin / cos of the angles (x, y, z)
    float s[3];
    bool unit[3];                    // the scale was 0 and became 1
};

__device__ __forceinline__ void anchor_rotation(const AnchorTerms &a, float (&R)[9]) {
    const float sx = a.sn[0], sy = a.sn[1], sz = a.sn[2], cx = a.cs[0], cy = a.cs[1], cz = a.cs[2];
    R[0] = cz * cy; R[1] = cz * sy * sx - sz * cx; R[2] = cz * sy * cx + sz * sx;
    R[3] = sz * cy; R[4] = sz * sy * sx + cz * cy; R[5] = sz * sy * cx - cz * sx;
    R[6] = -sy;     R[7] = cy * sx;                R[8] = cy * cx;
}

}  // namespace apn
