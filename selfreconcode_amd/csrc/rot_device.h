// Axis-angle -> rotation matrix (row major) through the half-angle quaternion, +1e-8 inside the norm (smpl_pytorch/util.py:35-78), on a
// scalar type S: float, or the forward-mode dual number of rot_dual.h with its own rot_sqrt / rot_sin / rot_cos and S{constant}.
#pragma once
#include "sr_common.h"

namespace srrot {
__device__ __forceinline__ float rot_sqrt(float a) { return sqrtf(a); }
__device__ __forceinline__ float rot_sin(float a) { return sinf(a); }
__device__ __forceinline__ float rot_cos(float a) { return cosf(a); }

template <typename S>
__device__ __forceinline__ void rodrigues(S tx, S ty, S tz, S (&R)[9]) {
  const S e = S{1e-8f};
  const S ax = tx + e, ay = ty + e, az = tz + e;
  const S angle = rot_sqrt(ax * ax + ay * ay + az * az);
  const S nx = tx / angle, ny = ty / angle, nz = tz / angle;
  const S half = angle * S{0.5f};
  const S qw0 = rot_cos(half), sh = rot_sin(half);
  const S qx0 = sh * nx, qy0 = sh * ny, qz0 = sh * nz;
  const S qn = rot_sqrt(qw0 * qw0 + qx0 * qx0 + qy0 * qy0 + qz0 * qz0);
  const S w = qw0 / qn, x = qx0 / qn, y = qy0 / qn, z = qz0 / qn;
  const S w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  const S wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
  const S two = S{2.f};
  R[0] = w2 + x2 - y2 - z2; R[1] = two * xy - two * wz; R[2] = two * wy + two * xz;
  R[3] = two * wz + two * xy; R[4] = w2 - x2 + y2 - z2; R[5] = two * yz - two * wx;
  R[6] = two * xz - two * wy; R[7] = two * wx + two * yz; R[8] = w2 - x2 - y2 + z2;
}
}  // namespace srrot
