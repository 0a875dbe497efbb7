// Forward-mode dual number (value + 3 partials) with the operations srrot::rodrigues needs: instantiating rodrigues<Dual> on
// (theta_x, theta_y, theta_z) seeded with the unit partials gives d R / d theta by the very arithmetic of the forward, the +1e-8 of the
// norm included.  Shared by the kinematic chain of csrc/lbs.hip and the pose adjoint of csrc/smpl_grad.hip.
#pragma once
#include "rot_device.h"

namespace srrot {
struct Dual {
  float v, d[3];
};
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return Dual{a.v + b.v, {a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2]}}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return Dual{a.v - b.v, {a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2]}}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) {
  return Dual{a.v * b.v, {a.d[0] * b.v + a.v * b.d[0], a.d[1] * b.v + a.v * b.d[1], a.d[2] * b.v + a.v * b.d[2]}};
}
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
  const float iv = 1.f / b.v, q = a.v * iv;
  return Dual{q, {(a.d[0] - q * b.d[0]) * iv, (a.d[1] - q * b.d[1]) * iv, (a.d[2] - q * b.d[2]) * iv}};
}
__device__ __forceinline__ Dual rot_sqrt(Dual a) { const float s = sqrtf(a.v), h = 0.5f / s; return Dual{s, {a.d[0] * h, a.d[1] * h, a.d[2] * h}}; }
__device__ __forceinline__ Dual rot_sin(Dual a) { const float s = sinf(a.v), c = cosf(a.v); return Dual{s, {a.d[0] * c, a.d[1] * c, a.d[2] * c}}; }
__device__ __forceinline__ Dual rot_cos(Dual a) { const float s = sinf(a.v), c = cosf(a.v); return Dual{c, {-a.d[0] * s, -a.d[1] * s, -a.d[2] * s}}; }
}  // namespace srrot
