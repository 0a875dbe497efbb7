// Wavefront reductions shared by the kernels of libselfrecon_hip.so: the xor butterfly over the 64 lanes of a wave (or over aligned
// groups of WIDTH lanes), distances WIDTH / 2 down to 1, own value combined with the fetched one.  Every lane ends with the result, and
// since a + b = b + a in IEEE arithmetic every lane ends with the same bits.  The shape is part of the stated summation order of the
// float and double callers: do not replace it by a DPP or a shuffle-down tree without re-recording their pins.
//
// Reductions of another shape stay with their kernels on purpose: lbs.hip's DPP wave_sum, icp.hip's __shfl_down tree, smpl_grad.hip's
// hand-folded 32 / 16 / 8 tree, and the scans of mc.hip, mjpeg.hip and shade.hip.
#pragma once
#include "sr_common.h"

template <typename T, int WIDTH = SR_WAVE>
__device__ __forceinline__ T sr_wave_sum(T v) {
#pragma unroll
  for (int s = WIDTH / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, WIDTH);
  return v;
}

template <typename T, int WIDTH = SR_WAVE>
__device__ __forceinline__ T sr_wave_min(T v) {
#pragma unroll
  for (int s = WIDTH / 2; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s, WIDTH));
  return v;
}

template <typename T, int WIDTH = SR_WAVE>
__device__ __forceinline__ T sr_wave_max(T v) {
#pragma unroll
  for (int s = WIDTH / 2; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, WIDTH));
  return v;
}
