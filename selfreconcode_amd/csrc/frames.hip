// Frames of a capture sequence, resident on the GPU as the bytes the image files hold, expanded into the float tensors of one batch
// (dataset/dataset.py:85-115 of the reference: __getitem__ + the loader's collate, without the decode and the upload).
//   frames_fetch_kernel: one lane per 16-byte chunk of a stored frame.  blockIdx.y is the batch slot, blockIdx.z the plane (0 img,
//     1 normal, 2 mask), both wave-uniform; blockIdx.x strides over the chunks.  A lane reads its chunk with one 16-byte load (every
//     frame starts 16-byte aligned: the frame pitch is a multiple of 16), converts the 16 bytes and writes 16 floats -- four 16-byte
//     stores when the output frames are 16-byte aligned (H W % 4 == 0 and aligned bases), dword stores otherwise and in the chunk
//     that holds the frame's tail.  The bytes of the padding behind a frame are loaded with the last chunk and never converted.
//     The normal's channel reversal (output float o of a frame reads byte o + 2 - 2 (o % 3)) reaches up to two bytes into either
//     neighbouring chunk: the lane also loads the dword before and the dword behind its chunk (both inside the frame's pitch, both
//     cache hits) and picks each byte from that 24-byte window with static shifts, selected by the chunk's phase c % 3.
// Arithmetic: the reference's float32 expressions with IEEE division (the default of hipcc for device code: no fast-math on this
// file), contraction off.  Multiplying by a float32 1/255 instead is wrong for 111 of the 256 byte values.
// No atomics, no LDS, no scratch: bit-identical call to call.
#include "sr_common.h"

#pragma clang fp contract(off)

#define FRAMES_BLOCK 256

__device__ __forceinline__ float frames_img_value(uint32_t b) { return ((float)b / 255.f - 0.5f) * 2.f; }      // dataset.py:88
__device__ __forceinline__ float frames_normal_value(uint32_t b) { return (2.f * (float)b) / 255.f - 1.f; }     // dataset.py:102

template <int J>
__device__ __forceinline__ uint32_t frames_window_byte(const uint32_t (&w)[6]) {
  return (w[J >> 2] >> (8 * (J & 3))) & 0xffu;
}

// output k of a chunk with phase ph = c % 3 reads window byte k + 6 - 2 ((ph + k) % 3); the window starts 4 bytes before the chunk
template <int K>
__device__ __forceinline__ float frames_normal_at(const uint32_t (&w)[6], int ph) {
  const uint32_t b0 = frames_window_byte<K + 6 - 2 * (K % 3)>(w);
  const uint32_t b1 = frames_window_byte<K + 6 - 2 * ((K + 1) % 3)>(w);
  const uint32_t b2 = frames_window_byte<K + 6 - 2 * ((K + 2) % 3)>(w);
  return frames_normal_value(ph == 0 ? b0 : (ph == 1 ? b1 : b2));
}

template <int K>
struct frames_normal_fill {
  static __device__ __forceinline__ void run(const uint32_t (&w)[6], int ph, float (&v)[16]) {
    v[K] = frames_normal_at<K>(w, ph);
    frames_normal_fill<K + 1>::run(w, ph, v);
  }
};
template <>
struct frames_normal_fill<16> {
  static __device__ __forceinline__ void run(const uint32_t (&)[6], int, float (&)[16]) {}
};

template <bool ALIGNED>
__global__ __launch_bounds__(FRAMES_BLOCK) void frames_fetch_kernel(const uint8_t* __restrict__ img_u8, const uint8_t* __restrict__ normal_u8,
                                                                    const uint8_t* __restrict__ mask_u8, int64_t pitch3, int64_t pitch1, int F,
                                                                    int64_t hw, sr_frame_ids ids, const int64_t* __restrict__ ids_device,
                                                                    float* __restrict__ out_img, float* __restrict__ out_normal,
                                                                    float* __restrict__ out_mask) {
  const int n = blockIdx.y, plane = blockIdx.z;
  if (plane == 1 && !normal_u8) return;
  const int64_t f = ids_device ? ids_device[n] : (int64_t)ids.id[n];
  const bool valid = f >= 0 && f < (int64_t)F;
  const int64_t len = plane == 2 ? hw : 3 * hw;                  // bytes of a stored frame = floats of an output frame
  const int64_t pitch = plane == 2 ? pitch1 : pitch3;
  const uint8_t* src = (plane == 0 ? img_u8 : (plane == 1 ? normal_u8 : mask_u8)) + (valid ? f : 0) * pitch;
  float* dst = (plane == 0 ? out_img : (plane == 1 ? out_normal : out_mask)) + (int64_t)n * len;
  const int chunks = (int)((len + 15) / 16);
  const float bad = plane == 2 ? 0.f : __builtin_nanf("");       // a frame id outside [0, F): nothing is read

  for (int c = blockIdx.x * FRAMES_BLOCK + threadIdx.x; c < chunks; c += gridDim.x * FRAMES_BLOCK) {
    const int64_t o = 16 * (int64_t)c;
    float v[16];
    if (!valid) {
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = bad;
    } else {
      const uint4 q = *reinterpret_cast<const uint4*>(src + o);  // o + 16 <= pitch: pitch is a multiple of 16 and >= len
      if (plane == 1) {
        uint32_t w[6];
        w[0] = c > 0 ? *reinterpret_cast<const uint32_t*>(src + o - 4) : 0u;
        w[1] = q.x; w[2] = q.y; w[3] = q.z; w[4] = q.w;
        w[5] = o + 16 < pitch ? *reinterpret_cast<const uint32_t*>(src + o + 16) : 0u;
        frames_normal_fill<0>::run(w, c % 3, v);
      } else {
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
          v[k] = plane == 0 ? frames_img_value(b) : (float)b;
        }
      }
    }
    if (ALIGNED && o + 16 <= len) {
      float4* d4 = reinterpret_cast<float4*>(dst + o);
#pragma unroll
      for (int j = 0; j < 4; ++j) d4[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
      const int cnt = (int)(len - o < 16 ? len - o : 16);          // the frame's tail: the padding is never written out
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < cnt) dst[o + k] = v[k];
    }
  }
}

extern "C" int sr_frames_fetch(const uint8_t* img_u8, const uint8_t* normal_u8, const uint8_t* mask_u8, int64_t pitch3, int64_t pitch1, int32_t F,
                               int32_t H, int32_t W, const sr_frame_ids* ids_by_value, const int64_t* ids_device, int32_t N, float* out_img,
                               float* out_normal, float* out_mask, void* stream) {
  if (!img_u8 || !mask_u8 || !out_img || !out_mask || (normal_u8 == nullptr) != (out_normal == nullptr)) return SR_EINVAL;
  if ((ids_by_value == nullptr) == (ids_device == nullptr)) return SR_EINVAL;
  if (F < 1 || H < 1 || W < 1 || N < 1 || N > 65535 || (ids_by_value && N > SR_FRAMES_MAX_BATCH)) return SR_EINVAL;
  const int64_t hw = (int64_t)H * W;
  if (hw > SR_FRAMES_MAX_PIXELS) return SR_EINVAL;
  if (pitch3 % 16 || pitch1 % 16 || pitch3 < 3 * hw || pitch1 < hw) return SR_EINVAL;
  if (((uintptr_t)img_u8 | (uintptr_t)normal_u8 | (uintptr_t)mask_u8) & 15) return SR_EINVAL;
  if (((uintptr_t)out_img | (uintptr_t)out_normal | (uintptr_t)out_mask) & 3) return SR_EINVAL;
  sr_frame_ids ids = {};
  if (ids_by_value) ids = *ids_by_value;
  const bool aligned = hw % 4 == 0 && ((((uintptr_t)out_img | (uintptr_t)out_normal | (uintptr_t)out_mask) & 15) == 0);
  const dim3 grid((unsigned)sr_stream_grid(sr_cdiv(3 * hw, 16), FRAMES_BLOCK), (unsigned)N, 3), block(FRAMES_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  if (aligned)
    hipLaunchKernelGGL((frames_fetch_kernel<true>), grid, block, 0, s, img_u8, normal_u8, mask_u8, pitch3, pitch1, F, hw, ids, ids_device, out_img,
                       out_normal, out_mask);
  else
    hipLaunchKernelGGL((frames_fetch_kernel<false>), grid, block, 0, s, img_u8, normal_u8, mask_u8, pitch3, pitch1, F, hw, ids, ids_device, out_img,
                       out_normal, out_mask);
  return sr_launch_status();
}
