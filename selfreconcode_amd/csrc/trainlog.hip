// Device-side training log: one row of scalars per iteration, gathered into a float32 ring in device memory (see sr_log_row in the
// header).  The reference prints ~15 loss values per iteration through .item(), each a wait for the whole stream; here the values
// stay where they were computed and ONE launch of one wave copies them into the ring, in stream order behind their producers.
//   log_row_kernel: lane k < n loads its source (a device float32 as its bits, a device int64 converted with (float), an immediate
//     that travelled inside the launch, or nothing) and stores one dword; lanes n <= k < ld store NaN.  A row wider than a wave is
//     covered by a stride-64 loop.  The slot table (416 bytes) is a kernel argument: no upload, no synchronisation.
// No atomics, no LDS, no scratch: bit-identical call to call.
#include "sr_common.h"

__global__ __launch_bounds__(SR_WAVE) void log_row_kernel(sr_log_slots slots, int n, float* __restrict__ dst, int ld) {
  const uint32_t nan_bits = 0x7fc00000u;
  uint32_t* out = reinterpret_cast<uint32_t*>(dst);
  for (int k = threadIdx.x; k < ld; k += SR_WAVE) {
    uint32_t bits = nan_bits;
    if (k < n) {
      const int kind = slots.kind[k];
      if (kind == SR_LOG_F32)
        bits = *reinterpret_cast<const uint32_t*>(slots.src[k]);              // bit for bit: a NaN keeps its payload, -0 its sign
      else if (kind == SR_LOG_I64)
        bits = __float_as_uint((float)*reinterpret_cast<const int64_t*>(slots.src[k]));
      else if (kind == SR_LOG_IMM)
        bits = __float_as_uint(slots.imm[k]);
    }
    out[k] = bits;
  }
}

extern "C" int sr_log_row(const sr_log_slots* slots_by_value, int32_t n, float* ring, int32_t ring_rows, int32_t ld, int64_t row,
                          void* stream) {
  if (!slots_by_value || !ring || ((uintptr_t)ring & 3)) return SR_EINVAL;
  if (n < 1 || n > SR_LOG_MAX_SLOTS || ld < n || ring_rows < 1 || row < 0) return SR_EINVAL;
  sr_log_slots slots = {};
  for (int k = 0; k < n; ++k) {                                               // (only the first n slots are read, here and in the kernel)
    const uint8_t kind = slots_by_value->kind[k];
    const void* src = slots_by_value->src[k];
    if (kind == SR_LOG_F32) {
      if (!src || ((uintptr_t)src & 3)) return SR_EINVAL;
    } else if (kind == SR_LOG_I64) {
      if (!src || ((uintptr_t)src & 7)) return SR_EINVAL;
    } else if (kind != SR_LOG_EMPTY && kind != SR_LOG_IMM) {
      return SR_EINVAL;
    }
    slots.kind[k] = kind;
    slots.src[k] = (kind == SR_LOG_F32 || kind == SR_LOG_I64) ? src : nullptr;
    slots.imm[k] = kind == SR_LOG_IMM ? slots_by_value->imm[k] : 0.f;
  }
  float* dst = ring + (row % ring_rows) * (int64_t)ld;
  hipLaunchKernelGGL(log_row_kernel, dim3(1), dim3(SR_WAVE), 0, (hipStream_t)stream, slots, (int)n, dst, (int)ld);
  return sr_launch_status();
}
