// Baseline JPEG (SOF0, YCbCr 4:2:0, one restart interval per MCU row) of uint8 RGB frames that are already on the GPU: the entropy-coded
// bytes of a batch, ready for the host to put between its header segments and EOI (see sr_jpeg_* in the header).  All
// arithmetic is integer, so the stream has one right answer; tests/_jpeg_ref.py restates it in numpy.
//   jpeg_transform_kernel: one wave per MCU (four per workgroup).  Lane (qy, qx) converts the 2 x 2 pixels of its quad (clamped to the
//     last row / column: the padding), writes four Y samples and the quad's averaged Cb and Cr into LDS; 48 lanes then run the 8-point
//     DCT along the rows of the six blocks, 48 along the columns, quantise and place the value at its zigzag position; the wave writes
//     the MCU's 384 int16 as 192 dwords.  RGB is read once, 3 B/pixel in and 3 B/pixel out.
//   jpeg_entropy_kernel: one workgroup per (MCU row, frame) = one restart interval.  Tile by tile of 256 blocks: each thread counts the
//     bits of its block (DC difference against the previous block of its component, found in the coefficients -- no serial chain), a
//     workgroup scan turns the counts into bit offsets, and the thread ORs its codes into the interval's zeroed big-endian bit buffer in
//     global memory (a worst-case interval does not fit in LDS).  The tail is padded with 1s.  Then, tile by tile of 4 KiB, each thread
//     counts the 0xFF among its 16 bytes, a second scan gives where its bytes land, and it writes them with a 0x00 after each 0xFF.
//   jpeg_offsets_kernel: one workgroup scans the interval lengths of all frames into each interval's place in the output and offsets[B+1].
//   jpeg_gather_kernel: one workgroup per interval copies its bytes there, behind its RSTm marker.
// Capacities are worst cases that hold for every input (SR_JPEG_BLOCK_BYTES), checked on the host before anything is launched: no
// kernel can write past a buffer.  The atomics are ORs into zeroed words: two calls give identical bytes.
#include "sr_common.h"

#define JPEG_THREADS 256
#define JPEG_BLOCK_DWORDS (SR_JPEG_BLOCK_BYTES / 4)

// C[u][x] = round(8192 c(u) / 2 cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt 2
__constant__ int JPEG_DCT[64] = {
    2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896,
    4017, 3406, 2276, 799, -799, -2276, -3406, -4017,
    3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784,
    3406, -799, -4017, -2276, 2276, 4017, 799, -3406,
    2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896,
    2276, -4017, 799, 3406, -3406, -799, 4017, -2276,
    1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567,
    799, -2276, 3406, -4017, 4017, -3406, 2276, -799};

// zigzag position of each natural (row-major) index
__constant__ uint8_t JPEG_ZIGZAG_POS[64] = {
    0, 1, 5, 6, 14, 15, 27, 28,
    2, 4, 7, 13, 16, 26, 29, 42,
    3, 8, 12, 17, 25, 30, 41, 43,
    9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54,
    20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61,
    35, 36, 48, 49, 57, 58, 62, 63};

static inline int64_t jpeg_rows(int32_t H) { return (H + 15) / 16; }
static inline int64_t jpeg_mpr(int32_t W) { return (W + 15) / 16; }
// dwords of one interval's bit buffer: its blocks' worst case, rounded up to whole 128-byte lines so that no line is shared by two workgroups
static inline int64_t jpeg_bits_stride(int64_t mpr) { return (mpr * 6 * JPEG_BLOCK_DWORDS + 31) / 32 * 32; }
static inline int64_t jpeg_row_stride(int64_t mpr) { return mpr * 6 * SR_JPEG_BLOCK_BYTES * 2; }

static inline bool jpeg_shape_ok(int32_t B, int32_t H, int32_t W) {
  return B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_transform_kernel(const uint8_t* __restrict__ rgb, int H, int W, int rows, int mpr,
                                                                      int64_t total, const uint16_t* __restrict__ qtab,
                                                                      int16_t* __restrict__ coef) {
  __shared__ int16_t px[4][6][64];
  __shared__ int32_t tmp[4][6][64];
  __shared__ int16_t outz[4][384];
  __shared__ uint16_t q[128];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < 128) q[tid] = qtab[tid];
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  const bool live = g < total;
  if (live) {
    const int64_t per = (int64_t)rows * mpr;
    const int64_t b = g / per;
    const int rem = (int)(g - b * per), r = rem / mpr, m = rem - r * mpr;
    const int qy = lane >> 3, qx = lane & 7;
    int cb = 0, cr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int yy = 2 * qy + dy, xx = 2 * qx + dx;
        const int y = min(r * 16 + yy, H - 1), x = min(m * 16 + xx, W - 1);
        const uint8_t* p = rgb + ((b * H + y) * (int64_t)W + x) * 3;
        const int R = p[0], G = p[1], Bl = p[2];
        const int Y = (19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16;
        cb += (-11059 * R - 21709 * G + 32768 * Bl + (128 << 16) + 32767) >> 16;
        cr += (32768 * R - 27439 * G - 5329 * Bl + (128 << 16) + 32767) >> 16;
        px[wave][(yy >> 3) * 2 + (xx >> 3)][(yy & 7) * 8 + (xx & 7)] = (int16_t)(Y - 128);
      }
    }
    px[wave][4][lane] = (int16_t)(((cb + 2) >> 2) - 128);
    px[wave][5][lane] = (int16_t)(((cr + 2) >> 2) - 128);
  }
  __syncthreads();
  const int blk = lane >> 3, k = lane & 7;                 // lanes 0..47: (block, row) and then (block, column)
  if (live && lane < 48) {
    int s[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) s[x] = px[wave][blk][k * 8 + x];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int acc = 0;
#pragma unroll
      for (int x = 0; x < 8; ++x) acc += JPEG_DCT[u * 8 + x] * s[x];
      tmp[wave][blk][k * 8 + u] = (acc + 1024) >> 11;
    }
  }
  __syncthreads();
  if (live && lane < 48) {
    int t[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) t[y] = tmp[wave][blk][y * 8 + k];
    const uint16_t* qt = q + (blk >= 4 ? 64 : 0);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      int acc = 0;
#pragma unroll
      for (int y = 0; y < 8; ++y) acc += JPEG_DCT[v * 8 + y] * t[y];
      const int F = (acc + 16384) >> 15;
      const int zz = JPEG_ZIGZAG_POS[v * 8 + k];
      const int Q = qt[zz];
      int val = (abs(F) + (Q >> 1)) / Q;
      if (F < 0) val = -val;
      if (zz) val = max(-1023, min(1023, val));
      outz[wave][blk * 64 + zz] = (int16_t)val;
    }
  }
  __syncthreads();
  if (live) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(outz[wave]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(coef + g * 384);
    for (int i = lane; i < 192; i += SR_WAVE) dst[i] = src[i];
  }
}

// exclusive scan of one value per thread over the workgroup; `total` is the sum.  `waves` is JPEG_THREADS / SR_WAVE words of LDS.
__device__ inline uint32_t jpeg_scan(uint32_t v, uint32_t* waves, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < SR_WAVE; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d, SR_WAVE);
    if (lane >= d) inc += t;
  }
  if (lane == SR_WAVE - 1) waves[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < JPEG_THREADS / SR_WAVE; ++w) {
    if (w < wave) base += waves[w];
    total += waves[w];
  }
  __syncthreads();
  return base + inc - v;
}

struct JpegCount {
  uint32_t bits = 0;
  __device__ void put(uint32_t, int len) { bits += len; }
  __device__ void flush() {}
};

// MSB-first bit writer into zeroed 32-bit words whose most significant bit comes first in the stream; a word may be shared with the
// neighbouring blocks' threads, hence OR.
struct JpegEmit {
  uint32_t* word;
  uint64_t acc = 0;
  int n;
  __device__ JpegEmit(uint32_t* base, uint32_t bit) : word(base + (bit >> 5)), n(bit & 31) {}
  __device__ void put(uint32_t code, int len) {            // len <= 26, n < 32 on entry
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      atomicOr(word++, (uint32_t)(acc >> (n - 32)));
      n -= 32;
    }
  }
  __device__ void flush() {
    if (n) atomicOr(word, (uint32_t)(acc << (32 - n)));
  }
};

// One block's codes: the DC difference's category code and value bits, then (run, category) codes with value bits, ZRL for each 16
// zeros before a non-zero coefficient, EOB when the block ends in zeros.  huff entries are code | length << 16.
template <class Sink>
__device__ inline void jpeg_code_block(const int16_t* __restrict__ c, int pred, const uint32_t* dc, const uint32_t* ac, Sink& sink) {
  int run = 0;
  for (int j = 0; j < 8; ++j) {
    const uint4 v4 = *reinterpret_cast<const uint4*>(c + j * 8);
    const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = (int16_t)(w[i >> 1] >> ((i & 1) * 16));
      if (j == 0 && i == 0) {
        const int diff = v - pred, cat = diff ? 32 - __clz(abs(diff)) : 0;
        const uint32_t e = dc[cat];
        sink.put(((e & 0xffffu) << cat) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u)), (int)(e >> 16) + cat);
        continue;
      }
      if (v == 0) {
        ++run;
        continue;
      }
      while (run >= 16) {
        const uint32_t z = ac[0xF0];
        sink.put(z & 0xffffu, (int)(z >> 16));
        run -= 16;
      }
      const int cat = 32 - __clz(abs(v));
      const uint32_t e = ac[(run << 4) | cat];
      sink.put(((e & 0xffffu) << cat) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u)), (int)(e >> 16) + cat);
      run = 0;
    }
  }
  if (run) {
    const uint32_t e = ac[0];
    sink.put(e & 0xffffu, (int)(e >> 16));
  }
  sink.flush();
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, int rows, int mpr,
                                                                    const uint32_t* __restrict__ huff, uint32_t* __restrict__ bits,
                                                                    int64_t bits_stride, uint8_t* __restrict__ rowbuf, int64_t row_stride,
                                                                    uint32_t* __restrict__ row_len) {
  __shared__ uint32_t sh[1024];
  __shared__ uint32_t waves[JPEG_THREADS / SR_WAVE];
  const int tid = threadIdx.x;
  for (int i = tid; i < 1024; i += JPEG_THREADS) sh[i] = huff[i];
  __syncthreads();
  const int64_t interval = (int64_t)blockIdx.y * rows + blockIdx.x;
  const int nb = mpr * 6;
  const int16_t* crow = coef + interval * nb * 64;
  uint32_t* bw = bits + interval * bits_stride;
  uint8_t* orow = rowbuf + interval * row_stride;

  uint32_t nbits = 0;
  for (int base = 0; base < nb; base += JPEG_THREADS) {
    const int i = base + tid;
    const bool live = i < nb;
    int pred = 0;
    const uint32_t *dc = sh, *ac = sh + 512;
    uint32_t mine = 0;
    if (live) {
      const int m = i / 6, k = i - m * 6;
      int prev = -1;                                       // the previous block of this block's component in the interval
      if (k >= 1 && k <= 3) prev = i - 1;
      else if (m > 0) prev = k == 0 ? i - 3 : i - 6;
      if (prev >= 0) pred = crow[(int64_t)prev * 64];
      if (k >= 4) dc = sh + 256, ac = sh + 768;
      JpegCount count;
      jpeg_code_block(crow + (int64_t)i * 64, pred, dc, ac, count);
      mine = count.bits;
    }
    uint32_t total;
    const uint32_t at = nbits + jpeg_scan(mine, waves, total);
    if (live) {
      JpegEmit emit(bw, at);
      jpeg_code_block(crow + (int64_t)i * 64, pred, dc, ac, emit);
    }
    nbits += total;
  }
  if (tid == 0 && (nbits & 7)) {                           // pad the interval to a byte with 1s
    const int n = 8 - (nbits & 7);
    atomicOr(bw + (nbits >> 5), ((1u << n) - 1u) << (32 - (nbits & 31) - n));
  }
  __threadfence();
  __syncthreads();

  const uint32_t nbytes = (nbits + 7) >> 3;
  uint32_t stuffed = 0;
  for (uint32_t base = 0; base < nbytes; base += JPEG_THREADS * 16) {
    const uint32_t start = base + tid * 16;
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t ff = 0;
    if (start < nbytes) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (start + 4 * j < nbytes) w[j] = __hip_atomic_load(bw + (start >> 2) + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        ff += (start + j < nbytes) && ((w[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu) == 0xffu;
    }
    uint32_t total;
    uint32_t o = start + stuffed + jpeg_scan(ff, waves, total);
    if (start < nbytes) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (start + j < nbytes) {
          const uint32_t byte = (w[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu;
          orow[o++] = (uint8_t)byte;
          if (byte == 0xffu) orow[o++] = 0;
        }
      }
    }
    stuffed += total;
  }
  if (tid == 0) row_len[interval] = nbytes + stuffed;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_offsets_kernel(const uint32_t* __restrict__ row_len, int B, int rows,
                                                                    int64_t* __restrict__ row_start, int64_t* __restrict__ offsets) {
  __shared__ uint32_t waves[JPEG_THREADS / SR_WAVE];
  const int tid = threadIdx.x;
  int64_t at = 0;
  if (tid == 0) offsets[0] = 0;
  for (int b = 0; b < B; ++b) {
    for (int base = 0; base < rows; base += JPEG_THREADS) {
      const int r = base + tid;
      const uint32_t len = r < rows ? row_len[(int64_t)b * rows + r] + (r ? 2u : 0u) : 0u;      // a marker in front of every interval but the first
      uint32_t total;
      const uint32_t ex = jpeg_scan(len, waves, total);
      if (r < rows) row_start[(int64_t)b * rows + r] = at + ex + (r ? 2 : 0);
      at += total;
    }
    if (tid == 0) offsets[b + 1] = at;
  }
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_gather_kernel(const uint8_t* __restrict__ rowbuf, int64_t row_stride,
                                                                   const uint32_t* __restrict__ row_len, const int64_t* __restrict__ row_start,
                                                                   int rows, uint8_t* __restrict__ out) {
  const int r = blockIdx.x;
  const int64_t interval = (int64_t)blockIdx.y * rows + r;
  const uint8_t* src = rowbuf + interval * row_stride;
  uint8_t* dst = out + row_start[interval];
  const uint32_t n = row_len[interval];
  if (r && threadIdx.x < 2) dst[(int)threadIdx.x - 2] = threadIdx.x ? (uint8_t)(0xD0 + ((r - 1) & 7)) : (uint8_t)0xFF;
  for (uint32_t i = threadIdx.x; i < n; i += JPEG_THREADS) dst[i] = src[i];
}

extern "C" int sr_jpeg_transform(const uint8_t* rgb, int32_t B, int32_t H, int32_t W, const uint16_t* qtab, int16_t* coef, void* stream) {
  if (!rgb || !qtab || !coef || !jpeg_shape_ok(B, H, W) || ((uintptr_t)coef & 3)) return SR_EINVAL;
  const int64_t rows = jpeg_rows(H), mpr = jpeg_mpr(W), total = (int64_t)B * rows * mpr;
  if (sr_cdiv(total, 4) > INT32_MAX) return SR_EINVAL;
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)sr_cdiv(total, 4)), dim3(JPEG_THREADS), 0, (hipStream_t)stream, rgb, (int)H, (int)W,
                     (int)rows, (int)mpr, total, qtab, coef);
  return sr_launch_status();
}

extern "C" int sr_jpeg_entropy(const int16_t* coef, int32_t B, int32_t H, int32_t W, const uint32_t* huff, uint32_t* bits, int64_t bits_dwords,
                               uint8_t* rowbuf, int64_t rowbuf_bytes, uint32_t* row_len, void* stream) {
  if (!coef || !huff || !bits || !rowbuf || !row_len || !jpeg_shape_ok(B, H, W)) return SR_EINVAL;
  if (((uintptr_t)coef & 15) || ((uintptr_t)bits & 127)) return SR_EINVAL;
  const int64_t rows = jpeg_rows(H), mpr = jpeg_mpr(W), intervals = (int64_t)B * rows;
  if (bits_dwords < intervals * jpeg_bits_stride(mpr) || rowbuf_bytes < intervals * jpeg_row_stride(mpr)) return SR_ENOSPC;
  if (hipMemsetAsync(bits, 0, (size_t)(intervals * jpeg_bits_stride(mpr)) * 4, (hipStream_t)stream) != hipSuccess) return SR_ELAUNCH;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)rows, (unsigned)B), dim3(JPEG_THREADS), 0, (hipStream_t)stream, coef, (int)rows, (int)mpr,
                     huff, bits, jpeg_bits_stride(mpr), rowbuf, jpeg_row_stride(mpr), row_len);
  return sr_launch_status();
}

extern "C" int sr_jpeg_gather(const uint8_t* rowbuf, const uint32_t* row_len, int32_t B, int32_t H, int32_t W, int64_t* row_start, uint8_t* out,
                              int64_t out_bytes, int64_t* offsets, void* stream) {
  if (!rowbuf || !row_len || !row_start || !out || !offsets || !jpeg_shape_ok(B, H, W)) return SR_EINVAL;
  const int64_t rows = jpeg_rows(H), mpr = jpeg_mpr(W);
  if (out_bytes < (int64_t)B * (rows * jpeg_row_stride(mpr) + 2 * (rows - 1))) return SR_ENOSPC;
  hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(JPEG_THREADS), 0, (hipStream_t)stream, row_len, (int)B, (int)rows, row_start, offsets);
  if (sr_launch_status() != SR_OK) return SR_ELAUNCH;
  hipLaunchKernelGGL(jpeg_gather_kernel, dim3((unsigned)rows, (unsigned)B), dim3(JPEG_THREADS), 0, (hipStream_t)stream, rowbuf, jpeg_row_stride(mpr),
                     row_len, row_start, (int)rows, out);
  return sr_launch_status();
}
