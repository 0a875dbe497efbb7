// Silhouette term of smpl_fit.py: the exact squared Euclidean distance transform of the masks, the contour flags the
// samples are compacted from, and the energy with its gradient.
//   edt_columns_kernel:    pass 1, one lane per (frame, column): two sweeps along y give g = the distance along the column to its nearest
//     mask pixel, EDT_GINF for a column without one.  Lanes are consecutive columns: every load and store is coalesced.
//   edt_rows_kernel:       pass 2, one workgroup per (frame, row), g^2 of the row in LDS.  Pixel x takes min_x' (x - x')^2 + g^2(x') by
//     the outward search k = 1, 2, ... that stops once k^2 >= best (lanes are consecutive x, so x - k and x + k are consecutive LDS
//     words: no bank conflict).  EDT_GINF^2 = SR_EDT_EMPTY, so a frame without a mask pixel holds the sentinel everywhere; a row whose
//     columns are all empty is written without a search.
//   contour_flags_kernel:  1 where a mask pixel has a 4-neighbour INSIDE the image that is background.
//   sil_project_kernel:    one lane per (frame, vertex): pixel position and validity (0: behind or non-finite, 1: in front but off the
//     image, 2: inside), written once for both terms; and the vertex's inside term (bilinear taps of sqrt(d2)): its value and its
//     gradient in the pixel position.
//   sil_match_kernel:      one lane per (frame, sample); the projected vertices pass through LDS in tiles of SIL_TILE; the nearest vertex
//     in front of the camera (ties: the lower index), the sample's residual value and its gradient at that vertex's pixel.
//   sil_grad_kernel:       one lane per (frame, vertex), SIL_GRAD_BLOCK vertices per workgroup.  A lane walks the frame's samples in
//     ascending order (staged through LDS, four matches per load) and adds the residual gradients of those matched to its vertex, then
//     chains that and the inside term's gradient through the projection.  One more workgroup per frame takes the frame's sums from
//     what the two launches before wrote: per lane ascending, the xor butterfly inside a wave, the waves in ascending order.
// No atomics; every loop is bounded by an integer fixed before it starts; two calls give identical bits.
#include "sr_common.h"
#include "sr_wave.h"

#define EDT_MAX_DIM 8192
#define EDT_GINF 32768                    // g of a column without a mask pixel; its square is SR_EDT_EMPTY
#define EDT_BLOCK 256
#define SIL_BLOCK 256
#define SIL_TILE 1024                     // projected vertices per LDS tile of the match launch
#define SIL_GRAD_BLOCK 256                // vertices per workgroup of the gradient launch
#define SIL_SAMPLE_TILE 2048              // samples per LDS tile of the gradient launch
#define SIL_MAX_SAMPLES 65536

static_assert((int64_t)EDT_GINF * EDT_GINF == SR_EDT_EMPTY, "an empty column squares to the sentinel");
static_assert((int64_t)SR_EDT_EMPTY + (int64_t)(EDT_MAX_DIM - 1) * (EDT_MAX_DIM - 1) < INT32_MAX, "pass 2 adds k^2 to g^2 in int32");
static_assert(SIL_SAMPLE_TILE % 4 == 0, "the walk reads four matches per LDS load");

struct sil_camera { float R[9], T[3], fx, fy, cx, cy; };

// ------------------------------------------------------------------------------------------------ distance transform
__global__ __launch_bounds__(EDT_BLOCK) void edt_columns_kernel(const uint8_t* __restrict__ mask, int H, int W, int32_t* __restrict__ g) {
  const int x = blockIdx.x * EDT_BLOCK + threadIdx.x, f = blockIdx.y;
  if (x >= W) return;
  const uint8_t* m = mask + (int64_t)f * H * W + x;
  int32_t* o = g + (int64_t)f * H * W + x;
  int d = EDT_GINF;
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    d = m[(int64_t)y * W] ? 0 : min(d + 1, EDT_GINF);
    o[(int64_t)y * W] = d;
  }
  d = EDT_GINF;
#pragma unroll 8
  for (int y = H - 1; y >= 0; --y) {
    const int down = o[(int64_t)y * W];
    d = down == 0 ? 0 : min(d + 1, EDT_GINF);
    o[(int64_t)y * W] = min(d, down);
  }
}

__global__ __launch_bounds__(EDT_BLOCK) void edt_rows_kernel(int H, int W, int32_t* __restrict__ d2) {
  __shared__ int32_t g2[EDT_MAX_DIM];
  __shared__ int any;
  const int y = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
  int32_t* row = d2 + ((int64_t)f * H + y) * W;
  if (t == 0) any = 0;
  __syncthreads();
  for (int x = t; x < W; x += EDT_BLOCK) {
    const int g = row[x];
    g2[x] = g * g;
    if (g < EDT_GINF) any = 1;                                  // (every writer stores the same value)
  }
  __syncthreads();
  const bool search = any != 0;
  for (int x = t; x < W; x += EDT_BLOCK) {
    int best = g2[x];
    const int reach = search ? max(x, W - 1 - x) : 0;
    for (int k = 1; k <= reach; ++k) {
      const int k2 = k * k;
      if (k2 >= best) break;
      if (x - k >= 0) best = min(best, k2 + g2[x - k]);
      if (x + k < W) best = min(best, k2 + g2[x + k]);
    }
    row[x] = best;
  }
}

extern "C" int sr_edt(const uint8_t* mask, int32_t F, int32_t H, int32_t W, int32_t* d2, void* stream) {
  if (!mask || !d2 || F < 1 || F > 65535 || H < 1 || W < 1 || H > EDT_MAX_DIM || W > EDT_MAX_DIM) return SR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(edt_columns_kernel, dim3((unsigned)sr_cdiv(W, EDT_BLOCK), (unsigned)F), dim3(EDT_BLOCK), 0, s, mask, H, W, d2);
  hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)H, (unsigned)F), dim3(EDT_BLOCK), 0, s, H, W, d2);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ contour flags
__global__ __launch_bounds__(EDT_BLOCK) void contour_flags_kernel(const uint8_t* __restrict__ mask, int H, int W, int64_t total,
                                                                  uint8_t* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * EDT_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * EDT_BLOCK) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    int c = 0;
    if (mask[i]) {
      if (x > 0 && !mask[i - 1]) c = 1;
      if (x < W - 1 && !mask[i + 1]) c = 1;
      if (y > 0 && !mask[i - W]) c = 1;
      if (y < H - 1 && !mask[i + W]) c = 1;
    }
    flag[i] = (uint8_t)c;
  }
}

extern "C" int sr_contour_flags(const uint8_t* mask, int32_t F, int32_t H, int32_t W, uint8_t* flags, void* stream) {
  if (!mask || !flags || F < 1 || H < 1 || W < 1 || H > EDT_MAX_DIM || W > EDT_MAX_DIM) return SR_EINVAL;
  const int64_t total = (int64_t)F * H * W;
  hipLaunchKernelGGL(contour_flags_kernel, dim3((unsigned)sr_stream_grid(total, EDT_BLOCK)), dim3(EDT_BLOCK), 0, (hipStream_t)stream, mask, H, W, total,
                     flags);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ the energy
__device__ __forceinline__ void sil_to_camera(const sil_camera& cam, const float* __restrict__ p, float& cx_, float& cy_, float& cz_) {
  const float px = p[0], py = p[1], pz = p[2];
  const float* R = cam.R;
  cx_ = fmaf(pz, R[6], fmaf(py, R[3], px * R[0])) + cam.T[0];
  cy_ = fmaf(pz, R[7], fmaf(py, R[4], px * R[1])) + cam.T[1];
  cz_ = fmaf(pz, R[8], fmaf(py, R[5], px * R[2])) + cam.T[2];
}

__global__ __launch_bounds__(SIL_BLOCK) void sil_project_kernel(const float* __restrict__ points, sil_camera cam, int64_t total, int V, int H, int W,
                                                                const int32_t* __restrict__ d2, float sigma, float* __restrict__ xy,
                                                                uint8_t* __restrict__ valid, float* __restrict__ vres) {
  const int64_t i = (int64_t)blockIdx.x * SIL_BLOCK + threadIdx.x;
  if (i >= total) return;
  float cx_, cy_, cz_;
  sil_to_camera(cam, points + i * 3, cx_, cy_, cz_);
  float x = 0.f, y = 0.f;
  int v = 0;
  if (cz_ > 0.f) {
    x = cam.cx - (cam.fx * cx_) / cz_;                            // (the order of RectifiedPerspectiveCameras.project)
    y = cam.cy - (cam.fy * cy_) / cz_;
    if (isfinite(x) && isfinite(y)) v = (x >= 0.f && x <= (float)(W - 1) && y >= 0.f && y <= (float)(H - 1)) ? 2 : 1;
  }
  if (v == 0) { x = 0.f; y = 0.f; }
  xy[2 * i] = x; xy[2 * i + 1] = y;
  valid[i] = (uint8_t)v;
  // the inside term of this vertex: its value and its gradient in the pixel position, the 1/V included
  float e = 0.f, igx = 0.f, igy = 0.f;
  const int32_t* field = d2 + (i / V) * ((int64_t)H * W);
  if (v == 2 && field[0] != SR_EDT_EMPTY) {                       // (a frame without a mask pixel has no inside term)
    const int x0 = min(max((int)floorf(x), 0), W - 2), y0 = min(max((int)floorf(y), 0), H - 2);
    const float fx = x - (float)x0, fy = y - (float)y0;
    const int32_t* tap = field + (int64_t)y0 * W + x0;
    const float d00 = sqrtf((float)tap[0]), d10 = sqrtf((float)tap[1]), d01 = sqrtf((float)tap[W]), d11 = sqrtf((float)tap[W + 1]);
    const float top = d00 + fx * (d10 - d00), bot = d01 + fx * (d11 - d01);
    const float d = top + fy * (bot - top);
    const float ddx = (d10 - d00) + fy * ((d11 - d01) - (d10 - d00)), ddy = bot - top;
    const float s2 = sigma * sigma, r2 = d * d, den = 1.f / (s2 + r2);
    e = s2 * r2 * den;
    const float w = 2.f * d * (s2 * den) * (s2 * den) / (float)V;   // d rho / d (r^2) * 2 d / V
    igx = w * ddx; igy = w * ddy;
  }
  vres[3 * i] = e; vres[3 * i + 1] = igx; vres[3 * i + 2] = igy;
}

__global__ __launch_bounds__(SIL_BLOCK) void sil_match_kernel(const float* __restrict__ xy, const uint8_t* __restrict__ valid,
                                                              const int32_t* __restrict__ samples, const int32_t* __restrict__ counts, float sigma,
                                                              float margin, int V, int S, int32_t* __restrict__ match, float* __restrict__ sres) {
  __shared__ float2 tile[SIL_TILE];
  const int t = blockIdx.y, s = blockIdx.x * SIL_BLOCK + threadIdx.x;
  const int n = min(max(counts[t], 0), S);
  const bool live = s < n;
  if (blockIdx.x * SIL_BLOCK >= n) {                             // (the whole workgroup: no sample of it is in use)
    if (s < S) {
      match[(int64_t)t * S + s] = -1;
      float* o = sres + ((int64_t)t * S + s) * 3;
      o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    }
    return;
  }
  float sx = 0.f, sy = 0.f;
  if (live) {
    sx = (float)samples[((int64_t)t * S + s) * 2];
    sy = (float)samples[((int64_t)t * S + s) * 2 + 1];
  }
  float best = INFINITY;
  int arg = -1;
  for (int v0 = 0; v0 < V; v0 += SIL_TILE) {
    const int m = min(SIL_TILE, V - v0);
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += SIL_BLOCK) {
      const int64_t i = (int64_t)t * V + v0 + j;
      tile[j] = valid[i] ? make_float2(xy[2 * i], xy[2 * i + 1]) : make_float2(INFINITY, INFINITY);
    }
    __syncthreads();
    if (live) {
#pragma unroll 16                                                 // (sixteen LDS reads in flight per wave instead of one)
      for (int j = 0; j < m; ++j) {                               // ascending vertex order, strict <: a tie keeps the lower index
        const float2 q = tile[j];
        const float dx = q.x - sx, dy = q.y - sy;
        const float d = dx * dx + dy * dy;
        if (d < best) { best = d; arg = v0 + j; }
      }
    }
  }
  if (s >= S) return;
  float e = 0.f, gx = 0.f, gy = 0.f;
  if (live && arg >= 0) {
    const int64_t i = (int64_t)t * V + arg;
    const float dist = sqrtf(best), r = dist - margin;
    if (r > 0.f) {                                                // (so dist > margin >= 0)
      const float s2 = sigma * sigma, den = 1.f / (s2 + r * r);
      e = s2 * (r * r) * den;
      const float w = 2.f * r * (s2 * den) * (s2 * den) / (dist * (float)n);
      gx = w * (xy[2 * i] - sx);
      gy = w * (xy[2 * i + 1] - sy);
    }
  }
  match[(int64_t)t * S + s] = live ? arg : -1;
  float* o = sres + ((int64_t)t * S + s) * 3;
  o[0] = e; o[1] = gx; o[2] = gy;
}

__global__ __launch_bounds__(SIL_GRAD_BLOCK) void sil_grad_kernel(const float* __restrict__ points,
                                                                  const uint8_t* __restrict__ valid, const float* __restrict__ vres,
                                                                  const int32_t* __restrict__ counts, const int32_t* __restrict__ match,
                                                                  const float* __restrict__ sres, sil_camera cam, int V, int S,
                                                                  int64_t term_stride, float* __restrict__ e_in, float* __restrict__ e_cov,
                                                                  int32_t* __restrict__ outside, float* __restrict__ g_points) {
  __shared__ __attribute__((aligned(16))) int32_t ms[SIL_SAMPLE_TILE];
  __shared__ float gxs[SIL_SAMPLE_TILE], gys[SIL_SAMPLE_TILE];
  __shared__ float wsum[2][SIL_GRAD_BLOCK / SR_WAVE];
  __shared__ int32_t wcnt[SIL_GRAD_BLOCK / SR_WAVE];
  const int t = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(counts[t], 0), S);
  const int nchunks = gridDim.x - 1, ntiles = (n + SIL_SAMPLE_TILE - 1) / SIL_SAMPLE_TILE;
  if ((int)blockIdx.x == nchunks) {
    // the frame's sums, from what the two launches before this one wrote: per lane ascending, butterfly, waves ascending
    float acc_in = 0.f, acc_cov = 0.f;
    int nout = 0;
    for (int v = tid; v < V; v += SIL_GRAD_BLOCK) {
      acc_in += vres[((int64_t)t * V + v) * 3];
      nout += valid[(int64_t)t * V + v] != 2;
    }
    for (int s = tid; s < n; s += SIL_GRAD_BLOCK) acc_cov += sres[((int64_t)t * S + s) * 3];
    acc_in = sr_wave_sum(acc_in); acc_cov = sr_wave_sum(acc_cov); nout = sr_wave_sum(nout);
    if ((tid & (SR_WAVE - 1)) == 0) { wsum[0][tid / SR_WAVE] = acc_in; wsum[1][tid / SR_WAVE] = acc_cov; wcnt[tid / SR_WAVE] = nout; }
    __syncthreads();
    if (tid == 0) {
      float a = 0.f, b = 0.f;
      int k = 0;
      for (int w = 0; w < SIL_GRAD_BLOCK / SR_WAVE; ++w) { a += wsum[0][w]; b += wsum[1][w]; k += wcnt[w]; }      // ascending wave order
      e_in[t] = a / (float)V;
      e_cov[t] = n > 0 ? b / (float)n : 0.f;
      outside[t] = k;
    }
    return;
  }
  {
    const int v = blockIdx.x * SIL_GRAD_BLOCK + tid;
    const bool has = v < V;
    float cgx = 0.f, cgy = 0.f;
    for (int tile = 0; tile < ntiles; ++tile) {
      const int s0 = tile * SIL_SAMPLE_TILE, m = min(SIL_SAMPLE_TILE, n - s0), m4 = (m + 3) & ~3;
      __syncthreads();                                            // (n is the frame's: uniform over the workgroup)
      for (int j = tid; j < m4; j += SIL_GRAD_BLOCK) {
        const int64_t i = (int64_t)t * S + s0 + j;
        ms[j] = j < m ? match[i] : -1;
        gxs[j] = j < m ? sres[i * 3 + 1] : 0.f;
        gys[j] = j < m ? sres[i * 3 + 2] : 0.f;
      }
      __syncthreads();
      if (has) {
#pragma unroll 4
        for (int j = 0; j < m4; j += 4) {                         // ascending sample order
          const int4 q = *reinterpret_cast<const int4*>(ms + j);
          if (q.x == v) { cgx += gxs[j]; cgy += gys[j]; }
          if (q.y == v) { cgx += gxs[j + 1]; cgy += gys[j + 1]; }
          if (q.z == v) { cgx += gxs[j + 2]; cgy += gys[j + 2]; }
          if (q.w == v) { cgx += gxs[j + 3]; cgy += gys[j + 3]; }
        }
      }
    }
    if (has) {
      const int64_t i = (int64_t)t * V + v;
      const int fl = valid[i];
      const float igx = vres[3 * i + 1], igy = vres[3 * i + 2];     // the inside term's gradient in the pixel position (launch 1)
      float gi[3] = {0.f, 0.f, 0.f}, gc[3] = {0.f, 0.f, 0.f};
      if (fl != 0) {
        float cx_, cy_, cz_;
        sil_to_camera(cam, points + i * 3, cx_, cy_, cz_);
        const float iz = 1.f / cz_;
        const float* R = cam.R;
        {
          const float c0 = -cam.fx * iz * igx, c1 = -cam.fy * iz * igy, c2 = (cam.fx * cx_ * igx + cam.fy * cy_ * igy) * iz * iz;
          gi[0] = fmaf(R[2], c2, fmaf(R[1], c1, R[0] * c0));
          gi[1] = fmaf(R[5], c2, fmaf(R[4], c1, R[3] * c0));
          gi[2] = fmaf(R[8], c2, fmaf(R[7], c1, R[6] * c0));
        }
        {
          const float c0 = -cam.fx * iz * cgx, c1 = -cam.fy * iz * cgy, c2 = (cam.fx * cx_ * cgx + cam.fy * cy_ * cgy) * iz * iz;
          gc[0] = fmaf(R[2], c2, fmaf(R[1], c1, R[0] * c0));
          gc[1] = fmaf(R[5], c2, fmaf(R[4], c1, R[3] * c0));
          gc[2] = fmaf(R[8], c2, fmaf(R[7], c1, R[6] * c0));
        }
      }
      float* o = g_points + i * 3;
      o[0] = gi[0]; o[1] = gi[1]; o[2] = gi[2];
      o[term_stride] = gc[0]; o[term_stride + 1] = gc[1]; o[term_stride + 2] = gc[2];
    }
  }
}

extern "C" int sr_silhouette_energy(const float* points, const int32_t* d2, const int32_t* samples, const int32_t* counts, const float* host_camera,
                                    float sigma, float margin, int32_t F, int32_t V, int32_t S, int32_t H, int32_t W, float* xy, uint8_t* valid,
                                    float* vres, int32_t* match, float* sres, float* e_in, float* e_cov, int32_t* outside, float* g_points,
                                    void* stream) {
  if (!points || !d2 || !samples || !counts || !host_camera || !xy || !valid || !vres || !match || !sres || !e_in || !e_cov || !outside || !g_points)
    return SR_EINVAL;
  if (F < 1 || F > 65535 || V < 1 || V > INT32_MAX / 4 || S < 1 || S > SIL_MAX_SAMPLES || H < 2 || W < 2 || H > EDT_MAX_DIM || W > EDT_MAX_DIM)
    return SR_EINVAL;
  if (!(sigma > 0.f) || !(margin >= 0.f)) return SR_EINVAL;
  sil_camera cam;
  for (int i = 0; i < 9; ++i) cam.R[i] = host_camera[i];
  for (int i = 0; i < 3; ++i) cam.T[i] = host_camera[9 + i];
  cam.fx = host_camera[12]; cam.fy = host_camera[13]; cam.cx = host_camera[14]; cam.cy = host_camera[15];
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)F * V;
  hipLaunchKernelGGL(sil_project_kernel, dim3((unsigned)sr_cdiv(total, SIL_BLOCK)), dim3(SIL_BLOCK), 0, s, points, cam, total, V, H, W, d2, sigma, xy, valid,
                     vres);
  hipLaunchKernelGGL(sil_match_kernel, dim3((unsigned)sr_cdiv(S, SIL_BLOCK), (unsigned)F), dim3(SIL_BLOCK), 0, s, xy, valid, samples, counts, sigma, margin,
                     V, S, match, sres);
  hipLaunchKernelGGL(sil_grad_kernel, dim3((unsigned)sr_cdiv(V, SIL_GRAD_BLOCK) + 1, (unsigned)F), dim3(SIL_GRAD_BLOCK), 0, s, points, valid, vres, counts,
                     match, sres, cam, V, S, total * 3, e_in, e_cov, outside, g_points);
  return sr_launch_status();
}
