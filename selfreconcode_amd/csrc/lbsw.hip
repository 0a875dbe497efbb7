// Skinning-weight field of a body mesh (model/Deformer.py:235-284 of the reference: compute_lbswField + smooth_weights).
//   lbsw_knn_blend_kernel: one thread per voxel, brute force over the vertices.  The vertices are the same for every lane, so they are
//     read through wave-uniform (scalar) loads, four per trip.  The k best (squared distance, index) pairs live in registers as a
//     sorted list with static indexing only; the unrolled shift-insert runs only in trips where some lane of the wave beats its
//     current last entry.  The k selected distances are then recomputed in double from a double voxel centre (30 of 6890: free),
//     so the blend weights do not carry the float32 rounding of the centre.  Stores are one coalesced row per channel.
//   lbsw_smooth_kernel: one Jacobi step, one thread per voxel looping over the channels (the channel sum comes for free).
// No atomics, no LDS, no scratch: bit-identical call to call.
#include "sr_common.h"

#define LBSW_BLOCK 256

// sorted ascending by (d2, index): a later vertex (higher index) with an equal d2 never displaces an earlier one
template <int KMAX>
__device__ __forceinline__ void lbsw_insert(float (&bd)[KMAX], int (&bi)[KMAX], float d2, int v) {
#pragma unroll
  for (int j = KMAX - 1; j > 0; --j) {              // selects on values already in registers: no control flow
    const float a = bd[j - 1], b = bd[j];
    const int ia = bi[j - 1], ib = bi[j];
    const int keep = b > d2 ? v : ib;
    bi[j] = a > d2 ? ia : keep;
    bd[j] = __builtin_amdgcn_fmed3f(a, b, d2);      // a <= b: a if d2 < a, d2 if a <= d2 < b, else b
  }
  if (bd[0] > d2) { bd[0] = d2; bi[0] = v; }
}

template <int KMAX, int CH>
__global__ __launch_bounds__(LBSW_BLOCK, 4) void lbsw_knn_blend_kernel(const float* __restrict__ verts, const float* __restrict__ vws, int nv, int nj,
                                                                    int k, int W, int H, int D, float bminx, float bminy, float bminz,
                                                                    float bmaxx, float bmaxy, float bmaxz, int align_corners,
                                                                    float* __restrict__ field) {
  const int64_t N = (int64_t)W * H * D;
  const int64_t i = (int64_t)blockIdx.x * LBSW_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int w = (int)(i % W), h = (int)((i / W) % H), d = (int)(i / ((int64_t)W * H));
  // voxel centre (Deformer.py:259-264), in double
  const double ux = align_corners ? (double)w / (W - 1) : (w + 0.5) / W;
  const double uy = align_corners ? (double)h / (H - 1) : (h + 0.5) / H;
  const double uz = align_corners ? (double)d / (D - 1) : (d + 0.5) / D;
  const double cxd = ux * ((double)bmaxx - bminx) + bminx, cyd = uy * ((double)bmaxy - bminy) + bminy, czd = uz * ((double)bmaxz - bminz) + bminz;
  const float cx = (float)cxd, cy = (float)cyd, cz = (float)czd;

  float bd[KMAX];
  int bi[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) { bd[j] = __builtin_inff(); bi[j] = 0; }

  int v = 0;
  for (; v + 4 <= nv; v += 4) {
    const float* p = verts + 3 * (int64_t)v;          // wave-uniform address: scalar loads
    float q[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) q[t] = p[t];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float dx = cx - q[3 * t], dy = cy - q[3 * t + 1], dz = cz - q[3 * t + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < bd[KMAX - 1]) lbsw_insert<KMAX>(bd, bi, d2, v + t);
    }
  }
  for (; v < nv; ++v) {
    const float dx = cx - verts[3 * (int64_t)v], dy = cy - verts[3 * (int64_t)v + 1], dz = cz - verts[3 * (int64_t)v + 2];
    const float d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < bd[KMAX - 1]) lbsw_insert<KMAX>(bd, bi, d2, v);
  }

  // inverse-distance weights of the k nearest, distances clamped to [1e-4, 1] (Deformer.py:270-272)
  double sum = 0.;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < k) {
      const float* p = verts + 3 * (int64_t)bi[j];
      const double dx = cxd - p[0], dy = cyd - p[1], dz = czd - p[2];
      double dist = sqrt(dx * dx + dy * dy + dz * dz);
      dist = fmin(fmax(dist, 1e-4), 1.);
      bd[j] = (float)(1. / dist);
      sum += (double)bd[j];
    }
  }
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {                                   // (a single neighbour gets exactly 1)
    bd[j] = (float)((double)bd[j] / sum);
    bi[j] *= nj;                                                     // 32-bit row offsets: 64-bit row addresses would double the registers
  }

  for (int c = 0; c < nj; c += CH) {
    float acc[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[e] = 0.f;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j < k) {
        const float* r = vws + (uint32_t)(bi[j] + c);
        if (CH == 4) {
          const float4 x = *reinterpret_cast<const float4*>(r);
          acc[0] += bd[j] * x.x; acc[1 % CH] += bd[j] * x.y; acc[2 % CH] += bd[j] * x.z; acc[3 % CH] += bd[j] * x.w;
        } else {
          acc[0] += bd[j] * r[0];
        }
      }
      if (j % 8 == 7) __builtin_amdgcn_sched_barrier(0);      // at most 8 gathers in flight: 32 at once would cost the occupancy
    }
#pragma unroll
    for (int e = 0; e < CH; ++e) field[(int64_t)(c + e) * N + i] = acc[e];
  }
}

template <int KMAX>
static int lbsw_launch(const float* verts, const float* vws, int nv, int nj, int k, int W, int H, int D, const float* bmin, const float* bmax,
                       int align_corners, float* field, hipStream_t s) {
  const int64_t N = (int64_t)W * H * D;
  const dim3 grid((unsigned)sr_cdiv(N, LBSW_BLOCK)), block(LBSW_BLOCK);
  if (nj % 4 == 0 && ((uintptr_t)vws & 15) == 0)
    hipLaunchKernelGGL((lbsw_knn_blend_kernel<KMAX, 4>), grid, block, 0, s, verts, vws, nv, nj, k, W, H, D, bmin[0], bmin[1], bmin[2], bmax[0], bmax[1],
                       bmax[2], align_corners, field);
  else
    hipLaunchKernelGGL((lbsw_knn_blend_kernel<KMAX, 1>), grid, block, 0, s, verts, vws, nv, nj, k, W, H, D, bmin[0], bmin[1], bmin[2], bmax[0], bmax[1],
                       bmax[2], align_corners, field);
  return sr_launch_status();
}

extern "C" int sr_lbsw_knn_blend(const float* verts, const float* vert_ws, int64_t nv, int32_t nj, int32_t k, int32_t W, int32_t H, int32_t D,
                                 const float* bmin, const float* bmax, int32_t align_corners, float* field, void* stream) {
  if (!verts || !vert_ws || !bmin || !bmax || !field || nj < 1 || W < 1 || H < 1 || D < 1 || nv < 1 || nv * nj > INT32_MAX) return SR_EINVAL;
  if (k < 1 || k > SR_LBSW_MAX_K || k > nv) return SR_EINVAL;
  if (align_corners && (W < 2 || H < 2 || D < 2)) return SR_EINVAL;
  if (sr_cdiv((int64_t)W * H * D, LBSW_BLOCK) > INT32_MAX) return SR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (k <= 8) return lbsw_launch<8>(verts, vert_ws, (int)nv, nj, k, W, H, D, bmin, bmax, align_corners, field, s);
  if (k <= 16) return lbsw_launch<16>(verts, vert_ws, (int)nv, nj, k, W, H, D, bmin, bmax, align_corners, field, s);
  return lbsw_launch<32>(verts, vert_ws, (int)nv, nj, k, W, H, D, bmin, bmax, align_corners, field, s);
}

// ------------------------------------------------------------------------------------------------ smooth_weights, one step
__device__ __forceinline__ float lbsw_relaxed(const float* __restrict__ p, int64_t i, bool interior, int W, int64_t HW) {
  const float x = p[i];
  if (!interior) return x;
  const float mean = (p[i + HW] + p[i - HW] + p[i + W] + p[i - W] + p[i + 1] + p[i - 1]) / 6.0f;      // (the reference's order of terms)
  return (x - mean) * 0.7f + mean;
}

// NJ > 0: the channel count, values kept in registers; NJ = 0: any count, values recomputed for the second pass
template <int NJ>
__global__ __launch_bounds__(LBSW_BLOCK) void lbsw_smooth_kernel(const float* __restrict__ src, float* __restrict__ dst, int nj, int W, int H, int D) {
  const int64_t HW = (int64_t)W * H, N = HW * D;
  const int64_t i = (int64_t)blockIdx.x * LBSW_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int w = (int)(i % W), h = (int)((i / W) % H), d = (int)(i / HW);
  const bool interior = w > 0 && w < W - 1 && h > 0 && h < H - 1 && d > 0 && d < D - 1;
  float sum = 0.f;
  if (NJ > 0) {
    float val[NJ > 0 ? NJ : 1];
#pragma unroll
    for (int c = 0; c < NJ; ++c) { val[c] = lbsw_relaxed(src + c * N, i, interior, W, HW); sum += val[c]; }
#pragma unroll
    for (int c = 0; c < NJ; ++c) dst[c * N + i] = val[c] / sum;
  } else {
    for (int c = 0; c < nj; ++c) sum += lbsw_relaxed(src + c * N, i, interior, W, HW);
    for (int c = 0; c < nj; ++c) dst[c * N + i] = lbsw_relaxed(src + c * N, i, interior, W, HW) / sum;
  }
}

extern "C" int sr_lbsw_smooth(const float* src, float* dst, int32_t nj, int32_t W, int32_t H, int32_t D, void* stream) {
  if (!src || !dst || src == dst || nj < 1 || W < 1 || H < 1 || D < 1) return SR_EINVAL;
  const int64_t N = (int64_t)W * H * D;
  if (sr_cdiv(N, LBSW_BLOCK) > INT32_MAX) return SR_EINVAL;
  const dim3 grid((unsigned)sr_cdiv(N, LBSW_BLOCK)), block(LBSW_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  if (nj == 24)
    hipLaunchKernelGGL((lbsw_smooth_kernel<24>), grid, block, 0, s, src, dst, nj, W, H, D);
  else
    hipLaunchKernelGGL((lbsw_smooth_kernel<0>), grid, block, 0, s, src, dst, nj, W, H, D);
  return sr_launch_status();
}
