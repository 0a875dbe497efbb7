// Pose conditioning: a deformer code for a pose that was never filmed, blended from the training frames whose poses
// are nearest in pose space.
//
//  * sr_pose_features: one thread per (pose, joint 1 .. 23): the nine entries of R_j - I, R_j from srrot::rodrigues as the body model's
//    forward takes it, times the joint's scale; stored feature-major so that the search reads consecutive poses from consecutive lanes.
//  * sr_pose_neighbors: one workgroup per tile of PC_QT queries, their features in the LDS.  Each thread strides over the candidates,
//    computes the tile's distances from one read of the candidate's feature and keeps, per query, its own K smallest as sorted 64-bit
//    keys (float bits of d2) << 32 | n in registers: K is a compile-time case (1, 2, 4, 8) and the insertion is fully unrolled, so no
//    index into the keys is a run-time value.  d2 >= 0, so the order of the keys is the order of (d2, n).  The merge is K rounds of a
//    workgroup minimum over every thread's smallest key (sr_wave_min across lanes, the LDS across waves); the thread that holds the
//    minimum drops it.  Keys of one query are distinct (n is), so exactly one thread does.
//  * sr_pose_dist: the witness.  The full distance matrix from the same device function, tile_d2, in the same tiling.  tile_d2 loads
//    PC_BATCH entries of a candidate's feature before it sums their terms: written entry by entry the compiler waits for each load
//    before the next is issued, and 207 exposed L2 latencies per candidate made both kernels 3 times slower.
//  * sr_code_blend: one thread per (query, code entry); every thread of a query recomputes its K weights in the same order.
//
// No atomics; every loop runs over an integer range fixed before it starts; a float comparison decides what a slot holds, never how
// long a loop runs.  Two calls give identical bits.
#include <cmath>
#include "posecond_abi.h"
#include "rot_device.h"
#include "sr_wave.h"

namespace {

#define PC_BLOCK 256
#define PC_WAVES (PC_BLOCK / SR_WAVE)
#define PC_QT 4                                         /* queries per workgroup */
#define PC_EMPTY 0xFFFFFFFFFFFFFFFFull                  /* no candidate: above every key (a NaN's bits with n = 2^32 - 1 never occur) */
#define PC_MAX_GRID 65536
#define PC_BATCH 23                                     /* feature entries loaded before their terms are summed: 207 = 9 * 23 */

__global__ __launch_bounds__(PC_BLOCK) void pose_features(const float* __restrict__ theta, int64_t N, const float* __restrict__ scale,
                                                           float* __restrict__ feat_t, int64_t ld) {
  const int64_t total = N * SR_POSE_JOINTS;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = i / N, n = i - j * N;              // joint j + 1 of pose n: consecutive lanes, consecutive n
    const float* t = theta + (n * 24 + j + 1) * 3;
    float R[9];
    srrot::rodrigues<float>(t[0], t[1], t[2], R);
    const float s = scale ? scale[j] : 1.f;
#pragma unroll
    for (int e = 0; e < 9; ++e) feat_t[(j * 9 + e) * ld + n] = (R[e] - ((e & 3) == 0 ? 1.f : 0.f)) * s;
  }
}

// The features of the tile's queries q0 .. q0 + PC_QT - 1 into the LDS, entry-major; zeros for a query >= Q.
__device__ __forceinline__ void stage_queries(float (*qs)[PC_QT], const float* __restrict__ featq_t, int64_t ldq, int64_t Q, int64_t q0) {
  for (int32_t s = threadIdx.x; s < SR_POSE_FEATS * PC_QT; s += PC_BLOCK) {
    const int32_t e = s / PC_QT, t = s - e * PC_QT;
    qs[e][t] = q0 + t < Q ? featq_t[(int64_t)e * ldq + q0 + t] : 0.f;
  }
}

// THE distance: acc[t] = sum_e (qs[e][t] - feat_t[e, n])^2, e ascending, one fused multiply-add per term.
__device__ __forceinline__ void tile_d2(const float (*qs)[PC_QT], const float* __restrict__ feat_t, int64_t ld, int64_t n, float (&acc)[PC_QT]) {
#pragma unroll
  for (int t = 0; t < PC_QT; ++t) acc[t] = 0.f;
  const float* __restrict__ p = feat_t + n;
  for (int32_t e0 = 0; e0 < SR_POSE_FEATS; e0 += PC_BATCH) {                // (207 = 9 * 23)
    float f[PC_BATCH];                                                       // a batch of loads in flight, then their terms in order
#pragma unroll
    for (int i = 0; i < PC_BATCH; ++i) f[i] = p[(int64_t)(e0 + i) * ld];
#pragma unroll
    for (int i = 0; i < PC_BATCH; ++i)
#pragma unroll
      for (int t = 0; t < PC_QT; ++t) {
        const float diff = qs[e0 + i][t] - f[i];
        acc[t] = fmaf(diff, diff, acc[t]);
      }
  }
}

// `key` into the ascending keys top[0 .. K-1] when it is below the largest; slots are walked from the top so that each reads its
// lower neighbour before that one changes.
template <int K>
__device__ __forceinline__ void insert_key(uint64_t (&top)[K], uint64_t key) {
#pragma unroll
  for (int k = K - 1; k >= 1; --k) {
    const bool below = key < top[k - 1];
    top[k] = below ? top[k - 1] : (key < top[k] ? key : top[k]);
  }
  top[0] = key < top[0] ? key : top[0];
}

template <int K>
__global__ __launch_bounds__(PC_BLOCK) void pose_neighbors(const float* __restrict__ featq_t, int64_t ldq, int64_t Q, const float* __restrict__ feat_t,
                                                            int64_t ld, int64_t N, int32_t Kout, const int32_t* __restrict__ query_frames,
                                                            int32_t exclude, int32_t* __restrict__ idx, float* __restrict__ d2) {
  __shared__ float qs[SR_POSE_FEATS][PC_QT];
  __shared__ uint64_t wave_min[2][PC_QT][PC_WAVES];
  const int32_t lane = threadIdx.x % SR_WAVE, wave = threadIdx.x / SR_WAVE;
  const int64_t tiles = (Q + PC_QT - 1) / PC_QT;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {        // (uniform over the workgroup)
    const int64_t q0 = tile * PC_QT;
    __syncthreads();                                                         // (the previous tile's reads of qs are over)
    stage_queries(qs, featq_t, ldq, Q, q0);
    int64_t frame[PC_QT];
#pragma unroll
    for (int t = 0; t < PC_QT; ++t) frame[t] = query_frames && exclude >= 0 && q0 + t < Q ? (int64_t)query_frames[q0 + t] : INT64_MIN / 2;
    __syncthreads();
    uint64_t top[PC_QT][K];
#pragma unroll
    for (int t = 0; t < PC_QT; ++t)
#pragma unroll
      for (int k = 0; k < K; ++k) top[t][k] = PC_EMPTY;
    for (int64_t n = threadIdx.x; n < N; n += PC_BLOCK) {
      float acc[PC_QT];
      tile_d2(qs, feat_t, ld, n, acc);
#pragma unroll
      for (int t = 0; t < PC_QT; ++t) {
        const int64_t off = n - frame[t];
        const bool skip = !isfinite(acc[t]) || (off >= -(int64_t)exclude && off <= (int64_t)exclude);      // (frame = -2^62: never near)
        const uint64_t key = skip ? PC_EMPTY : ((uint64_t)__float_as_uint(acc[t]) << 32) | (uint64_t)n;
        insert_key<K>(top[t], key);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {                                             // round k: the k-th smallest key of every query of the tile
      uint64_t best[PC_QT];
#pragma unroll
      for (int t = 0; t < PC_QT; ++t) {
        best[t] = sr_wave_min<uint64_t>(top[t][0]);
        if (lane == 0) wave_min[k & 1][t][wave] = best[t];
      }
      __syncthreads();                                                         // (round k + 1 writes the other half; round k + 2 comes after its barrier)
#pragma unroll
      for (int t = 0; t < PC_QT; ++t) {
        uint64_t m = wave_min[k & 1][t][0];
#pragma unroll
        for (int w = 1; w < PC_WAVES; ++w) m = min(m, wave_min[k & 1][t][w]);
        if (m != PC_EMPTY && top[t][0] == m) {                                 // the one holder drops it
#pragma unroll
          for (int s = 0; s + 1 < K; ++s) top[t][s] = top[t][s + 1];
          top[t][K - 1] = PC_EMPTY;
        }
        if (threadIdx.x == 0 && k < Kout && q0 + t < Q) {
          const bool any = m != PC_EMPTY;
          idx[(q0 + t) * Kout + k] = any ? (int32_t)(uint32_t)(m & 0xFFFFFFFFull) : -1;
          d2[(q0 + t) * Kout + k] = any ? __uint_as_float((uint32_t)(m >> 32)) : INFINITY;
        }
      }
    }
  }
}

__global__ __launch_bounds__(PC_BLOCK) void pose_dist(const float* __restrict__ featq_t, int64_t ldq, int64_t Q, const float* __restrict__ feat_t, int64_t ld,
                                                       int64_t N, float* __restrict__ D) {
  __shared__ float qs[SR_POSE_FEATS][PC_QT];
  const int64_t tiles = (Q + PC_QT - 1) / PC_QT;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {        // (uniform over the workgroup)
    const int64_t q0 = tile * PC_QT;
    __syncthreads();
    stage_queries(qs, featq_t, ldq, Q, q0);
    __syncthreads();
    for (int64_t n = threadIdx.x; n < N; n += PC_BLOCK) {
      float acc[PC_QT];
      tile_d2(qs, feat_t, ld, n, acc);
#pragma unroll
      for (int t = 0; t < PC_QT; ++t)
        if (q0 + t < Q) D[(q0 + t) * N + n] = acc[t];
    }
  }
}

__global__ __launch_bounds__(PC_BLOCK) void code_blend(const int32_t* __restrict__ idx, const float* __restrict__ d2, int64_t Q, int32_t K, float inv_two_sigma2,
                                                        const float* __restrict__ codes, int64_t N, int64_t L, float* __restrict__ out,
                                                        float* __restrict__ weights) {
  const int64_t total = Q * L;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = i / L, l = i - q * L;
    float w[SR_POSE_MAX_K];
    int64_t row[SR_POSE_MAX_K];
    float base = 0.f, sum = 0.f;
    bool found = false;
#pragma unroll
    for (int k = 0; k < SR_POSE_MAX_K; ++k) {
      const int32_t r = k < K ? idx[q * K + k] : -1;
      const bool valid = r >= 0 && (int64_t)r < N;
      const float d = valid ? d2[q * K + k] : 0.f;
      if (valid && !found) { base = d; found = true; }
      w[k] = valid ? expf(-(d - base) * inv_two_sigma2) : 0.f;
      row[k] = valid ? (int64_t)r : 0;
      sum += w[k];
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SR_POSE_MAX_K; ++k) {
      w[k] = found ? w[k] / sum : 0.f;
      acc = fmaf(w[k], w[k] != 0.f ? codes[row[k] * L + l] : 0.f, acc);
      if (l == 0 && k < K) weights[q * K + k] = w[k];
    }
    out[i] = acc;
  }
}

inline bool bad_count(int64_t n) { return n <= 0 || n >= INT32_MAX; }

inline int tile_grid(int64_t Q) {
  const int64_t tiles = sr_cdiv(Q, PC_QT);
  return (int)(tiles < PC_MAX_GRID ? tiles : PC_MAX_GRID);
}

}  // namespace

extern "C" int sr_pose_features(const float* theta, int64_t N, const float* scale, float* feat_t, int64_t ld, void* stream) {
  if (!theta || !feat_t || bad_count(N) || ld < N || bad_count(ld)) return SR_EINVAL;
  sr_launch_stream(pose_features, N * SR_POSE_JOINTS, PC_BLOCK, stream, theta, N, scale, feat_t, ld);
  return sr_launch_status();
}

extern "C" int sr_pose_neighbors(const float* featq_t, int64_t ldq, int64_t Q, const float* feat_t, int64_t ld, int64_t N, int32_t K,
                                 const int32_t* query_frames, int32_t exclude, int32_t* idx, float* d2, void* stream) {
  if (!featq_t || !feat_t || !idx || !d2 || bad_count(Q) || bad_count(N) || ldq < Q || ld < N || bad_count(ldq) || bad_count(ld) || K < 1 ||
      K > SR_POSE_MAX_K)
    return SR_EINVAL;
  const dim3 grid(tile_grid(Q)), block(PC_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  if (K == 1)
    hipLaunchKernelGGL(pose_neighbors<1>, grid, block, 0, s, featq_t, ldq, Q, feat_t, ld, N, K, query_frames, exclude, idx, d2);
  else if (K == 2)
    hipLaunchKernelGGL(pose_neighbors<2>, grid, block, 0, s, featq_t, ldq, Q, feat_t, ld, N, K, query_frames, exclude, idx, d2);
  else if (K <= 4)
    hipLaunchKernelGGL(pose_neighbors<4>, grid, block, 0, s, featq_t, ldq, Q, feat_t, ld, N, K, query_frames, exclude, idx, d2);
  else
    hipLaunchKernelGGL(pose_neighbors<8>, grid, block, 0, s, featq_t, ldq, Q, feat_t, ld, N, K, query_frames, exclude, idx, d2);
  return sr_launch_status();
}

extern "C" int sr_pose_dist(const float* featq_t, int64_t ldq, int64_t Q, const float* feat_t, int64_t ld, int64_t N, float* D, void* stream) {
  if (!featq_t || !feat_t || !D || bad_count(Q) || bad_count(N) || ldq < Q || ld < N || bad_count(ldq) || bad_count(ld)) return SR_EINVAL;
  hipLaunchKernelGGL(pose_dist, dim3(tile_grid(Q)), dim3(PC_BLOCK), 0, (hipStream_t)stream, featq_t, ldq, Q, feat_t, ld, N, D);
  return sr_launch_status();
}

extern "C" int sr_code_blend(const int32_t* idx, const float* d2, int64_t Q, int32_t K, float inv_two_sigma2, const float* codes, int64_t N, int64_t L,
                             float* out, float* weights, void* stream) {
  if (!idx || !d2 || !codes || !out || !weights || bad_count(Q) || bad_count(N) || bad_count(L) || K < 1 || K > SR_POSE_MAX_K ||
      !(inv_two_sigma2 >= 0.f) || !std::isfinite(inv_two_sigma2))
    return SR_EINVAL;
  sr_launch_stream(code_blend, Q * L, PC_BLOCK, stream, idx, d2, Q, K, inv_two_sigma2, codes, N, L, out, weights);
  return sr_launch_status();
}
