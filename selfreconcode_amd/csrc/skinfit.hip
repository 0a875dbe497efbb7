// Fitting a fixed-weight skin to the trained deformer: what a glTF skin can hold of a model whose skinning weights
// are looked up at the deformed point and so change from frame to frame.
//
//  * sr_skinfit_accumulate: one lane per vertex, SF_WAVES waves per workgroup.  With sum_k x_k = 1 the skinning residual of frame t is
//    sum_k x_k d_tk, so the fit needs only H = sum_t D^T D: C (C + 1) / 2 doubles per vertex, kept in registers (C is a compile-time
//    case, every index into the accumulators is a constant).  A batch's transforms go through the LDS in slabs of SR_SKINFIT_SLAB
//    frames (24 x 12 floats each); a candidate's 12 floats are three 16-byte LDS reads.  The waves of a workgroup share its 64
//    vertices and split a slab's frames, which is what fills the machine for a template of 10 - 20 k vertices; their partial sums
//    are added through the LDS one wave after the other, in ascending wave order.  q and y are read once each, a lane's three floats
//    next to its neighbour's.
//  * sr_skinfit_solve: one lane per vertex.  H, the Cholesky factor and the vectors live in registers: a support is a bit mask that
//    is the same in every lane, the problem on it is embedded in the full C x C one (rows outside the support are the identity's, so
//    their unknowns are exactly 0 and the others see the sums of the compact factorisation plus zeros), and every loop over
//    candidates is unrolled -- no array is indexed by a run-time value, so nothing goes to scratch.
//
// No atomics; every loop runs over an integer range fixed before it starts; a float comparison decides what is kept, never how long
// a loop runs.  Two calls give identical bits.
#include <cmath>
#include "skinfit_abi.h"
#include "sr_common.h"

namespace {

#define SF_WAVES 8
#define SF_BLOCK (SF_WAVES * SR_WAVE)
#define SF_A_FLOATS (SR_SKINFIT_JOINTS * 12)
#define SF_SOLVE_BLOCK 64

static_assert(SR_SKINFIT_TRI == SR_SKINFIT_MAX_CANDS * (SR_SKINFIT_MAX_CANDS + 1) / 2, "triangle of the largest candidate set");
static_assert(SR_SKINFIT_SLAB * SF_A_FLOATS * sizeof(float) <= SR_SKINFIT_TRI * SR_WAVE * sizeof(double), "the slab fits the exchange buffer");
static_assert(SF_A_FLOATS * sizeof(float) % 16 == 0, "a frame's transforms keep the 16-byte alignment");

__host__ __device__ constexpr int tri(int k, int l) { return k * (k + 1) / 2 + l; }

template <int C>
__global__ __launch_bounds__(SF_BLOCK) void skinfit_accumulate(const float* __restrict__ q, const float* __restrict__ y, const float* __restrict__ A,
                                                                const float* __restrict__ trans, int64_t T, int64_t V,
                                                                const int32_t* __restrict__ cands, double* __restrict__ H) {
  constexpr int E = C * (C + 1) / 2;
  __shared__ __attribute__((aligned(16))) double buf[SR_SKINFIT_TRI * SR_WAVE];      // a slab of A as floats, then the waves' partial sums
  float* As = reinterpret_cast<float*>(buf);
  const int32_t lane = threadIdx.x % SR_WAVE, wave = threadIdx.x / SR_WAVE;
  const int64_t v = (int64_t)blockIdx.x * SR_WAVE + lane;
  const bool live = v < V;
  int32_t off[C];                                                                     // the candidates' offsets into a frame's transforms
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int32_t j = live ? cands[v * C + k] : 0;
    off[k] = (j < 0 ? 0 : (j >= SR_SKINFIT_JOINTS ? SR_SKINFIT_JOINTS - 1 : j)) * 12;
  }
  double acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.;
  for (int64_t t0 = 0; t0 < T; t0 += SR_SKINFIT_SLAB) {                               // (uniform over the workgroup)
    const int32_t n = (int32_t)(T - t0 < SR_SKINFIT_SLAB ? T - t0 : SR_SKINFIT_SLAB);
    __syncthreads();                                                                  // (the previous slab's reads are over)
    for (int32_t i = threadIdx.x; i < n * SF_A_FLOATS; i += SF_BLOCK) As[i] = A[t0 * SF_A_FLOATS + i];
    __syncthreads();
    for (int32_t f = wave; f < n; f += SF_WAVES) {                                    // (uniform over the wave)
      if (!live) continue;
      const int64_t t = t0 + f;
      const float* qp = q + (t * V + v) * 3;
      const float* yp = y + (t * V + v) * 3;
      const double qx = qp[0], qy = qp[1], qz = qp[2];
      const double tx = (double)yp[0] - (double)trans[t * 3 + 0], ty = (double)yp[1] - (double)trans[t * 3 + 1],
                   tz = (double)yp[2] - (double)trans[t * 3 + 2];
      double d[C][3];
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const float4* row = reinterpret_cast<const float4*>(As + f * SF_A_FLOATS + off[k]);
        const float4 r0 = row[0], r1 = row[1], r2 = row[2];
        d[k][0] = ((((double)r0.x * qx + (double)r0.y * qy) + (double)r0.z * qz) + (double)r0.w) - tx;
        d[k][1] = ((((double)r1.x * qx + (double)r1.y * qy) + (double)r1.z * qz) + (double)r1.w) - ty;
        d[k][2] = ((((double)r2.x * qx + (double)r2.y * qy) + (double)r2.z * qz) + (double)r2.w) - tz;
      }
#pragma unroll
      for (int k = 0; k < C; ++k)
#pragma unroll
        for (int l = 0; l <= k; ++l) acc[tri(k, l)] += (d[k][0] * d[l][0] + d[k][1] * d[l][1]) + d[k][2] * d[l][2];
    }
  }
  for (int32_t w = 1; w < SF_WAVES; ++w) {                                            // wave 0 += wave w, w ascending
    __syncthreads();                                                                  // (the slab, or wave w - 1's sums, have been read)
    if (wave == w) {
#pragma unroll
      for (int e = 0; e < E; ++e) buf[e * SR_WAVE + lane] = acc[e];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] += buf[e * SR_WAVE + lane];
    }
  }
  if (wave == 0 && live) {
#pragma unroll
    for (int e = 0; e < E; ++e) H[(int64_t)e * V + v] += acc[e];
  }
}

template <int C>
__global__ __launch_bounds__(SF_SOLVE_BLOCK) void skinfit_solve(const double* __restrict__ H, const double* __restrict__ xbar,
                                                                 const int32_t* __restrict__ cands, int64_t V, int32_t K, double reg,
                                                                 double lambda_floor, int32_t* __restrict__ joints, float* __restrict__ weights,
                                                                 double* __restrict__ objective, int32_t* __restrict__ mask_out,
                                                                 double* __restrict__ lambda_out) {
  constexpr int E = C * (C + 1) / 2;
  const int64_t v = (int64_t)blockIdx.x * SF_SOLVE_BLOCK + threadIdx.x;
  if (v >= V) return;
  double h[E], xb[C];
  double check = 0., trace = 0.;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    h[e] = H[(int64_t)e * V + v];
    check += h[e];
  }
#pragma unroll
  for (int k = 0; k < C; ++k) {
    xb[k] = xbar[(int64_t)k * V + v];
    check += xb[k];
    trace += h[tri(k, k)];
  }
  const double lam = reg * trace / (double)C + lambda_floor;
  double best[C], best_obj = INFINITY;
  int32_t best_mask = 0, best_count = 0;
#pragma unroll
  for (int k = 0; k < C; ++k) best[k] = 0.;
  if (!std::isfinite(check) || !std::isfinite(lam)) {
    // no search: the K largest xbar, one per round, a tie (or values that do not compare) to the lower candidate
    double sum = 0.;
    for (int32_t r = 0; r < K; ++r) {
      int32_t pick = -1;
      double top = 0.;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const bool taken = (best_mask >> k) & 1;
        if (!taken && (pick < 0 || xb[k] > top)) {
          pick = k;
          top = xb[k];
        }
      }
      best_mask |= 1 << pick;                                   // (K <= C: a free candidate exists in every round)
    }
#pragma unroll
    for (int k = 0; k < C; ++k) sum += ((best_mask >> k) & 1) && xb[k] > 0. ? xb[k] : 0.;
    const bool usable = std::isfinite(sum) && sum > 0.;
    bool first = true;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const bool in = (best_mask >> k) & 1;
      best[k] = !in ? 0. : (usable ? (xb[k] > 0. ? xb[k] / sum : 0.) : (first ? 1. : 0.));
      first = first && !in;
    }
    best_obj = NAN;
  } else {
    const int32_t masks = 1 << C;
    for (int32_t m = 1; m < masks; ++m) {                       // (uniform over the launch)
      const int32_t count = __popc(m);
      if (count > K) continue;
      bool in[C];
#pragma unroll
      for (int k = 0; k < C; ++k) in[k] = (m >> k) & 1;
      double L[E], u[C], w[C];
      bool ok = true;
#pragma unroll
      for (int j = 0; j < C; ++j) {
        double s = in[j] ? h[tri(j, j)] + lam : 1.;
#pragma unroll
        for (int p = 0; p < j; ++p) s -= L[tri(j, p)] * L[tri(j, p)];
        ok = ok && s > 0.;
        const double root = sqrt(s), inv = 1. / root;
        L[tri(j, j)] = root;
#pragma unroll
        for (int i = j + 1; i < C; ++i) {
          double a = in[i] && in[j] ? h[tri(i, j)] : 0.;
#pragma unroll
          for (int p = 0; p < j; ++p) a -= L[tri(i, p)] * L[tri(j, p)];
          L[tri(i, j)] = a * inv;
        }
      }
#pragma unroll
      for (int i = 0; i < C; ++i) {                             // L a = b, L c = 1 on the support
        double a = in[i] ? lam * xb[i] : 0., c = in[i] ? 1. : 0.;
#pragma unroll
        for (int p = 0; p < i; ++p) {
          a -= L[tri(i, p)] * u[p];
          c -= L[tri(i, p)] * w[p];
        }
        u[i] = a / L[tri(i, i)];
        w[i] = c / L[tri(i, i)];
      }
#pragma unroll
      for (int i = C - 1; i >= 0; --i) {                        // L^T u = a, L^T w = c
        double a = u[i], c = w[i];
#pragma unroll
        for (int p = i + 1; p < C; ++p) {
          a -= L[tri(p, i)] * u[p];
          c -= L[tri(p, i)] * w[p];
        }
        u[i] = a / L[tri(i, i)];
        w[i] = c / L[tri(i, i)];
      }
      double su = 0., sw = 0.;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        su += u[k];
        sw += w[k];
      }
      const double nu = (su - 1.) / sw;
      double x[C], fit = 0., prior = 0.;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        x[k] = in[k] ? u[k] - nu * w[k] : 0.;
        ok = ok && !(x[k] < 0.);
      }
#pragma unroll
      for (int i = 0; i < C; ++i) {
        double row = 0.;
#pragma unroll
        for (int j = 0; j < i; ++j) row += h[tri(i, j)] * x[j];
        fit += x[i] * (h[tri(i, i)] * x[i] + 2. * row);
        prior += (x[i] - xb[i]) * (x[i] - xb[i]);
      }
      const double obj = fit + lam * prior;
      ok = ok && std::isfinite(obj);
      if (ok && (obj < best_obj || (obj == best_obj && count < best_count))) {       // (masks ascend: an equal count keeps the lower)
        best_obj = obj;
        best_mask = m;
        best_count = count;
#pragma unroll
        for (int k = 0; k < C; ++k) best[k] = x[k];
      }
    }
    if (best_mask == 0) {                                       // (cannot happen for finite input: a single candidate is always feasible)
      best_mask = 1;
      best[0] = 1.;
      best_obj = NAN;
    }
  }
  // float32 weights whose sum is 1: the largest takes what the rounding left
  float w32[C];
  double left = 1., top = -1.;
  int32_t big = 0;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    w32[k] = (float)best[k];
    left -= (double)w32[k];
    if (best[k] > top) {
      top = best[k];
      big = k;
    }
  }
  int32_t slot = 0;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    if ((best_mask >> k) & 1) {
      if (slot < K) {                                           // (popcount(best_mask) <= K: always)
        const float wk = k == big ? (float)((double)w32[k] + left) : w32[k];
        joints[v * K + slot] = wk > 0.f ? cands[v * C + k] : 0;      // (a weight that rounds to 0 names joint 0, as an unused slot does)
        weights[v * K + slot] = wk;
      }
      ++slot;
    }
  }
  for (; slot < K; ++slot) {
    joints[v * K + slot] = 0;
    weights[v * K + slot] = 0.f;
  }
  objective[v] = best_obj;
  if (mask_out) mask_out[v] = best_mask;
  if (lambda_out) lambda_out[v] = lam;
}

inline bool bad_count(int64_t n) { return n <= 0 || n >= INT32_MAX; }

}  // namespace

#define SF_CASES(LAUNCH) \
  switch (C) {           \
    case 1: LAUNCH(1); break; \
    case 2: LAUNCH(2); break; \
    case 3: LAUNCH(3); break; \
    case 4: LAUNCH(4); break; \
    case 5: LAUNCH(5); break; \
    case 6: LAUNCH(6); break; \
    case 7: LAUNCH(7); break; \
    default: LAUNCH(8); break; \
  }

extern "C" int sr_skinfit_accumulate(const float* q, const float* y, const float* A, const float* trans, int64_t T, int64_t V, const int32_t* cands,
                                     int32_t C, double* H, void* stream) {
  if (!q || !y || !A || !trans || !cands || !H || bad_count(T) || bad_count(V) || C < 1 || C > SR_SKINFIT_MAX_CANDS) return SR_EINVAL;
  const dim3 grid((unsigned)sr_cdiv(V, SR_WAVE)), block(SF_BLOCK);
#define SF_LAUNCH(N) hipLaunchKernelGGL(skinfit_accumulate<N>, grid, block, 0, (hipStream_t)stream, q, y, A, trans, T, V, cands, H)
  SF_CASES(SF_LAUNCH)
#undef SF_LAUNCH
  return sr_launch_status();
}

extern "C" int sr_skinfit_solve(const double* H, const double* xbar, const int32_t* cands, int64_t V, int32_t C, int32_t K, double reg,
                                double lambda_floor, int32_t* joints, float* weights, double* objective, int32_t* mask, double* lambda, void* stream) {
  if (!H || !xbar || !cands || !joints || !weights || !objective || bad_count(V) || C < 1 || C > SR_SKINFIT_MAX_CANDS || K < 1 || K > C ||
      !std::isfinite(reg) || reg < 0. || !std::isfinite(lambda_floor) || !(lambda_floor > 0.))
    return SR_EINVAL;
  const dim3 grid((unsigned)sr_cdiv(V, SF_SOLVE_BLOCK)), block(SF_SOLVE_BLOCK);
#define SF_LAUNCH(N) \
  hipLaunchKernelGGL(skinfit_solve<N>, grid, block, 0, (hipStream_t)stream, H, xbar, cands, V, K, reg, lambda_floor, joints, weights, objective, mask, lambda)
  SF_CASES(SF_LAUNCH)
#undef SF_LAUNCH
  return sr_launch_status();
}
