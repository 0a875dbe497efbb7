// SMPL body model, backward, float32: the adjoints of the stages of csrc/smpl.hip (shapes as in its header comment), and the keypoint
// data term of smpl_fit.py.
//   smpl_regress_bwd_kernel:  g_x[b,v,:] (+)= sum_k reg[v,k] g_out[b,k,:], one thread per (b, v), g_out[b] in LDS.
//   smpl_shape_bwd_*:         g_beta[b,i] = sum_e shapedirs[i,e] g_vshaped[b,e]: a workgroup reduces SHAPE_CHUNK elements (a serial
//     ascending sum per thread, the xor butterfly inside a wave, the waves in ascending order) into one partial row; a second launch adds
//     the partial rows in ascending order.
//   smpl_skin_bwd_kernel:     the forward's tiling (one thread per vertex, SR_SMPL_BATCH_TILE batch items per workgroup, the tile's A and
//     pose features in LDS).  g_rest = (sum_j w_j R_j)^T gV needs no v_posed, so it comes first; then ONE pass over posedirs gives both
//     the pose blend (v_posed, recomputed, not stored by the forward) and the workgroup's share of g_feature (per basis vector the
//     tile's 8 products are reduced over the wave by a halving butterfly: 4 + 2 + 1 exchanges fold the 8 values onto lane groups, 3
//     more finish the sum; the two waves are added in ascending order).  gA[b,j] = sum_v w_vj gV_v (x) [v_posed_v; 1] is a
//     [24 x 128] x [128 x 12] product per batch item through LDS, every output summed over the vertices in ascending order.  The
//     workgroup writes one partial row (288 + 207 floats) per batch item; smpl_skin_bwd_final_kernel adds the rows in ascending order.
//   smpl_pose_bwd_kernel:     one thread per batch item, the reverse of smpl_pose_kernel: A = G - pad(G [J;0]), the chain with children
//     before parents, R[1:] - I, and the axis-angle route differentiated as written (the dual numbers of rot_dual.h through
//     srrot::rodrigues, the +1e-8 included: finite at theta = 0).  The chain's cotangents live in LDS, element-major.
//   keypoint_energy_kernel:   one wave per frame, lane k = joint k; value and gradient of sum_k (w_k c_k)^2 rho_sigma(r_k); the sums over
//     k are taken by lane 0 in ascending order.
// No float atomics; every sum has an order fixed by the shapes: two calls give identical bits.
#include "sr_common.h"
#include "sr_wave.h"
#include "rot_dual.h"

#define SMPL_NJ 24
#define SMPL_NPOSE 207
#define SMPL_BT SR_SMPL_BATCH_TILE
#define SMPL_SKIN_BLOCK 128
#define SMPL_EW_BLOCK 256
#define SHAPE_CHUNK 2048                  // elements of [nv*3] per partial row of the shape adjoint
#define SHAPE_MAX_BETA 32
#define REG_MAX_K 42                      // 3 nk <= 128 in the forward regression
#define GA_ROW (SMPL_NJ * 12)             // 288
#define SKIN_ROW (GA_ROW + SMPL_NPOSE)    // one partial row of the skin adjoint: gA then g_feature
#define POSE_T 32                         // batch items per workgroup of the pose adjoint
#define KP_MAX 64

static_assert(SMPL_BT == 8, "the halving butterfly of smpl_skin_bwd_kernel folds exactly 8 values");

struct smpl_parents_g { int32_t p[SMPL_NJ]; };
struct kp_camera { float R[9], T[3], fx, fy, cx, cy; };

using srrot::Dual;

// ------------------------------------------------------------------------------------------------ partial rows -> sums
__global__ __launch_bounds__(SMPL_EW_BLOCK) void smpl_rows_final_kernel(const float* __restrict__ partial, int B, int nchunks, int row,
                                                                        float* __restrict__ out) {
  const int i = blockIdx.x * SMPL_EW_BLOCK + threadIdx.x;
  if (i >= B * row) return;
  const int b = i / row, e = i % row;
  const float* p = partial + (int64_t)b * nchunks * row + e;
  float acc = 0.f;
  for (int c = 0; c < nchunks; ++c) acc += p[(int64_t)c * row];                         // ascending chunk order
  out[i] = acc;
}

// ------------------------------------------------------------------------------------------------ joint regressions
__global__ __launch_bounds__(SMPL_EW_BLOCK) void smpl_regress_bwd_kernel(const float* __restrict__ g_out, const float* __restrict__ reg, int nv, int nk,
                                                                         int accumulate, float* __restrict__ g_x) {
  __shared__ float gs[REG_MAX_K * 3];
  const int b = blockIdx.y, t = threadIdx.x;
  if (t < 3 * nk) gs[t] = g_out[(int64_t)b * 3 * nk + t];
  __syncthreads();
  const int v = blockIdx.x * SMPL_EW_BLOCK + t;
  if (v >= nv) return;
  const float* r = reg + (int64_t)v * nk;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int k = 0; k < nk; ++k) {                                                        // ascending joint order
    const float w = r[k];
    a0 = fmaf(w, gs[3 * k], a0); a1 = fmaf(w, gs[3 * k + 1], a1); a2 = fmaf(w, gs[3 * k + 2], a2);
  }
  float* o = g_x + ((int64_t)b * nv + v) * 3;
  if (accumulate) { o[0] += a0; o[1] += a1; o[2] += a2; }
  else { o[0] = a0; o[1] = a1; o[2] = a2; }
}

extern "C" int sr_smpl_regress_bwd(const float* g_out, const float* reg, int32_t B, int64_t nv, int32_t nk, int32_t accumulate, float* g_x,
                                   void* stream) {
  if (!g_out || !reg || !g_x || B < 1 || B > 65535 || nv < 1 || nv > INT32_MAX / 4 || nk < 1 || nk > REG_MAX_K) return SR_EINVAL;
  if (nv * nk > INT32_MAX) return SR_EINVAL;
  const dim3 grid((unsigned)sr_cdiv(nv, SMPL_EW_BLOCK), (unsigned)B), block(SMPL_EW_BLOCK);
  hipLaunchKernelGGL(smpl_regress_bwd_kernel, grid, block, 0, (hipStream_t)stream, g_out, reg, (int)nv, nk, accumulate, g_x);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ shape blend
__global__ __launch_bounds__(SMPL_EW_BLOCK) void smpl_shape_bwd_partial_kernel(const float* __restrict__ shapedirs, const float* __restrict__ g_vshaped,
                                                                               int nbeta, int64_t n3, float* __restrict__ partial) {
  __shared__ float ws[SHAPE_MAX_BETA * (SMPL_EW_BLOCK / SR_WAVE)];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x, t = threadIdx.x;
  const int64_t e0 = (int64_t)chunk * SHAPE_CHUNK;
  const int n = (int)min((int64_t)SHAPE_CHUNK, n3 - e0);
  const float* g = g_vshaped + (int64_t)b * n3 + e0;
  float gv[SHAPE_CHUNK / SMPL_EW_BLOCK];
#pragma unroll
  for (int q = 0; q < SHAPE_CHUNK / SMPL_EW_BLOCK; ++q) {
    const int e = q * SMPL_EW_BLOCK + t;
    gv[q] = e < n ? g[e] : 0.f;
  }
  for (int i = 0; i < nbeta; ++i) {
    const float* s = shapedirs + (int64_t)i * n3 + e0;
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < SHAPE_CHUNK / SMPL_EW_BLOCK; ++q) {
      const int e = q * SMPL_EW_BLOCK + t;
      acc = fmaf(e < n ? s[e] : 0.f, gv[q], acc);
    }
    acc = sr_wave_sum(acc);
    if ((t & (SR_WAVE - 1)) == 0) ws[i * (SMPL_EW_BLOCK / SR_WAVE) + t / SR_WAVE] = acc;
  }
  __syncthreads();
  if (t < nbeta) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < SMPL_EW_BLOCK / SR_WAVE; ++w) acc += ws[t * (SMPL_EW_BLOCK / SR_WAVE) + w];   // ascending wave order
    partial[((int64_t)b * nchunks + chunk) * nbeta + t] = acc;
  }
}

extern "C" int64_t sr_smpl_shape_bwd_workspace_floats(int32_t B, int32_t nbeta, int64_t nv) {
  if (B < 1 || nbeta < 1 || nv < 1) return -1;
  return (int64_t)B * sr_cdiv(3 * nv, SHAPE_CHUNK) * nbeta;
}

extern "C" int sr_smpl_shape_bwd(const float* shapedirs, const float* g_vshaped, int32_t B, int32_t nbeta, int64_t nv, float* partial, float* g_beta,
                                 void* stream) {
  if (!shapedirs || !g_vshaped || !partial || !g_beta || B < 1 || B > 65535 || nbeta < 1 || nbeta > SHAPE_MAX_BETA || nv < 1 || nv > INT32_MAX / 4)
    return SR_EINVAL;
  const int64_t n3 = 3 * nv;
  const int nchunks = (int)sr_cdiv(n3, SHAPE_CHUNK);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(smpl_shape_bwd_partial_kernel, dim3((unsigned)nchunks, (unsigned)B), dim3(SMPL_EW_BLOCK), 0, s, shapedirs, g_vshaped, nbeta, n3, partial);
  hipLaunchKernelGGL(smpl_rows_final_kernel, dim3((unsigned)sr_cdiv((int64_t)B * nbeta, SMPL_EW_BLOCK)), dim3(SMPL_EW_BLOCK), 0, s, partial, B, nchunks, nbeta,
                     g_beta);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ skin stage
// LDS of the skin adjoint, in floats.  H (one batch item's gV (x) [v_posed; 1], [vertex][12]) reuses the pose features once the pass over
// posedirs is done; the weights ([joint][129]: a row of 129 keeps the 24 joints of one vertex on different banks) reuse the g_feature
// sums once those are written out.
#define SK_FEAT 0                                               // [207][tile]
#define SK_H 0                                                  // [128][12]
#define SK_AS (SK_FEAT + SMPL_NPOSE * SMPL_BT)                  // [tile][24][12]
#define SK_GR (SK_AS + SMPL_BT * SMPL_NJ * 12)                  // [tile][3][thread]: g_rest, then v_posed
#define SK_GV (SK_GR + SMPL_BT * 3 * SMPL_SKIN_BLOCK)           // [tile][3][thread]: gV
#define SK_GF (SK_GV + SMPL_BT * 3 * SMPL_SKIN_BLOCK)           // [207][tile][wave]
#define SK_W SK_GF                                              // [24][129]
#define SK_WPITCH (SMPL_SKIN_BLOCK + 1)
#define SK_TOTAL (SK_GF + SMPL_NPOSE * SMPL_BT * 2)
static_assert(SMPL_SKIN_BLOCK * 12 <= SMPL_NPOSE * SMPL_BT, "H fits where the pose features were");
static_assert(SMPL_NJ * SK_WPITCH <= SMPL_NPOSE * SMPL_BT * 2, "the weights fit where the g_feature sums were");
static_assert(SK_TOTAL * 4 <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(SMPL_SKIN_BLOCK) void smpl_skin_bwd_kernel(const float* __restrict__ rest, int64_t rest_stride, const float* __restrict__ posedirs,
                                                                        const float* __restrict__ feature, const float* __restrict__ weights,
                                                                        const float* __restrict__ A, const float* __restrict__ gV, int B, int nv,
                                                                        float* __restrict__ g_rest, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float sm[SK_TOTAL];
  float* feat = sm + SK_FEAT;
  float* As = sm + SK_AS;
  float* gr = sm + SK_GR;
  float* gvs = sm + SK_GV;
  float* gf = sm + SK_GF;
  float* Hs = sm + SK_H;
  float* Ws = sm + SK_W;
  const int t = threadIdx.x;
  const int b0 = blockIdx.y * SMPL_BT;
  const int nb = min(SMPL_BT, B - b0);
  const int chunk = blockIdx.x, nchunks = gridDim.x;
  const int v = chunk * SMPL_SKIN_BLOCK + t;
  const int vc = min(v, nv - 1);                       // threads past the end read the last vertex, carry a zero cotangent and store nothing
  const bool live = v < nv;

  if (posedirs) {
    for (int e = t; e < SMPL_NPOSE * SMPL_BT; e += SMPL_SKIN_BLOCK) {
      const int k = e / SMPL_BT, bb = e % SMPL_BT;
      feat[e] = bb < nb ? feature[(int64_t)(b0 + bb) * SMPL_NPOSE + k] : 0.f;
    }
  }
  for (int e = t; e < SMPL_BT * SMPL_NJ * 12; e += SMPL_SKIN_BLOCK) {
    const int bb = e / (SMPL_NJ * 12), r = e % (SMPL_NJ * 12);
    As[e] = bb < nb ? A[((int64_t)(b0 + bb) * SMPL_NJ + r / 12) * 16 + r % 12] : 0.f;
  }
  __syncthreads();

  float w[SMPL_NJ];
  const float* wr = weights + (int64_t)vc * SMPL_NJ;
#pragma unroll
  for (int j = 0; j < SMPL_NJ; ++j) w[j] = wr[j];

  // g_rest = (sum_j w_j R_j)^T gV; items past the batch keep zeros in their LDS columns
#pragma unroll 1
  for (int bb = 0; bb < SMPL_BT; ++bb) {
    float g[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 0.f};
    if (bb < nb) {
      if (live) {
        const float* gp = gV + ((int64_t)(b0 + bb) * nv + v) * 3;
        g[0] = gp[0]; g[1] = gp[1]; g[2] = gp[2];
      }
#pragma unroll 1
      for (int r = 0; r < 3; ++r) {
        const float* Ab = As + bb * SMPL_NJ * 12 + 4 * r;
        float T0 = 0.f, T1 = 0.f, T2 = 0.f;
#pragma unroll
        for (int j = 0; j < SMPL_NJ; ++j) {
          const float4 a = *reinterpret_cast<const float4*>(Ab + j * 12);
          T0 = fmaf(w[j], a.x, T0); T1 = fmaf(w[j], a.y, T1); T2 = fmaf(w[j], a.z, T2);
        }
        const float gr_ = r == 0 ? g[0] : (r == 1 ? g[1] : g[2]);
        o[0] = fmaf(T0, gr_, o[0]); o[1] = fmaf(T1, gr_, o[1]); o[2] = fmaf(T2, gr_, o[2]);    // rows in ascending order
      }
      if (live) {
        float* op = g_rest + ((int64_t)(b0 + bb) * nv + v) * 3;
        op[0] = o[0]; op[1] = o[1]; op[2] = o[2];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      gr[(bb * 3 + c) * SMPL_SKIN_BLOCK + t] = o[c];
      gvs[(bb * 3 + c) * SMPL_SKIN_BLOCK + t] = g[c];
    }
  }
  // (each thread reads back only its own columns of gr / gvs: no barrier needed)

  float acc[SMPL_BT][3];
#pragma unroll
  for (int bb = 0; bb < SMPL_BT; ++bb) { acc[bb][0] = 0.f; acc[bb][1] = 0.f; acc[bb][2] = 0.f; }
  if (posedirs) {
    float go[SMPL_BT][3];
#pragma unroll
    for (int bb = 0; bb < SMPL_BT; ++bb)
#pragma unroll
      for (int c = 0; c < 3; ++c) go[bb][c] = gr[(bb * 3 + c) * SMPL_SKIN_BLOCK + t];
    const float* pd = posedirs + 3 * (int64_t)vc;
    const int64_t n3 = 3 * (int64_t)nv;
    const int lane = t & (SR_WAVE - 1), wave = t / SR_WAVE;
    const bool h32 = (lane & 32) != 0, h16 = (lane & 16) != 0, h8 = (lane & 8) != 0;
    const int mybb = (h32 ? 4 : 0) + (h16 ? 2 : 0) + (h8 ? 1 : 0);               // the batch item whose sum ends on this lane
#pragma unroll 1
    for (int k = 0; k < SMPL_NPOSE; ++k) {
      const float px = pd[k * n3], py = pd[k * n3 + 1], pz = pd[k * n3 + 2];
      float f[SMPL_BT], d[SMPL_BT];
#pragma unroll
      for (int q = 0; q < SMPL_BT / 4; ++q) {
        const float4 u = *reinterpret_cast<const float4*>(&feat[k * SMPL_BT + 4 * q]);
        f[4 * q] = u.x; f[4 * q + 1] = u.y; f[4 * q + 2] = u.z; f[4 * q + 3] = u.w;
      }
#pragma unroll
      for (int bb = 0; bb < SMPL_BT; ++bb) {
        acc[bb][0] = fmaf(f[bb], px, acc[bb][0]); acc[bb][1] = fmaf(f[bb], py, acc[bb][1]); acc[bb][2] = fmaf(f[bb], pz, acc[bb][2]);
        d[bb] = fmaf(pz, go[bb][2], fmaf(py, go[bb][1], px * go[bb][0]));
      }
      // 8 values per lane -> 1: a lane keeps the half of the values its bit selects and receives the partner's sums of that half
      float d4[4], d2[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float keep = h32 ? d[4 + i] : d[i], send = h32 ? d[i] : d[4 + i];
        d4[i] = keep + __shfl_xor(send, 32, SR_WAVE);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float keep = h16 ? d4[2 + i] : d4[i], send = h16 ? d4[i] : d4[2 + i];
        d2[i] = keep + __shfl_xor(send, 16, SR_WAVE);
      }
      float s = (h8 ? d2[1] : d2[0]) + __shfl_xor(h8 ? d2[0] : d2[1], 8, SR_WAVE);
      s += __shfl_xor(s, 4, SR_WAVE);
      s += __shfl_xor(s, 2, SR_WAVE);
      s += __shfl_xor(s, 1, SR_WAVE);
      if ((lane & 7) == 0) gf[(k * SMPL_BT + mybb) * 2 + wave] = s;
    }
  }
  // v_posed over g_rest's columns (each thread overwrites what only it reads)
#pragma unroll
  for (int bb = 0; bb < SMPL_BT; ++bb) {
    if (bb < nb) {
      const float* r = rest + (int64_t)(b0 + bb) * rest_stride + 3 * (int64_t)vc;
#pragma unroll
      for (int c = 0; c < 3; ++c) gr[(bb * 3 + c) * SMPL_SKIN_BLOCK + t] = acc[bb][c] + r[c];
    }
  }
  __syncthreads();                                       // gf complete; nobody reads feat any more
  if (posedirs) {
    for (int e = t; e < SMPL_NPOSE * nb; e += SMPL_SKIN_BLOCK) {
      const int bb = e / SMPL_NPOSE, k = e % SMPL_NPOSE;
      partial[((int64_t)(b0 + bb) * nchunks + chunk) * SKIN_ROW + GA_ROW + k] = gf[(k * SMPL_BT + bb) * 2] + gf[(k * SMPL_BT + bb) * 2 + 1];
    }
    __syncthreads();                                     // gf read out before the weights take its place
  }
#pragma unroll
  for (int j = 0; j < SMPL_NJ; ++j) Ws[j * SK_WPITCH + t] = live ? wr[j] : 0.f;     // (read again: the registers were given back)

  // gA[bb][j][r][c] = sum_v w_vj gV_v[r] [v_posed_v; 1][c]: thread (j, r) owns one row of four
  const int oj = t / 3, orow = t % 3;
#pragma unroll 1
  for (int bb = 0; bb < nb; ++bb) {
    const float x = gr[(bb * 3) * SMPL_SKIN_BLOCK + t], y = gr[(bb * 3 + 1) * SMPL_SKIN_BLOCK + t], z = gr[(bb * 3 + 2) * SMPL_SKIN_BLOCK + t];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float g = gvs[(bb * 3 + r) * SMPL_SKIN_BLOCK + t];
      *reinterpret_cast<float4*>(&Hs[t * 12 + 4 * r]) = make_float4(g * x, g * y, g * z, g);
    }
    __syncthreads();
    if (t < SMPL_NJ * 3) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      const float* wj = Ws + oj * SK_WPITCH;
#pragma unroll 4
      for (int u = 0; u < SMPL_SKIN_BLOCK; ++u) {         // ascending vertex order
        const float4 h = *reinterpret_cast<const float4*>(&Hs[u * 12 + 4 * orow]);
        const float ww = wj[u];
        a0 = fmaf(ww, h.x, a0); a1 = fmaf(ww, h.y, a1); a2 = fmaf(ww, h.z, a2); a3 = fmaf(ww, h.w, a3);
      }
      float* o = partial + ((int64_t)(b0 + bb) * nchunks + chunk) * SKIN_ROW + oj * 12 + 4 * orow;
      o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(SMPL_EW_BLOCK) void smpl_skin_bwd_final_kernel(const float* __restrict__ partial, int B, int nchunks, int nf,
                                                                            float* __restrict__ gA, float* __restrict__ g_feature) {
  const int row = GA_ROW + nf;                           // nf = 207, or 0 without posedirs
  const int i = blockIdx.x * SMPL_EW_BLOCK + threadIdx.x;
  if (i >= B * row) return;
  const int b = i / row, e = i % row;
  const float* p = partial + (int64_t)b * nchunks * SKIN_ROW + e;
  float acc = 0.f;
  for (int c = 0; c < nchunks; ++c) acc += p[(int64_t)c * SKIN_ROW];                      // ascending chunk order
  if (e < GA_ROW) gA[(int64_t)b * GA_ROW + e] = acc;
  else g_feature[(int64_t)b * SMPL_NPOSE + e - GA_ROW] = acc;
}

extern "C" int64_t sr_smpl_skin_bwd_workspace_floats(int32_t B, int64_t nv) {
  if (B < 1 || nv < 1) return -1;
  return (int64_t)B * sr_cdiv(nv, SMPL_SKIN_BLOCK) * SKIN_ROW;
}

extern "C" int sr_smpl_skin_bwd(const float* rest, int64_t rest_batch_stride, const float* posedirs, const float* feature, const float* weights,
                                const float* A, const float* gV, int32_t B, int64_t nv, float* partial, float* g_rest, float* gA, float* g_feature,
                                void* stream) {
  if (!rest || !weights || !A || !gV || !partial || !g_rest || !gA || B < 1 || nv < 1 || nv > INT32_MAX / 4 || rest_batch_stride < 0) return SR_EINVAL;
  if ((posedirs != nullptr) != (feature != nullptr) || (posedirs != nullptr) != (g_feature != nullptr)) return SR_EINVAL;
  if (sr_cdiv(B, SMPL_BT) > 65535 || (int64_t)B * SKIN_ROW > INT32_MAX) return SR_EINVAL;
  const int nchunks = (int)sr_cdiv(nv, SMPL_SKIN_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nchunks, (unsigned)sr_cdiv(B, SMPL_BT)), block(SMPL_SKIN_BLOCK);
  hipLaunchKernelGGL(smpl_skin_bwd_kernel, grid, block, 0, s, rest, rest_batch_stride, posedirs, feature, weights, A, gV, B, (int)nv, g_rest, partial);
  const int nf = posedirs ? SMPL_NPOSE : 0;
  hipLaunchKernelGGL(smpl_skin_bwd_final_kernel, dim3((unsigned)sr_cdiv((int64_t)B * (GA_ROW + nf), SMPL_EW_BLOCK)), dim3(SMPL_EW_BLOCK), 0, s, partial, B,
                     nchunks, nf, gA, g_feature);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ pose stage
// gG: this thread's cotangent of the chain matrices G (rows 0..2 of each 4x4), element e of joint j at sm[(j * 12 + e) * POSE_T + thread]
struct pose_lds {
  float* base;
  __device__ __forceinline__ float& operator()(int joint, int e) const { return base[(joint * 12 + e) * POSE_T]; }
};

__global__ __launch_bounds__(POSE_T) void smpl_pose_bwd_kernel(const float* __restrict__ theta, const float* __restrict__ Rs, const float* __restrict__ J,
                                                               const float* __restrict__ A, smpl_parents_g parents, int B,
                                                               const float* __restrict__ gA, const float* __restrict__ gJt,
                                                               const float* __restrict__ g_feature, const float* __restrict__ gRs,
                                                               float* __restrict__ g_theta, float* __restrict__ gRs_out, float* gJ) {
  __shared__ float sm[SMPL_NJ * 12 * POSE_T];
  const int b = blockIdx.x * POSE_T + threadIdx.x;
  if (b >= B) return;
  const pose_lds gG{sm + threadIdx.x};
  const float* Jb = J + (int64_t)b * SMPL_NJ * 3;
  const float* Ab = A + (int64_t)b * SMPL_NJ * 16;
  const float* Rb = Rs + (int64_t)b * SMPL_NJ * 9;
  float* gJb = gJ + (int64_t)b * SMPL_NJ * 3;

  // A_i = [G3_i | t_i - G3_i J_i], J_transformed_i = t_i
  for (int i = 0; i < SMPL_NJ; ++i) {
    const float jx = Jb[3 * i], jy = Jb[3 * i + 1], jz = Jb[3 * i + 2];
    float at[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      if (gA) {
        const float* ga = gA + ((int64_t)b * SMPL_NJ + i) * 12 + 4 * r;
        a0 = ga[0]; a1 = ga[1]; a2 = ga[2]; at[r] = ga[3];
      }
      gG(i, 4 * r) = a0 - at[r] * jx; gG(i, 4 * r + 1) = a1 - at[r] * jy; gG(i, 4 * r + 2) = a2 - at[r] * jz;
      gG(i, 4 * r + 3) = at[r] + (gJt ? gJt[((int64_t)b * SMPL_NJ + i) * 3 + r] : 0.f);
    }
    const float* G = Ab + i * 16;
#pragma unroll
    for (int c = 0; c < 3; ++c) gJb[3 * i + c] = -fmaf(G[8 + c], at[2], fmaf(G[4 + c], at[1], G[c] * at[0]));       // -G3^T ga_t
  }
  // the chain, children before parents: G3_i = G3_p R_i, t_i = G3_p (J_i - J_p) + t_p
  for (int i = SMPL_NJ - 1; i >= 0; --i) {
    float g[12], gR[9];
#pragma unroll
    for (int e = 0; e < 12; ++e) g[e] = gG(i, e);
    if (i == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gR[3 * r + c] = g[4 * r + c];
        gJb[r] += g[4 * r + 3];
      }
    } else {
      const int pa = parents.p[i];
      const float* P = Ab + pa * 16;                               // G3 of the parent = rows 0..2, columns 0..2 of its A
      float R[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) R[e] = Rb[i * 9 + e];
      const float rel[3] = {Jb[3 * i] - Jb[3 * pa], Jb[3 * i + 1] - Jb[3 * pa + 1], Jb[3 * i + 2] - Jb[3 * pa + 2]};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          gG(pa, 4 * r + c) += fmaf(g[4 * r + 3], rel[c], fmaf(g[4 * r + 2], R[3 * c + 2], fmaf(g[4 * r + 1], R[3 * c + 1], g[4 * r] * R[3 * c])));
        gG(pa, 4 * r + 3) += g[4 * r + 3];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gR[3 * r + c] = fmaf(P[8 + r], g[8 + c], fmaf(P[4 + r], g[4 + c], P[r] * g[c]));
        const float grel = fmaf(P[8 + r], g[11], fmaf(P[4 + r], g[7], P[r] * g[3]));
        gJb[3 * i + r] += grel;
        gJb[3 * pa + r] -= grel;
      }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      if (gRs) gR[e] += gRs[((int64_t)b * SMPL_NJ + i) * 9 + e];
      if (g_feature && i > 0) gR[e] += g_feature[(int64_t)b * SMPL_NPOSE + (i - 1) * 9 + e];
    }
    if (theta) {
      const float* th = theta + ((int64_t)b * SMPL_NJ + i) * 3;
      Dual D[9];
      const Dual tx{th[0], {1.f, 0.f, 0.f}}, ty{th[1], {0.f, 1.f, 0.f}}, tz{th[2], {0.f, 0.f, 1.f}};
      srrot::rodrigues<Dual>(tx, ty, tz, D);
      float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
      for (int e = 0; e < 9; ++e) { o0 = fmaf(gR[e], D[e].d[0], o0); o1 = fmaf(gR[e], D[e].d[1], o1); o2 = fmaf(gR[e], D[e].d[2], o2); }
      float* o = g_theta + ((int64_t)b * SMPL_NJ + i) * 3;
      o[0] = o0; o[1] = o1; o[2] = o2;
    } else {
#pragma unroll
      for (int e = 0; e < 9; ++e) gRs_out[((int64_t)b * SMPL_NJ + i) * 9 + e] = gR[e];
    }
  }
}

extern "C" int sr_smpl_pose_bwd(const float* theta, const float* Rs, const float* J, const float* A, const int32_t* host_parents, int32_t B,
                                const float* gA, const float* gJ_transformed, const float* g_feature, const float* gRs, float* g_theta,
                                float* gRs_out, float* gJ, void* stream) {
  if (!Rs || !J || !A || !host_parents || !gJ || B < 1) return SR_EINVAL;
  if (theta ? !g_theta : !gRs_out) return SR_EINVAL;
  smpl_parents_g pa;
  pa.p[0] = 0;
  for (int i = 1; i < SMPL_NJ; ++i) {
    if (host_parents[i] < 0 || host_parents[i] >= i) return SR_EINVAL;     // a parent comes before its children
    pa.p[i] = host_parents[i];
  }
  hipLaunchKernelGGL(smpl_pose_bwd_kernel, dim3((unsigned)sr_cdiv(B, POSE_T)), dim3(POSE_T), 0, (hipStream_t)stream, theta, Rs, J, A, pa, B, gA,
                     gJ_transformed, g_feature, gRs, g_theta, gRs_out, gJ);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ keypoint data term
__global__ __launch_bounds__(SR_WAVE) void keypoint_energy_kernel(const float* __restrict__ joints, const float* __restrict__ trans,
                                                                  const float* __restrict__ kp, const float* __restrict__ jw, kp_camera cam, float sigma,
                                                                  int K, float* __restrict__ energy, float* __restrict__ g_joints,
                                                                  float* __restrict__ g_trans, int32_t* __restrict__ behind) {
  __shared__ float term[KP_MAX * 4];
  __shared__ int32_t beh[KP_MAX];
  const int t = blockIdx.x, k = threadIdx.x;
  float e = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
  int isbehind = 0;
  if (k < K) {
    const float* p = joints + ((int64_t)t * K + k) * 3;
    const float* tr = trans + (int64_t)t * 3;
    const float* q = kp + ((int64_t)t * K + k) * 3;
    const float px = p[0] + tr[0], py = p[1] + tr[1], pz = p[2] + tr[2];
    const float kx = q[0], ky = q[1], conf = q[2];
    if (isfinite(kx) && isfinite(ky) && isfinite(conf) && conf != 0.f) {
      const float* R = cam.R;
      const float cx_ = fmaf(pz, R[6], fmaf(py, R[3], px * R[0])) + cam.T[0];
      const float cy_ = fmaf(pz, R[7], fmaf(py, R[4], px * R[1])) + cam.T[1];
      const float cz_ = fmaf(pz, R[8], fmaf(py, R[5], px * R[2])) + cam.T[2];
      if (cz_ > 0.f) {
        const float iz = 1.f / cz_;
        const float dx = cam.cx - cam.fx * cx_ * iz - kx, dy = cam.cy - cam.fy * cy_ * iz - ky;
        const float s = (jw[k] * conf) * (jw[k] * conf), s2 = sigma * sigma;
        const float r2 = dx * dx + dy * dy, den = 1.f / (s2 + r2);
        e = s * s2 * r2 * den;
        const float dr = 2.f * s * (s2 * den) * (s2 * den);             // d e / d (r^2) * 2
        const float gx = dr * dx, gy = dr * dy;
        const float c0 = -cam.fx * iz * gx, c1 = -cam.fy * iz * gy;
        const float c2 = (cam.fx * cx_ * gx + cam.fy * cy_ * gy) * iz * iz;
        g0 = fmaf(R[2], c2, fmaf(R[1], c1, R[0] * c0));
        g1 = fmaf(R[5], c2, fmaf(R[4], c1, R[3] * c0));
        g2 = fmaf(R[8], c2, fmaf(R[7], c1, R[6] * c0));
      } else {
        isbehind = 1;
      }
    }
    float* o = g_joints + ((int64_t)t * K + k) * 3;
    o[0] = g0; o[1] = g1; o[2] = g2;
    term[4 * k] = e; term[4 * k + 1] = g0; term[4 * k + 2] = g1; term[4 * k + 3] = g2;
    beh[k] = isbehind;
  }
  __syncthreads();
  if (k == 0) {
    float se = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    int nbh = 0;
    for (int i = 0; i < K; ++i) { se += term[4 * i]; s0 += term[4 * i + 1]; s1 += term[4 * i + 2]; s2 += term[4 * i + 3]; nbh += beh[i]; }   // ascending joint order
    energy[t] = se;
    g_trans[3 * t] = s0; g_trans[3 * t + 1] = s1; g_trans[3 * t + 2] = s2;
    behind[t] = nbh;
  }
}

extern "C" int sr_keypoint_energy(const float* joints, const float* trans, const float* kp, const float* joint_weights, const float* host_camera,
                                  float sigma, int32_t T, int32_t K, float* energy, float* g_joints, float* g_trans, int32_t* behind, void* stream) {
  if (!joints || !trans || !kp || !joint_weights || !host_camera || !energy || !g_joints || !g_trans || !behind) return SR_EINVAL;
  if (T < 1 || K < 1 || K > KP_MAX || !(sigma > 0.f)) return SR_EINVAL;
  kp_camera cam;
  for (int i = 0; i < 9; ++i) cam.R[i] = host_camera[i];
  for (int i = 0; i < 3; ++i) cam.T[i] = host_camera[9 + i];
  cam.fx = host_camera[12]; cam.fy = host_camera[13]; cam.cx = host_camera[14]; cam.cy = host_camera[15];
  hipLaunchKernelGGL(keypoint_energy_kernel, dim3((unsigned)T), dim3(SR_WAVE), 0, (hipStream_t)stream, joints, trans, kp, joint_weights, cam, sigma, K, energy,
                     g_joints, g_trans, behind);
  return sr_launch_status();
}
