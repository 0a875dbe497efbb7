// Mesh regularisers of the template step (model/network.py:655-670 of the reference): pytorch3d 0.4.0's
// mesh_laplacian_smoothing(method='uniform'), mesh_edge_loss and mesh_normal_consistency on the ONE shared template
// (TmpVs [V,3], Tmpfs), restated (pytorch3d is not available, the semantics are unpinned).
//
//   lap  = (1/V) sum_i |d_i|,  d_i = (1/deg_i) sum_{j in N(i)} (v_j - v_i)   (d_i = -v_i for a vertex no face references)
//   edge = (1/E) sum_e (|v0 - v1| - t)^2
//   nc   = (1/P) sum_p (1 - n0.n1 / max(|n0||n1|, 1e-8)),  n0 = (v1-v0) x (a-v0),  n1 = -(v1-v0) x (b-v0)
//
// The topology (neighbour CSR, pair rows, the (pair, slot) CSR) is built once per remesh on the host side
// (mesh_losses.MeshTopology); per iteration this file is at most FOUR launches for all three terms, forward and backward:
//   1. vertex pass   one thread per vertex over its neighbour row: |d_i| and the edge terms of the edges (i, j > i) as block
//                    partials; q_i = unit(d_i) / max(deg_i, 1) and e_i = sum_j (1 - t/|v_i - v_j|)(v_i - v_j) kept for the backward
//   2. pair pass     one thread per pair row: 1 - c as block partials, -dc/d(v0, v1, a, b) staged per row (12 floats)
//   3. finish        one workgroup adds the block partials in a fixed order and writes the three means
//   4. backward      one thread per vertex GATHERS: sum_j (q_j - q_i) through the neighbour CSR, e_i, and the staged rows through the
//                    (pair, slot) CSR in ascending order, each times its cotangent READ FROM DEVICE MEMORY
// A term that is switched off launches and reads nothing.  No atomics of any kind: every sum has a fixed order, two runs give identical
// bits.  The data are a few MB and the arithmetic a few hundred operations per thread, so the cost is the launches; the arithmetic
// inside a thread is therefore done in double (float32 in memory, double in registers), which costs nothing measurable here and leaves
// the float32 rounding of the stored q / e / staged rows and of the final gradient as the only error against a float64 evaluation.
#include "sr_common.h"
#include "sr_wave.h"

namespace {
constexpr int kBlk = 256;
constexpr double kCosEps = 1e-8;

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ld3(const float* __restrict__ p, int64_t i) { return {(double)p[i * 3], (double)p[i * 3 + 1], (double)p[i * 3 + 2]}; }
__device__ __forceinline__ D3 operator-(const D3& a, const D3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator+(const D3& a, const D3& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator*(double s, const D3& a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(const D3& a, const D3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(const D3& a, const D3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ void st3(float* __restrict__ p, int64_t i, const D3& a) { p[i * 3] = (float)a.x; p[i * 3 + 1] = (float)a.y; p[i * 3 + 2] = (float)a.z; }

// fixed order: lanes of a wave (xor butterfly) -> the waves of the workgroup in ascending order; the total returns in thread 0
__device__ __forceinline__ double block_sum(double v, double* smem /* [kBlk / 64] */) {
  v = sr_wave_sum(v);
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.;
  if (threadIdx.x == 0)
    for (int w = 0; w < kBlk / 64; ++w) t += smem[w];
  __syncthreads();
  return t;
}

// 1. vertex pass.  partial: [gridDim.x] |d_i| sums, then [gridDim.x] edge sums (each edge counted at its lower vertex).
__global__ __launch_bounds__(kBlk) void meshreg_vertex_fwd_kernel(const float* __restrict__ verts, int V, const int32_t* __restrict__ row,
                                                                   const int32_t* __restrict__ nbr, int do_lap, int do_edge, double target,
                                                                   float* __restrict__ lap_q, float* __restrict__ edge_g,
                                                                   double* __restrict__ partial) {
  __shared__ double smem[kBlk / 64];
  const int i = blockIdx.x * kBlk + threadIdx.x;
  double lap = 0., edge = 0.;
  if (i < V) {
    const int b = row[i], e = row[i + 1];
    const D3 vi = ld3(verts, i);
    D3 s = {0., 0., 0.}, es = {0., 0., 0.};
    for (int k = b; k < e; ++k) {
      const int j = nbr[k];
      const D3 d = ld3(verts, j) - vi;                 // differences first: mean(v_j) - v_i loses the direction of d_i in float32
      s = s + d;
      if (do_edge) {
        const double len = sqrt(dot(d, d));
        if (j > i) edge += (len - target) * (len - target);
        const double coef = target > 0. ? (len > 0. ? 1. - target / len : 0.) : 1.;      // zero length with t > 0: gradient 0
        es = es - coef * d;
      }
    }
    if (do_lap) {
      const int deg = e - b;
      const D3 di = deg > 0 ? (1. / (double)deg) * s : -1. * vi;
      lap = sqrt(dot(di, di));
      const double inv = lap > 0. ? 1. / (lap * (double)(deg > 0 ? deg : 1)) : 0.;     // |d_i| = 0: contributes 0, gradient 0
      st3(lap_q, i, inv * di);
    }
    if (do_edge) st3(edge_g, i, es);
  }
  if (do_lap) {
    const double t = block_sum(lap, smem);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
  }
  if (do_edge) {
    const double t = block_sum(edge, smem);
    if (threadIdx.x == 0) partial[gridDim.x + blockIdx.x] = t;
  }
}

// 2. pair pass.  pair_g (optional) [P,4,3]: -dc/d(v0, v1, a, b) of the row, i.e. the gradient of (1 - c).
__global__ __launch_bounds__(kBlk) void meshreg_pair_fwd_kernel(const float* __restrict__ verts, const int4* __restrict__ pairs, int P,
                                                                 float4* __restrict__ pair_g, double* __restrict__ partial) {
  __shared__ double smem[kBlk / 64];
  const int p = blockIdx.x * kBlk + threadIdx.x;
  double term = 0.;
  if (p < P) {
    const int4 ix = pairs[p];
    const D3 v0 = ld3(verts, ix.x);
    const D3 e = ld3(verts, ix.y) - v0, pa = ld3(verts, ix.z) - v0, pb = ld3(verts, ix.w) - v0;
    const D3 n0 = cross(e, pa), n1 = cross(pb, e);
    const double l0 = sqrt(dot(n0, n0)), l1 = sqrt(dot(n1, n1)), prod = l0 * l1;
    const bool clamped = prod < kCosEps;
    const double den = clamped ? kCosEps : prod;
    const double c = dot(n0, n1) / den;
    term = 1. - c;
    if (pair_g) {
      // dc/dn0 = n1 / den - c n0 / |n0|^2 (the second part only while the clamp is inactive: a clamped denominator is a constant)
      const D3 g0 = clamped ? (1. / den) * n1 : (1. / den) * n1 - (c / (l0 * l0)) * n0;
      const D3 g1 = clamped ? (1. / den) * n0 : (1. / den) * n0 - (c / (l1 * l1)) * n1;
      // n0 = e x pa, n1 = pb x e:  d/de = pa x g0 + g1 x pb,  d/dpa = g0 x e,  d/dpb = e x g1
      const D3 ge = cross(pa, g0) + cross(g1, pb), ga = cross(g0, e), gb = cross(e, g1);
      const D3 gv0 = -1. * (ge + ga + gb);
      float4* o = pair_g + (int64_t)p * 3;
      o[0] = make_float4((float)-gv0.x, (float)-gv0.y, (float)-gv0.z, (float)-ge.x);
      o[1] = make_float4((float)-ge.y, (float)-ge.z, (float)-ga.x, (float)-ga.y);
      o[2] = make_float4((float)-ga.z, (float)-gb.x, (float)-gb.y, (float)-gb.z);
    }
  }
  const double t = block_sum(term, smem);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// 3. ordered final sums: thread t adds the partials t, t + 256, ... in ascending order, then the fixed block order.
__device__ __forceinline__ double strided_total(const double* __restrict__ partial, int n, double* smem) {
  double s = 0.;
  for (int b = threadIdx.x; b < n; b += kBlk) s += partial[b];
  return block_sum(s, smem);
}
__global__ __launch_bounds__(kBlk) void meshreg_finish_kernel(const double* __restrict__ partial, int bv, int bp, int do_lap, int do_edge, int do_nc,
                                                               double V, double E, double P, float* __restrict__ out) {
  __shared__ double smem[kBlk / 64];
  const double lap = do_lap ? strided_total(partial, bv, smem) : 0.;
  const double edge = do_edge ? strided_total(partial + bv, bv, smem) : 0.;
  const double nc = do_nc ? strided_total(partial + 2 * bv, bp, smem) : 0.;
  if (threadIdx.x == 0) {
    out[0] = do_lap && V > 0. ? (float)(lap / V) : 0.f;
    out[1] = do_edge && E > 0. ? (float)(edge / E) : 0.f;
    out[2] = do_nc && P > 0. ? (float)(nc / P) : 0.f;
  }
}

// 4. backward: grad_i of  g_lap lap + g_edge edge + g_nc nc.  A null cotangent pointer (or buffer) switches the term off.
__global__ __launch_bounds__(kBlk) void meshreg_bwd_kernel(int V, const int32_t* __restrict__ row, const int32_t* __restrict__ nbr,
                                                            const float* __restrict__ lap_q, const float* __restrict__ edge_g,
                                                            const int32_t* __restrict__ prow, const int32_t* __restrict__ pent,
                                                            const float* __restrict__ pair_g, const float* __restrict__ g_lap,
                                                            const float* __restrict__ g_edge, const float* __restrict__ g_nc, double inv_V,
                                                            double two_inv_E, double inv_P, float* __restrict__ grad) {
  const int i = blockIdx.x * kBlk + threadIdx.x;
  if (i >= V) return;
  D3 acc = {0., 0., 0.};
  if (lap_q && g_lap) {
    // d lap / d v_i = (1/V) (sum_{j in N(i)} u_j / deg_j - u_i) = (1/V) sum_j (q_j - q_i), again as differences; no neighbour: -u_i
    const int b = row[i], e = row[i + 1];
    const D3 qi = ld3(lap_q, i);
    D3 s = e > b ? D3{0., 0., 0.} : -1. * qi;
    for (int k = b; k < e; ++k) s = s + (ld3(lap_q, nbr[k]) - qi);
    acc = acc + ((double)g_lap[0] * inv_V) * s;
  }
  if (edge_g && g_edge) acc = acc + ((double)g_edge[0] * two_inv_E) * ld3(edge_g, i);
  if (pair_g && g_nc) {
    D3 s = {0., 0., 0.};
    for (int k = prow[i], e = prow[i + 1]; k < e; ++k) s = s + ld3(pair_g, pent[k]);      // entry = pair * 4 + slot, ascending
    acc = acc + ((double)g_nc[0] * inv_P) * s;
  }
  st3(grad, i, acc);
}

inline int blocks_of(int64_t n) { return (int)sr_cdiv(n, kBlk); }
}  // namespace

extern "C" int64_t sr_meshreg_workspace_bytes(int64_t V, int64_t P) {
  if (V < 0 || P < 0 || V > INT32_MAX || P > INT32_MAX / 12) return SR_EINVAL;
  return (int64_t)sizeof(double) * (2 * (int64_t)blocks_of(V) + blocks_of(P));
}

extern "C" int sr_meshreg_fwd(const float* verts, int64_t V, const int32_t* nbr_row, const int32_t* nbr, int64_t E, const int32_t* pairs, int64_t P,
                              int32_t terms, float target_length, float* lap_q, float* edge_g, float* pair_g, void* workspace, float* out,
                              void* stream) {
  const int do_lap = terms & SR_MESHREG_LAP, do_edge = terms & SR_MESHREG_EDGE, do_nc = terms & SR_MESHREG_NORMAL;
  if (!verts || !out || !workspace || V < 1 || V > INT32_MAX || E < 0 || P < 0 || P > INT32_MAX / 12 || (terms & ~7) || !(target_length >= 0.f))
    return SR_EINVAL;
  if ((do_lap || do_edge) && (!nbr_row || (E > 0 && !nbr) || 2 * E > INT32_MAX)) return SR_EINVAL;
  if ((do_lap && !lap_q) || (do_edge && !edge_g) || (do_nc && P > 0 && !pairs)) return SR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)workspace;
  const int bv = blocks_of(V), bp = blocks_of(P);
  if (do_lap || do_edge)
    hipLaunchKernelGGL(meshreg_vertex_fwd_kernel, dim3(bv), dim3(kBlk), 0, s, verts, (int)V, nbr_row, nbr, do_lap, do_edge,
                       (double)target_length, lap_q, edge_g, partial);
  if (do_nc && P > 0)
    hipLaunchKernelGGL(meshreg_pair_fwd_kernel, dim3(bp), dim3(kBlk), 0, s, verts, (const int4*)pairs, (int)P, (float4*)pair_g, partial + 2 * bv);
  hipLaunchKernelGGL(meshreg_finish_kernel, dim3(1), dim3(kBlk), 0, s, (const double*)partial, bv, do_nc ? bp : 0, do_lap, do_edge, do_nc, (double)V,
                     (double)E, (double)P, out);
  return sr_launch_status();
}

extern "C" int sr_meshreg_bwd(int64_t V, const int32_t* nbr_row, const int32_t* nbr, int64_t E, const int32_t* pair_row, const int32_t* pair_ent,
                              int64_t P, const float* lap_q, const float* edge_g, const float* pair_g, const float* g_lap, const float* g_edge,
                              const float* g_nc, float* grad, void* stream) {
  if (!grad || V < 1 || V > INT32_MAX || E < 0 || 2 * E > INT32_MAX || P < 0 || P > INT32_MAX / 12) return SR_EINVAL;
  if (lap_q && g_lap && (!nbr_row || (E > 0 && !nbr))) return SR_EINVAL;
  if (P == 0) pair_g = nullptr;
  if (pair_g && g_nc && (!pair_row || !pair_ent)) return SR_EINVAL;
  hipLaunchKernelGGL(meshreg_bwd_kernel, dim3(blocks_of(V)), dim3(kBlk), 0, (hipStream_t)stream, (int)V, nbr_row, nbr, lap_q, edge_g, pair_row, pair_ent,
                     pair_g, g_lap, g_edge, g_nc, 1. / (double)V, E > 0 ? 2. / (double)E : 0., P > 0 ? 1. / (double)P : 0., grad);
  return sr_launch_status();
}
