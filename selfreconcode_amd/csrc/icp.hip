// Point-to-plane ICP of surface samples against a triangle mesh (semantics stated there, this package's own, held to
// a float64 restatement): two launches per iteration and no host contact until the last one has run.
//
//  * sr_icp_accumulate: one lane per sample, grid-stride over a block count fixed from S alone.  q = fl32(M p + t) from the float64
//    state, the float32 grid search of surfdist_device.h (the triple of sr_surfdist_query, bit for bit), the face's unit normal in
//    double, and the row [a | r] of the normalised point-to-plane system.  The upper triangle of [a | r]^T [a | r] (36 sums), the
//    count of kept pairs and the sum of d^2 stay in registers across the stride loop, are reduced over the wave with shuffles and
//    over the four waves through the LDS, and leave as one row of partial [blocks, 40] per block.  No atomics; distances, faces and
//    closest points never reach memory.
//  * sr_icp_solve: one wave.  Lane k sums column k of `partial` over the blocks in ascending order; lane 0 solves the scaled normal
//    equations by Cholesky (a pivot below 2^-20 drops its unknown), composes the update with the exact rotation exp(omega) and
//    writes the state, a row of `history` and the `done` flag.
//  * sr_icp_score: one 256-lane workgroup per candidate transform of a table, lanes striding over the samples.  The
//    same q and the same grid search; min(d, trunc)^2 and a count stay in registers, are reduced over the wave by sr_wave_sum and over
//    the four waves through the LDS, and leave as score [c] = (sum, count).  No atomics.
//
// Once `done` is set both kernels return without touching the state (sr_icp_solve repeats the last history row), so the number of
// launches is fixed before the loop starts.  Everything in double is compiled without contraction and in a stated order, so a sum of
// one sample is the restatement's to the bit and two runs give identical bits.  Every loop runs over an integer range fixed before it
// starts.
#include "sr_wave.h"
#include "surfdist_device.h"

#define ICP_SUMS 38                                    /* 36 products, the kept count, the sum of d^2 */
#define ICP_TABLE 12                                   /* doubles per candidate transform: M (row major), t */
#define ICP_UNKNOWNS 7                                 /* omega (3), tau (3), sigma */
#define ICP_PIVOT_MIN 9.5367431640625e-7               /* 2^-20, on the system scaled to a unit diagonal */
#define ICP_COLUMN_MIN 1.4210854715202004e-14          /* 2^-46 = (2^-23)^2: a column whose mean square is below it is dropped */

namespace {
using namespace srsd;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = SR_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, SR_WAVE);
  return v;                                            // (lane 0 holds the sum)
}

__global__ __launch_bounds__(256) void icp_accumulate(const float* __restrict__ points, int64_t S, const float4* __restrict__ tri, int64_t F,
                                                       const float* __restrict__ lo, float cell, int32_t nx, int32_t ny, int32_t nz,
                                                       const int64_t* __restrict__ cell_start, const int32_t* __restrict__ cell_faces,
                                                       int64_t pairs, const double* __restrict__ state, double ox, double oy, double oz, double rho,
                                                       float max_dist, int32_t measure, double* __restrict__ partial) {
#pragma clang fp contract(off)
  if (!measure && state[SR_ICP_DONE] != 0.) return;    // (uniform over the grid)
  const Grid g{tri, F, lo, cell, nx, ny, nz, cell_start, cell_faces, pairs};
  double M[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = state[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = state[9 + k];
  double acc[ICP_SUMS];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) acc[k] = 0.;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (int64_t)gridDim.x * blockDim.x) {
    const double px = (double)points[i * 3], py = (double)points[i * 3 + 1], pz = (double)points[i * 3 + 2];
    const float q[3] = {(float)(((M[0] * px + M[1] * py) + M[2] * pz) + t[0]), (float)(((M[3] * px + M[4] * py) + M[5] * pz) + t[1]),
                        (float)(((M[6] * px + M[7] * py) + M[8] * pz) + t[2])};
    if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) continue;
    const Best b = grid_search(q, g);
    if (b.f == INT32_MAX) continue;
    const float d = sqrtf(b.d2);
    if (!(d <= max_dist)) continue;
    const Tri f = load_tri(tri, b.f);
    const double ux = (double)f.bx - (double)f.ax, uy = (double)f.by - (double)f.ay, uz = (double)f.bz - (double)f.az;
    const double vx = (double)f.cx - (double)f.ax, vy = (double)f.cy - (double)f.ay, vz = (double)f.cz - (double)f.az;
    double n0 = uy * vz - uz * vy, n1 = uz * vx - ux * vz, n2 = ux * vy - uy * vx;
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    if (len > 0.) { n0 = n0 / len; n1 = n1 / len; n2 = n2 / len; } else { n0 = 0.; n1 = 0.; n2 = 0.; }
    const double x0 = ((double)q[0] - ox) / rho, x1 = ((double)q[1] - oy) / rho, x2 = ((double)q[2] - oz) / rho;
    const double e0 = (double)q[0] - (double)b.qx, e1 = (double)q[1] - (double)b.qy, e2 = (double)q[2] - (double)b.qz;
    const double w[8] = {x1 * n2 - x2 * n1, x2 * n0 - x0 * n2, x0 * n1 - x1 * n0, n0, n1, n2, (n0 * x0 + n1 * x1) + n2 * x2,
                         ((n0 * e0 + n1 * e1) + n2 * e2) / rho};
    int k = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int l = j; l < 8; ++l, ++k) acc[k] += w[j] * w[l];
    acc[36] += 1.;
    acc[37] += (double)d * (double)d;
  }
  __shared__ double red[4][ICP_SUMS];
  const int lane = threadIdx.x & (SR_WAVE - 1), wave = threadIdx.x / SR_WAVE;
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < SR_ICP_COLS) {
    const int k = threadIdx.x;
    partial[(int64_t)blockIdx.x * SR_ICP_COLS + k] = k < ICP_SUMS ? ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k] : 0.;
  }
}

// position of (j, l), j <= l < 8, in the row-major upper triangle
__device__ __forceinline__ int tri_index(int j, int l) { return j * 8 - j * (j - 1) / 2 + (l - j); }

// exp of the rotation vector w, row major: the half-angle quaternion of rot_device.h in double, without its +1e-8 (which belongs to
// the SMPL convention, not to a rotation), normalised before the matrix is formed
__device__ __forceinline__ void rotation_exp(const double (&w)[3], double (&R)[9]) {
#pragma clang fp contract(off)
  const double angle = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  double qw = 1., qx = 0., qy = 0., qz = 0.;
  if (angle > 0.) {
    const double half = 0.5 * angle, k = sin(half) / angle;
    qw = cos(half); qx = k * w[0]; qy = k * w[1]; qz = k * w[2];
    const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw = qw / qn; qx = qx / qn; qy = qy / qn; qz = qz / qn;
  }
  const double w2 = qw * qw, x2 = qx * qx, y2 = qy * qy, z2 = qz * qz;
  const double wx = qw * qx, wy = qw * qy, wz = qw * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz;
  R[0] = ((w2 + x2) - y2) - z2; R[1] = 2. * xy - 2. * wz; R[2] = 2. * wy + 2. * xz;
  R[3] = 2. * wz + 2. * xy; R[4] = ((w2 - x2) + y2) - z2; R[5] = 2. * yz - 2. * wx;
  R[6] = 2. * xz - 2. * wy; R[7] = 2. * wx + 2. * yz; R[8] = ((w2 - x2) - y2) + z2;
}

__global__ __launch_bounds__(SR_WAVE) void icp_solve(const double* __restrict__ partial, int32_t blocks, double ox, double oy, double oz, double rho,
                                                      int32_t scale, double tol, int32_t it, double* __restrict__ state,
                                                      double* __restrict__ history) {
#pragma clang fp contract(off)
  __shared__ double sum[SR_ICP_COLS];
  const int tid = threadIdx.x;
  if (state[SR_ICP_DONE] != 0.) {                      // frozen: the last live row again, done = 1
    if (tid < SR_ICP_HISTORY) history[it * SR_ICP_HISTORY + tid] = tid == SR_ICP_HISTORY - 1 ? 1. : it > 0 ? history[(it - 1) * SR_ICP_HISTORY + tid] : 0.;
    return;
  }
  if (tid < SR_ICP_COLS) {
    double v = 0.;
    for (int32_t b = 0; b < blocks; ++b) v += partial[(int64_t)b * SR_ICP_COLS + tid];
    sum[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  constexpr int U = ICP_UNKNOWNS;
  const int nu = scale ? U : U - 1;
  const double count = sum[36];
  double A[U][U], L[U][U], rhs[U], dsc[U], y[U], xi[U];
  bool keep[U];
  for (int j = 0; j < U; ++j) {
    const double h = sum[tri_index(j, j)];
    keep[j] = j < nu && h > count * ICP_COLUMN_MIN;
    dsc[j] = keep[j] ? 1. / sqrt(h) : 0.;
    y[j] = 0.; xi[j] = 0.;
    for (int l = 0; l < U; ++l) L[j][l] = 0.;
  }
  for (int j = 0; j < U; ++j) {
    for (int l = 0; l < U; ++l) A[j][l] = (sum[j <= l ? tri_index(j, l) : tri_index(l, j)] * dsc[j]) * dsc[l];
    rhs[j] = -(sum[tri_index(j, 7)] * dsc[j]);
  }
  int rank = 0;
  for (int j = 0; j < U; ++j) {                        // Cholesky, column by column; an unknown without a pivot leaves the system
    if (!keep[j]) continue;
    double p = A[j][j];
    for (int k = 0; k < j; ++k) p -= L[j][k] * L[j][k];
    if (!(p >= ICP_PIVOT_MIN)) {
      keep[j] = false;
      for (int k = 0; k < j; ++k) L[j][k] = 0.;
      continue;
    }
    ++rank;
    L[j][j] = sqrt(p);
    for (int i = j + 1; i < U; ++i) {
      if (!keep[i]) continue;
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  for (int j = 0; j < U; ++j) {
    if (!keep[j]) continue;
    double v = rhs[j];
    for (int k = 0; k < j; ++k) v -= L[j][k] * y[k];
    y[j] = v / L[j][j];
  }
  for (int j = U - 1; j >= 0; --j) {
    if (!keep[j]) continue;
    double v = y[j];
    for (int i = j + 1; i < U; ++i)
      if (keep[i]) v -= L[i][j] * xi[i];
    xi[j] = v / L[j][j];
  }
  double step = 0.;
  for (int j = 0; j < U; ++j) {
    xi[j] = keep[j] ? xi[j] * dsc[j] : 0.;
    step = fmax(step, fabs(xi[j]));
  }
  bool finite = true;
  for (int j = 0; j < U; ++j) finite = finite && isfinite(xi[j]);
  if (!finite) {                                       // (sums that overflowed: no update, and the loop ends)
    for (int j = 0; j < U; ++j) xi[j] = 0.;
    step = 0.; rank = 0;
  }
  const double omega[3] = {xi[0], xi[1], xi[2]};
  double R[9], M[9], N[9];
  rotation_exp(omega, R);
  const double sd = 1. + xi[6];
  for (int k = 0; k < 9; ++k) M[k] = state[k];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) N[i * 3 + j] = sd * ((R[i * 3] * M[j] + R[i * 3 + 1] * M[3 + j]) + R[i * 3 + 2] * M[6 + j]);
  const double o[3] = {ox, oy, oz};
  const double v[3] = {state[9] - ox, state[10] - oy, state[11] - oz};
  double tn[3];
  for (int i = 0; i < 3; ++i) tn[i] = (o[i] + sd * ((R[i * 3] * v[0] + R[i * 3 + 1] * v[1]) + R[i * 3 + 2] * v[2])) + rho * xi[3 + i];
  double ss = 0.;
  for (int k = 0; k < 9; ++k) ss += N[k] * N[k];
  const bool done = step < tol;
  for (int k = 0; k < 9; ++k) state[k] = N[k];
  for (int k = 0; k < 3; ++k) state[9 + k] = tn[k];
  state[SR_ICP_DONE] = done ? 1. : 0.;
  state[SR_ICP_DONE + 1] = (double)(it + 1);
  double* row = history + (int64_t)it * SR_ICP_HISTORY;
  row[0] = count;
  row[1] = count > 0. ? sqrt(sum[37] / count) : 0.;
  row[2] = step;
  row[3] = (double)rank;
  row[4] = sqrt(ss / 3.);
  row[5] = done ? 1. : 0.;
}

// One workgroup per candidate c: T_c(p) = M p + t from row c of table [N, ICP_TABLE].  The samples come sorted by their cell keys in
// their own mesh's grid; a similarity keeps neighbours neighbours, so a wave walks adjacent cells of the target under every candidate.
// A candidate far from the target walks many rings: exactness is kept.
__global__ __launch_bounds__(256) void icp_score(const float* __restrict__ points, int64_t S, const double* __restrict__ table,
                                                  const float4* __restrict__ tri, int64_t F, const float* __restrict__ lo, float cell, int32_t nx,
                                                  int32_t ny, int32_t nz, const int64_t* __restrict__ cell_start,
                                                  const int32_t* __restrict__ cell_faces, int64_t pairs, const float* __restrict__ trunc,
                                                  double* __restrict__ score) {
#pragma clang fp contract(off)
  const Grid g{tri, F, lo, cell, nx, ny, nz, cell_start, cell_faces, pairs};
  const double* __restrict__ row = table + (int64_t)blockIdx.x * ICP_TABLE;
  double M[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = row[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = row[9 + k];
  const float cap = trunc[blockIdx.x];
  double sum = 0., count = 0.;
  for (int64_t i = threadIdx.x; i < S; i += 256) {
    const double px = (double)points[i * 3], py = (double)points[i * 3 + 1], pz = (double)points[i * 3 + 2];
    const float q[3] = {(float)(((M[0] * px + M[1] * py) + M[2] * pz) + t[0]), (float)(((M[3] * px + M[4] * py) + M[5] * pz) + t[1]),
                        (float)(((M[6] * px + M[7] * py) + M[8] * pz) + t[2])};
    if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) continue;
    const Best b = grid_search(q, g);
    if (b.f == INT32_MAX) continue;
    const float e = fminf(sqrtf(b.d2), cap);
    sum += (double)e * (double)e;
    count += 1.;
  }
  __shared__ double red[4][2];
  const int lane = threadIdx.x & (SR_WAVE - 1), wave = threadIdx.x / SR_WAVE;
  sum = sr_wave_sum(sum);
  count = sr_wave_sum(count);
  if (lane == 0) { red[wave][0] = sum; red[wave][1] = count; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int k = threadIdx.x;
    score[(int64_t)blockIdx.x * 2 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

int32_t icp_blocks(int64_t S) {
  const int64_t b = sr_cdiv(S, 256);
  return (int32_t)(b < SR_ICP_MAX_BLOCKS ? b : SR_ICP_MAX_BLOCKS);
}
bool bad_frame(double ox, double oy, double oz, double rho) { return !isfinite(ox) || !isfinite(oy) || !isfinite(oz) || !(rho > 0.) || !isfinite(rho); }
}  // namespace

extern "C" int sr_icp_accumulate(const float* points, int64_t S, const float* tri, int64_t F, const float* lo, float cell, int32_t nx, int32_t ny,
                                 int32_t nz, const int64_t* cell_start, const int32_t* cell_faces, int64_t pairs, const double* state, double ox,
                                 double oy, double oz, double rho, float max_dist, int32_t measure, double* partial, int32_t blocks, void* stream) {
  if (!points || !tri || !lo || !cell_start || !cell_faces || !state || !partial || S <= 0 || F <= 0 || F >= INT32_MAX || pairs < 0 ||
      misaligned(tri) || bad_grid(cell, nx, ny, nz) || bad_frame(ox, oy, oz, rho) || !(max_dist >= 0.f) || blocks != icp_blocks(S))
    return SR_EINVAL;
  hipLaunchKernelGGL(icp_accumulate, dim3(blocks), dim3(256), 0, (hipStream_t)stream, points, S, (const float4*)tri, F, lo, cell, nx, ny, nz,
                     cell_start, cell_faces, pairs, state, ox, oy, oz, rho, max_dist, measure, partial);
  return sr_launch_status();
}

extern "C" int sr_icp_solve(const double* partial, int32_t blocks, double ox, double oy, double oz, double rho, int32_t scale, double tol,
                            int32_t it, int32_t iters, double* state, double* history, void* stream) {
  if (!partial || !state || !history || blocks <= 0 || blocks > SR_ICP_MAX_BLOCKS || iters <= 0 || it < 0 || it >= iters ||
      bad_frame(ox, oy, oz, rho) || !(tol >= 0.))
    return SR_EINVAL;
  hipLaunchKernelGGL(icp_solve, dim3(1), dim3(SR_WAVE), 0, (hipStream_t)stream, partial, blocks, ox, oy, oz, rho, scale, tol, it, state, history);
  return sr_launch_status();
}

extern "C" int sr_icp_score(const float* points, int64_t S, const double* table, int32_t N, const float* tri, int64_t F, const float* lo, float cell,
                            int32_t nx, int32_t ny, int32_t nz, const int64_t* cell_start, const int32_t* cell_faces, int64_t pairs,
                            const float* trunc, double* score, void* stream) {
  if (!points || !table || !tri || !lo || !cell_start || !cell_faces || !trunc || !score || S <= 0 || N <= 0 || F <= 0 || F >= INT32_MAX ||
      pairs < 0 || misaligned(tri) || bad_grid(cell, nx, ny, nz))
    return SR_EINVAL;
  hipLaunchKernelGGL(icp_score, dim3(N), dim3(256), 0, (hipStream_t)stream, points, S, table, (const float4*)tri, F, lo, cell, nx, ny, nz,
                     cell_start, cell_faces, pairs, trunc, score);
  return sr_launch_status();
}
