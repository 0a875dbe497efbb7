// SMPL body model, forward only, float32 (smpl_pytorch/SMPL.py:93-173 and smpl_pytorch/util.py:35-103 of the reference).
//   smpl_shape_kernel:   v_shaped = v_template + shapedirs . beta, one thread per (batch item, coordinate).
//   smpl_regress_*:      out[b,k,:] = sum_v reg[v,k] x[b,v,:] (rest joints from v_shaped, regressed joints from verts).  A workgroup
//     sums SMPL_CHUNK vertices in ascending order into one partial row; a second launch adds the partial rows in ascending order.
//   smpl_pose_kernel:    one thread per batch item: axis-angle -> rotation by the reference's route (|theta + 1e-8|, half-angle
//     quaternion, normalise, quat2mat), the pose feature (R[1:] - I), the 24-step chain and A = G - pad(G [J;0]).  The chain keeps
//     its matrices in the A output (each thread reads back only what it wrote itself).
//   smpl_skin_kernel:    one thread per vertex, SR_SMPL_BATCH_TILE batch items per workgroup.  The tile's pose features ([207][tile],
//     so that one vertex reads the tile's values of a basis vector as two 16-byte LDS reads) and skinning matrices ([tile][24][12])
//     live in LDS.  posedirs is [207, nv, 3] (the reference's buffer): for one basis vector consecutive threads read consecutive
//     12-byte rows, and a workgroup streams its slice of the array once per batch tile, not once per frame.  The blended v_posed
//     of the tile is parked in LDS ([tile][3][thread]) so that the skinning loop over the tile's items is a rolled loop around one
//     unrolled 24 x 12 blend with the vertex's weights in registers.
// No atomics anywhere: two calls give identical bits.
#include "sr_common.h"
#include "rot_device.h"

#define SMPL_NJ 24
#define SMPL_NPOSE 207                    // 23 x 9
#define SMPL_BT SR_SMPL_BATCH_TILE
#define SMPL_SKIN_BLOCK 128
#define SMPL_CHUNK 128                    // vertices per partial sum of the regressions (= its block size)
#define SMPL_EW_BLOCK 256

struct smpl_parents { int32_t p[SMPL_NJ]; };

// ------------------------------------------------------------------------------------------------ shape blend
__global__ __launch_bounds__(SMPL_EW_BLOCK) void smpl_shape_kernel(const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                                   const float* __restrict__ beta, int nbeta, int64_t n3,
                                                                   float* __restrict__ v_shaped) {
  const int64_t i = (int64_t)blockIdx.x * SMPL_EW_BLOCK + threadIdx.x;
  if (i >= n3) return;
  const float* bt = beta + (int64_t)blockIdx.y * nbeta;          // wave-uniform
  float acc = 0.f;
  for (int k = 0; k < nbeta; ++k) acc = fmaf(bt[k], shapedirs[(int64_t)k * n3 + i], acc);
  v_shaped[(int64_t)blockIdx.y * n3 + i] = acc + v_template[i];
}

extern "C" int sr_smpl_shape(const float* v_template, const float* shapedirs, const float* beta, int32_t B, int32_t nbeta, int64_t nv,
                             float* v_shaped, void* stream) {
  if (!v_template || !shapedirs || !beta || !v_shaped || B < 1 || B > 65535 || nbeta < 1 || nv < 1 || nv > INT32_MAX / 4) return SR_EINVAL;
  const int64_t n3 = 3 * nv;
  const dim3 grid((unsigned)sr_cdiv(n3, SMPL_EW_BLOCK), (unsigned)B), block(SMPL_EW_BLOCK);
  hipLaunchKernelGGL(smpl_shape_kernel, grid, block, 0, (hipStream_t)stream, v_template, shapedirs, beta, nbeta, n3, v_shaped);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ joint regressions
__global__ __launch_bounds__(SMPL_CHUNK) void smpl_regress_partial_kernel(const float* __restrict__ x, const float* __restrict__ reg, int nv, int nk,
                                                                          float* __restrict__ partial) {
  __shared__ float xs[SMPL_CHUNK * 3];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x, t = threadIdx.x;
  const int v0 = chunk * SMPL_CHUNK;
  const int n = min(SMPL_CHUNK, nv - v0);
  const float* xb = x + ((int64_t)b * nv + v0) * 3;
  for (int e = t; e < 3 * n; e += SMPL_CHUNK) xs[e] = xb[e];
  __syncthreads();
  if (t >= 3 * nk) return;
  const int k = t / 3, c = t % 3;
  const float* r = reg + (int64_t)v0 * nk + k;
  float acc = 0.f;
  for (int v = 0; v < n; ++v) acc = fmaf(r[(int64_t)v * nk], xs[3 * v + c], acc);      // ascending vertex order
  partial[((int64_t)b * nchunks + chunk) * (3 * nk) + t] = acc;
}

__global__ __launch_bounds__(SMPL_EW_BLOCK) void smpl_regress_final_kernel(const float* __restrict__ partial, int B, int nchunks, int row,
                                                                           float* __restrict__ out) {
  const int i = blockIdx.x * SMPL_EW_BLOCK + threadIdx.x;
  if (i >= B * row) return;
  const int b = i / row, e = i % row;
  const float* p = partial + (int64_t)b * nchunks * row + e;
  float acc = 0.f;
  for (int c = 0; c < nchunks; ++c) acc += p[(int64_t)c * row];                         // ascending chunk order
  out[i] = acc;
}

extern "C" int64_t sr_smpl_regress_workspace_floats(int32_t B, int64_t nv, int32_t nk) {
  if (B < 1 || nv < 1 || nk < 1) return -1;
  return (int64_t)B * sr_cdiv(nv, SMPL_CHUNK) * 3 * nk;
}

extern "C" int sr_smpl_regress(const float* x, const float* reg, int32_t B, int64_t nv, int32_t nk, float* partial, float* out, void* stream) {
  if (!x || !reg || !partial || !out || B < 1 || B > 65535 || nv < 1 || nv > INT32_MAX / 4 || nk < 1 || 3 * nk > SMPL_CHUNK) return SR_EINVAL;
  if (nv * nk > INT32_MAX || (int64_t)B * 3 * nk > INT32_MAX) return SR_EINVAL;
  const int nchunks = (int)sr_cdiv(nv, SMPL_CHUNK);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(smpl_regress_partial_kernel, dim3((unsigned)nchunks, (unsigned)B), dim3(SMPL_CHUNK), 0, s, x, reg, (int)nv, nk, partial);
  hipLaunchKernelGGL(smpl_regress_final_kernel, dim3((unsigned)sr_cdiv((int64_t)B * 3 * nk, SMPL_EW_BLOCK)), dim3(SMPL_EW_BLOCK), 0, s, partial, B, nchunks,
                     3 * nk, out);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ pose stage
__global__ __launch_bounds__(SR_WAVE) void smpl_pose_kernel(const float* __restrict__ theta, float* Rs, const float* __restrict__ J, smpl_parents parents,
                                                            int B, float* __restrict__ feature, float* __restrict__ Jt, float* A) {
  const int b = blockIdx.x * SR_WAVE + threadIdx.x;
  if (b >= B) return;
  float* Rb = Rs + (int64_t)b * SMPL_NJ * 9;
  const float* Jb = J + (int64_t)b * SMPL_NJ * 3;
  float* Ab = A + (int64_t)b * SMPL_NJ * 16;
  float* Jtb = Jt + (int64_t)b * SMPL_NJ * 3;
  for (int i = 0; i < SMPL_NJ; ++i) {
    float R[9];
    if (theta) {
      const float* th = theta + ((int64_t)b * SMPL_NJ + i) * 3;
      srrot::rodrigues<float>(th[0], th[1], th[2], R);
#pragma unroll
      for (int e = 0; e < 9; ++e) Rb[i * 9 + e] = R[e];
    } else {
#pragma unroll
      for (int e = 0; e < 9; ++e) R[e] = Rb[i * 9 + e];
    }
    if (i > 0) {
#pragma unroll
      for (int e = 0; e < 9; ++e) feature[(int64_t)b * SMPL_NPOSE + (i - 1) * 9 + e] = R[e] - ((e % 4 == 0) ? 1.f : 0.f);
    }
    // G_i = G_parent [R_i | J_i - J_parent] (the root: [R_0 | J_0]); rows 0..2 of the 4x4 are kept in A[b,i] until the second pass
    float G[12];
    if (i == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) { G[4 * r] = R[3 * r]; G[4 * r + 1] = R[3 * r + 1]; G[4 * r + 2] = R[3 * r + 2]; G[4 * r + 3] = Jb[r]; }
    } else {
      const int pa = parents.p[i];
      const float* P = Ab + pa * 16;                              // written by this thread in an earlier step
      const float jx = Jb[3 * i] - Jb[3 * pa], jy = Jb[3 * i + 1] - Jb[3 * pa + 1], jz = Jb[3 * i + 2] - Jb[3 * pa + 2];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float p0 = P[4 * r], p1 = P[4 * r + 1], p2 = P[4 * r + 2], p3 = P[4 * r + 3];
#pragma unroll
        for (int c = 0; c < 3; ++c) G[4 * r + c] = fmaf(p2, R[6 + c], fmaf(p1, R[3 + c], p0 * R[c]));
        G[4 * r + 3] = fmaf(p2, jz, fmaf(p1, jy, p0 * jx)) + p3;
      }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) Ab[i * 16 + e] = G[e];
    Jtb[3 * i] = G[3]; Jtb[3 * i + 1] = G[7]; Jtb[3 * i + 2] = G[11];
  }
  // A = G - pad(G [J; 0]): only the translation column changes; the last row is (0, 0, 0, 1)
  for (int i = 0; i < SMPL_NJ; ++i) {
    float* G = Ab + i * 16;
    const float jx = Jb[3 * i], jy = Jb[3 * i + 1], jz = Jb[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) G[4 * r + 3] = G[4 * r + 3] - fmaf(G[4 * r + 2], jz, fmaf(G[4 * r + 1], jy, G[4 * r] * jx));
    G[12] = 0.f; G[13] = 0.f; G[14] = 0.f; G[15] = 1.f;
  }
}

extern "C" int sr_smpl_pose(const float* theta, float* Rs, const float* J, const int32_t* host_parents, int32_t B, float* feature,
                            float* J_transformed, float* A, void* stream) {
  if (!Rs || !J || !host_parents || !feature || !J_transformed || !A || B < 1) return SR_EINVAL;
  smpl_parents pa;
  pa.p[0] = 0;
  for (int i = 1; i < SMPL_NJ; ++i) {
    if (host_parents[i] < 0 || host_parents[i] >= i) return SR_EINVAL;     // a parent comes before its children
    pa.p[i] = host_parents[i];
  }
  hipLaunchKernelGGL(smpl_pose_kernel, dim3((unsigned)sr_cdiv(B, SR_WAVE)), dim3(SR_WAVE), 0, (hipStream_t)stream, theta, Rs, J, pa, B, feature,
                     J_transformed, A);
  return sr_launch_status();
}

// ------------------------------------------------------------------------------------------------ skin stage
__global__ __launch_bounds__(SMPL_SKIN_BLOCK) void smpl_skin_kernel(const float* __restrict__ rest, int64_t rest_stride, const float* __restrict__ posedirs,
                                                                    const float* __restrict__ feature, const float* __restrict__ weights,
                                                                    const float* __restrict__ A, int B, int nv, float* __restrict__ verts) {
  __shared__ __attribute__((aligned(16))) float feat[SMPL_NPOSE * SMPL_BT];          // [k][bb]
  __shared__ __attribute__((aligned(16))) float As[SMPL_BT * SMPL_NJ * 12];          // [bb][j][3x4]
  __shared__ float vp[SMPL_BT * 3 * SMPL_SKIN_BLOCK];                               // [bb][c][thread]
  const int t = threadIdx.x;
  const int b0 = blockIdx.y * SMPL_BT;
  const int nb = min(SMPL_BT, B - b0);
  const int v = blockIdx.x * SMPL_SKIN_BLOCK + t;
  const int vc = min(v, nv - 1);                       // threads past the end compute on the last vertex and store nothing

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

  float acc[SMPL_BT][3];
#pragma unroll
  for (int bb = 0; bb < SMPL_BT; ++bb) { acc[bb][0] = 0.f; acc[bb][1] = 0.f; acc[bb][2] = 0.f; }
  if (posedirs) {
    const float* pd = posedirs + 3 * (int64_t)vc;
    const int64_t n3 = 3 * (int64_t)nv;
#pragma unroll 4
    for (int k = 0; k < SMPL_NPOSE; ++k) {
      const float px = pd[k * n3], py = pd[k * n3 + 1], pz = pd[k * n3 + 2];
      float f[SMPL_BT];
#pragma unroll
      for (int q = 0; q < SMPL_BT / 4; ++q) {
        const float4 u = *reinterpret_cast<const float4*>(&feat[k * SMPL_BT + 4 * q]);
        f[4 * q] = u.x; f[4 * q + 1] = u.y; f[4 * q + 2] = u.z; f[4 * q + 3] = u.w;
      }
#pragma unroll
      for (int bb = 0; bb < SMPL_BT; ++bb) {
        acc[bb][0] = fmaf(f[bb], px, acc[bb][0]); acc[bb][1] = fmaf(f[bb], py, acc[bb][1]); acc[bb][2] = fmaf(f[bb], pz, acc[bb][2]);
      }
    }
  }
#pragma unroll
  for (int bb = 0; bb < SMPL_BT; ++bb) {
    if (bb < nb) {
      const float* r = rest + (int64_t)(b0 + bb) * rest_stride + 3 * (int64_t)vc;
#pragma unroll
      for (int c = 0; c < 3; ++c) vp[(bb * 3 + c) * SMPL_SKIN_BLOCK + t] = acc[bb][c] + r[c];
    }
  }
  // (each thread reads back only its own column of vp: no barrier needed)

  float w[SMPL_NJ];
  const float* wr = weights + (int64_t)vc * SMPL_NJ;
#pragma unroll
  for (int j = 0; j < SMPL_NJ; ++j) w[j] = wr[j];

  for (int bb = 0; bb < nb; ++bb) {
    const float x = vp[(bb * 3) * SMPL_SKIN_BLOCK + t], y = vp[(bb * 3 + 1) * SMPL_SKIN_BLOCK + t], z = vp[(bb * 3 + 2) * SMPL_SKIN_BLOCK + t];
    float* o = verts + ((int64_t)(b0 + bb) * nv + vc) * 3;
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {                       // one row of T = sum_j w_j A_j at a time: four accumulators, 24 16-byte LDS reads
      const float* Ab = As + bb * SMPL_NJ * 12 + 4 * r;
      float T0 = 0.f, T1 = 0.f, T2 = 0.f, T3 = 0.f;
#pragma unroll
      for (int j = 0; j < SMPL_NJ; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(Ab + j * 12);
        T0 = fmaf(w[j], a.x, T0); T1 = fmaf(w[j], a.y, T1); T2 = fmaf(w[j], a.z, T2); T3 = fmaf(w[j], a.w, T3);
      }
      if (v < nv) o[r] = fmaf(T2, z, fmaf(T1, y, T0 * x)) + T3;
    }
  }
}

extern "C" int sr_smpl_skin(const float* rest, int64_t rest_batch_stride, const float* posedirs, const float* feature, const float* weights,
                            const float* A, int32_t B, int64_t nv, float* verts, void* stream) {
  if (!rest || !weights || !A || !verts || B < 1 || nv < 1 || nv > INT32_MAX / 4 || rest_batch_stride < 0) return SR_EINVAL;
  if ((posedirs != nullptr) != (feature != nullptr)) return SR_EINVAL;
  if (sr_cdiv(B, SMPL_BT) > 65535) return SR_EINVAL;
  const dim3 grid((unsigned)sr_cdiv(nv, SMPL_SKIN_BLOCK), (unsigned)sr_cdiv(B, SMPL_BT)), block(SMPL_SKIN_BLOCK);
  hipLaunchKernelGGL(smpl_skin_kernel, grid, block, 0, (hipStream_t)stream, rest, rest_batch_stride, posedirs, feature, weights, A, B, (int)nv, verts);
  return sr_launch_status();
}
