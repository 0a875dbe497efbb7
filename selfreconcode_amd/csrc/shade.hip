// The two Phong-shaded mesh previews of the reference's `infer` (model/network.py:306-337): pytorch3d 0.4.0's HardPhongShader as
// infer.py:80-90 installs it, restated from its published semantics (third-party code that is not in the reference repository;
// parity unpinned):
//
//  * sr_vertex_adjacency + sr_vertex_normals: Meshes.verts_normals_packed of N deformed copies of one template.  pytorch3d
//    scatters the three corner cross products of every face with index_add (float atomics: order-dependent bits); here the
//    template's vertex -> (face, corner) lists are built once as a CSR sorted by 3 f + corner, and the normals are a gather in that
//    fixed order -- two calls give identical bits.
//  * sr_shade_phong: phong_shading (vertex positions and normals interpolated with the rasteriser's barycentrics, one point light,
//    TexturesVertex of ones) + hard_rgb_blend (background colour where pix_to_face < 0, alpha 1).
//
// All of it is a bandwidth-bound gather: no LDS tiling, no MFMA.
#include "sr_common.h"
#include "mesh_device.h"

namespace {

// offsets[v + 1] += number of corners of used faces at v (integer atomics: the counts do not depend on the order)
__global__ __launch_bounds__(256) void adj_count(const int64_t* __restrict__ faces, int64_t V, int64_t F, unsigned long long* __restrict__ offsets) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (!sr_face_ok(a, b, c, V)) continue;
    atomicAdd(offsets + a + 1, 1ull); atomicAdd(offsets + b + 1, 1ull); atomicAdd(offsets + c + 1, 1ull);
  }
}

// in-place inclusive scan of offsets[0 .. n) by one workgroup of 1024 threads, a tile of 1024 entries per step (offsets[0] = 0)
__global__ __launch_bounds__(1024) void adj_scan(int64_t* __restrict__ offsets, int64_t n) {
  __shared__ int64_t wsum[1024 / SR_WAVE];
  const int lane = threadIdx.x & (SR_WAVE - 1), w = threadIdx.x / SR_WAVE;
  int64_t carry = 0;
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + threadIdx.x;
    int64_t x = i < n ? offsets[i] : 0;
#pragma unroll
    for (int d = 1; d < SR_WAVE; d <<= 1) {
      const int64_t y = __shfl_up(x, d, SR_WAVE);
      if (lane >= d) x += y;
    }
    if (lane == SR_WAVE - 1) wsum[w] = x;
    __syncthreads();
    int64_t pre = carry, tile = 0;
    for (int k = 0; k < 1024 / SR_WAVE; ++k) {
      pre += k < w ? wsum[k] : 0;
      tile += wsum[k];
    }
    if (i < n) offsets[i] = x + pre;
    carry += tile;
    __syncthreads();                                  // wsum is rewritten by the next tile
  }
}

// keys[offsets[v] + slot] = 3 f + corner, slots in arrival order (sorted by adj_finish)
__global__ __launch_bounds__(256) void adj_fill(const int64_t* __restrict__ faces, int64_t V, int64_t F, const int64_t* __restrict__ offsets,
                                                 int32_t* __restrict__ cursor, int64_t* __restrict__ keys) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v[3] = {faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2]};
    if (!sr_face_ok(v[0], v[1], v[2], V)) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) keys[offsets[v[c]] + atomicAdd(cursor + v[c], 1)] = 3 * f + c;
  }
}

// per vertex: sort its keys (insertion sort: a marching-cubes vertex has a handful of corners), then replace each key in place by the
// corner's two other vertices (next, previous) -- `pairs` aliases `keys`, and every thread touches its own segment only
__global__ __launch_bounds__(256) void adj_finish(const int64_t* __restrict__ faces, int64_t V, const int64_t* __restrict__ offsets,
                                                   int64_t* keys, int2* pairs) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = offsets[v], e = offsets[v + 1];
    for (int64_t j = b + 1; j < e; ++j) {
      const int64_t k = keys[j];
      int64_t i = j - 1;
      while (i >= b && keys[i] > k) { keys[i + 1] = keys[i]; --i; }
      keys[i + 1] = k;
    }
    for (int64_t j = b; j < e; ++j) {
      const int64_t k = keys[j], f = k / 3;
      const int c = (int)(k - 3 * f);
      const int next = c == 2 ? 0 : c + 1, prev = c == 0 ? 2 : c - 1;
      pairs[j] = make_int2((int)faces[f * 3 + next], (int)faces[f * 3 + prev]);
    }
  }
}

// thread per (image, vertex): n = sum over the vertex's corners, in CSR order, of cross(p_next - p, p_prev - p); n / max(|n|, 1e-6)
__global__ __launch_bounds__(256) void vn_gather(const float* __restrict__ verts, int64_t N, int64_t V, const int64_t* __restrict__ offsets,
                                                  const int2* __restrict__ pairs, float* __restrict__ normals) {
  const int64_t total = N * V;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t img = i / V, v = i - img * V;
    const float* P = verts + img * V * 3;
    const float px = P[v * 3], py = P[v * 3 + 1], pz = P[v * 3 + 2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    const int64_t e = offsets[v + 1];
    for (int64_t j = offsets[v]; j < e; ++j) {
      const int2 q = pairs[j];
      const float ux = P[(int64_t)q.x * 3] - px, uy = P[(int64_t)q.x * 3 + 1] - py, uz = P[(int64_t)q.x * 3 + 2] - pz;
      const float wx = P[(int64_t)q.y * 3] - px, wy = P[(int64_t)q.y * 3 + 1] - py, wz = P[(int64_t)q.y * 3 + 2] - pz;
      nx += uy * wz - uz * wy; ny += uz * wx - ux * wz; nz += ux * wy - uy * wx;
    }
    const float d = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-6f);     // F.normalize(eps = 1e-6)
    normals[i * 3] = nx / d; normals[i * 3 + 1] = ny / d; normals[i * 3 + 2] = nz / d;
  }
}

struct Phong { float ka[3], kd[3], ks[3], shininess, bg[3]; };

__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
  const float d = fmaxf(sqrtf(x * x + y * y + z * z), 1e-6f);
  x /= d; y /= d; z /= d;
}

// thread per pixel; one 16-byte store of (r, g, b, 1)
__global__ __launch_bounds__(256) void phong_shade(const float* __restrict__ verts, const float* __restrict__ normals, const int64_t* __restrict__ faces,
                                                    int64_t N, int64_t V, int64_t F, int64_t HW, const int64_t* __restrict__ pix_to_face,
                                                    const float* __restrict__ bary, const float* __restrict__ cam, const float* __restrict__ light,
                                                    Phong ph, float4* __restrict__ rgba) {
  const int64_t total = N * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = pix_to_face[i];
    float4 o = make_float4(ph.bg[0], ph.bg[1], ph.bg[2], 1.f);
    if (p >= 0 && p < N * F) {
      const int64_t fi = p / F, f = p - fi * F;              // packed index: the face's mesh is image fi
      const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
      if (sr_face_ok(a, b, c, V)) {
        const float b0 = bary[i * 3], b1 = bary[i * 3 + 1], b2 = bary[i * 3 + 2];
        const float* P = verts + fi * V * 3;
        const float* Q = normals + fi * V * 3;
        float x = b0 * P[a * 3] + b1 * P[b * 3] + b2 * P[c * 3];
        float y = b0 * P[a * 3 + 1] + b1 * P[b * 3 + 1] + b2 * P[c * 3 + 1];
        float z = b0 * P[a * 3 + 2] + b1 * P[b * 3 + 2] + b2 * P[c * 3 + 2];
        float nx = b0 * Q[a * 3] + b1 * Q[b * 3] + b2 * Q[c * 3];
        float ny = b0 * Q[a * 3 + 1] + b1 * Q[b * 3 + 1] + b2 * Q[c * 3 + 1];
        float nz = b0 * Q[a * 3 + 2] + b1 * Q[b * 3 + 2] + b2 * Q[c * 3 + 2];
        const int64_t img = i / HW;                          // lights and cameras are per image
        float lx = light[img * 3] - x, ly = light[img * 3 + 1] - y, lz = light[img * 3 + 2] - z;
        float vx = cam[img * 3] - x, vy = cam[img * 3 + 1] - y, vz = cam[img * 3 + 2] - z;
        normalize3(nx, ny, nz); normalize3(lx, ly, lz); normalize3(vx, vy, vz);
        const float cosl = nx * lx + ny * ly + nz * lz;
        const float diff = fmaxf(cosl, 0.f);
        const float rx = 2.f * (cosl * nx) - lx, ry = 2.f * (cosl * ny) - ly, rz = 2.f * (cosl * nz) - lz;
        const float al = cosl > 0.f ? fmaxf(vx * rx + vy * ry + vz * rz, 0.f) : 0.f;
        const float spec = powf(al, ph.shininess);
        const float texel = b0 + b1 + b2;                    // TexturesVertex of ones
        o.x = (ph.ka[0] + ph.kd[0] * diff) * texel + ph.ks[0] * spec;
        o.y = (ph.ka[1] + ph.kd[1] * diff) * texel + ph.ks[1] * spec;
        o.z = (ph.ka[2] + ph.kd[2] * diff) * texel + ph.ks[2] * spec;
      }
    }
    rgba[i] = o;
  }
}
}  // namespace

extern "C" int sr_vertex_adjacency(const int64_t* faces, int64_t V, int64_t F, int64_t* offsets, int32_t* cursor, int32_t* nbr, void* stream) {
  if (!faces || !offsets || !cursor || !nbr || V <= 0 || F <= 0 || F >= ((int64_t)1 << 32) || V > INT32_MAX || ((uintptr_t)nbr & 7))
    return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(offsets, 0, (size_t)(V + 1) * 8, st) != hipSuccess || hipMemsetAsync(cursor, 0, (size_t)V * 4, st) != hipSuccess)
    return SR_ELAUNCH;
  const int g = sr_stream_grid(F, 256);
  hipLaunchKernelGGL(adj_count, dim3(g), dim3(256), 0, st, faces, V, F, (unsigned long long*)offsets);
  hipLaunchKernelGGL(adj_scan, dim3(1), dim3(1024), 0, st, offsets, V + 1);
  hipLaunchKernelGGL(adj_fill, dim3(g), dim3(256), 0, st, faces, V, F, (const int64_t*)offsets, cursor, (int64_t*)nbr);
  sr_launch_stream(adj_finish, V, 256, st, faces, V, (const int64_t*)offsets, (int64_t*)nbr, (int2*)nbr);
  return sr_launch_status();
}

extern "C" int sr_vertex_normals(const float* verts, int64_t N, int64_t V, const int64_t* offsets, const int32_t* nbr, float* normals, void* stream) {
  if (!verts || !offsets || !nbr || !normals || N <= 0 || V <= 0 || V > INT32_MAX || ((uintptr_t)nbr & 7)) return SR_EINVAL;
  sr_launch_stream(vn_gather, N * V, 256, stream, verts, N, V, offsets, (const int2*)nbr, normals);
  return sr_launch_status();
}

extern "C" int sr_shade_phong(const float* verts, const float* normals, const int64_t* faces, int64_t N, int64_t V, int64_t F, int32_t H, int32_t W,
                              const int64_t* pix_to_face, const float* bary, const float* cam_pos, const float* light_loc, const float* host_phong,
                              float* rgba, void* stream) {
  if (!verts || !normals || !faces || !pix_to_face || !bary || !cam_pos || !light_loc || !host_phong || !rgba || N <= 0 || V <= 0 || F <= 0 ||
      H <= 0 || W <= 0 || F >= ((int64_t)1 << 32) || ((uintptr_t)rgba & 15))
    return SR_EINVAL;
  Phong ph;
  for (int k = 0; k < 3; ++k) {
    ph.ka[k] = host_phong[k]; ph.kd[k] = host_phong[3 + k]; ph.ks[k] = host_phong[6 + k]; ph.bg[k] = host_phong[10 + k];
  }
  ph.shininess = host_phong[9];
  const int64_t HW = (int64_t)H * W;
  sr_launch_stream(phong_shade, N * HW, 256, stream, verts, normals, faces, N, V, F, HW, pix_to_face, bary, cam_pos, light_loc, ph, (float4*)rgba);
  return sr_launch_status();
}
