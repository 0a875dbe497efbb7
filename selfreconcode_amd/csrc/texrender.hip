// Drawing the textured template (render.py): a mip-mapped UV shader on the rasteriser's fragments.  The semantics are
// this package's own (stated in the header, restated in float64 by tests/_texrender_ref.py, unpinned):
//
//  * sr_texture_mips: the atlas as premultiplied (rgb w, w) float4 texels, w = 1 on valid texels and 0 elsewhere, averaged down a 2x
//    pyramid to 1 x 1.  The fourth component is the share of valid texels under a texel: a filter footprint that leaves the filled
//    part of the atlas loses weight instead of picking up the black background, and the shader divides by what is left.
//  * sr_texture_face_lod: one level of detail per (image, face) from the affine map pixel -> uv of the projected triangle.
//  * sr_shade_textured: trilinear sample (four clamp-to-edge taps on two levels) per covered pixel, one 16-byte store per pixel.
//
// The shader is a bandwidth-bound gather like phong_shade: a thread per pixel, 16-byte taps, no LDS tiling, no MFMA, no atomics.
#include "sr_common.h"
#include "mesh_device.h"

namespace {

constexpr int MIP_MAX_LEVELS = 17;         // R <= 65536

struct MipLayout { int32_t L; int32_t side[MIP_MAX_LEVELS]; int64_t off[MIP_MAX_LEVELS]; };

// level l + 1 has side (R_l + 1) / 2, the last level side 1; off: the level's first texel in the concatenated buffer (float4 units)
inline MipLayout mip_layout(int32_t R) {
  MipLayout m;
  int64_t off = 0;
  int l = 0;
  for (int32_t s = R;; s = (s + 1) / 2) {
    m.side[l] = s; m.off[l] = off;
    off += (int64_t)s * s;
    ++l;
    if (s == 1) break;
  }
  m.L = l;
  for (int k = l; k < MIP_MAX_LEVELS; ++k) { m.side[k] = 1; m.off[k] = m.off[l - 1]; }
  return m;
}

template <typename T> __device__ __forceinline__ float texel_value(T x);
template <> __device__ __forceinline__ float texel_value<float>(float x) { return x; }
template <> __device__ __forceinline__ float texel_value<uint8_t>(uint8_t x) { return (float)x / 255.f; }

template <typename T>
__global__ __launch_bounds__(256) void mips_first(const T* __restrict__ tex, const uint8_t* __restrict__ valid, int64_t total, float4* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const float w = (!valid || valid[i]) ? 1.f : 0.f;
    out[i] = make_float4(texel_value<T>(tex[i * 3]) * w, texel_value<T>(tex[i * 3 + 1]) * w, texel_value<T>(tex[i * 3 + 2]) * w, w);
  }
}

// texel (r, c) of the n x n level = the sum of the in-range texels of {2r, 2r + 1} x {2c, 2c + 1} of the m x m level / their number
__global__ __launch_bounds__(256) void mips_next(const float4* __restrict__ src, int32_t m, int32_t n, float4* __restrict__ dst) {
  const int64_t total = (int64_t)n * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / n), c = (int)(i - (int64_t)r * n);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    float cnt = 0.f;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr)
#pragma unroll
      for (int dc = 0; dc < 2; ++dc) {
        const int rr = 2 * r + dr, cc = 2 * c + dc;
        if (rr < m && cc < m) {
          const float4 t = src[(int64_t)rr * m + cc];
          s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
          cnt += 1.f;
        }
      }
    dst[i] = make_float4(s.x / cnt, s.y / cnt, s.z / cnt, s.w / cnt);
  }
}

// thread per (image, face)
__global__ __launch_bounds__(256) void face_lod(const float* __restrict__ xy, const int64_t* __restrict__ faces, const float* __restrict__ vt,
                                                 const int64_t* __restrict__ ft, int64_t N, int64_t V, int64_t F, int64_t Vt, float R, float bias,
                                                 float top, float* __restrict__ lod) {
  const int64_t total = N * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / F, f = i - n * F;
    const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    const int64_t ta = ft[f * 3], tb = ft[f * 3 + 1], tc = ft[f * 3 + 2];
    float out = top;
    if (sr_face_ok(a, b, c, V) && sr_face_ok(ta, tb, tc, Vt)) {
      const float2* P = (const float2*)xy + n * V;
      const float2* T = (const float2*)vt;
      const float2 p0 = P[a], p1 = P[b], p2 = P[c], t0 = T[ta], t1 = T[tb], t2 = T[tc];
      const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e2x = p2.x - p0.x, e2y = p2.y - p0.y;
      const float det = e1x * e2y - e1y * e2x;
      if (fabsf(det) >= 1e-12f) {
        const float u1 = t1.x - t0.x, v1 = t1.y - t0.y, u2 = t2.x - t0.x, v2 = t2.y - t0.y;
        const float dudx = (u1 * e2y - u2 * e1y) / det, dvdx = (v1 * e2y - v2 * e1y) / det;       // [uv1 uv2] [e1 e2]^-1
        const float dudy = (u2 * e1x - u1 * e2x) / det, dvdy = (v2 * e1x - v1 * e2x) / det;
        const float rho = R * fmaxf(sqrtf(dudx * dudx + dvdx * dvdx), sqrtf(dudy * dudy + dvdy * dvdy));
        out = fminf(fmaxf(log2f(rho) + bias, 0.f), top);
      }
    }
    lod[i] = out;
  }
}

struct ShadeColours { float bg[3], hole[3]; };

// bilinear sample of one n x n level at (u, v): x = u n - 0.5, y = (1 - v) n - 0.5, clamp to edge.  Clamping the sample point to
// [0, n - 1] first is the same function as clamping the four tap indices, and keeps every index in range whatever uv holds (NaN -> 0).
__device__ __forceinline__ float4 sample_level(const float4* __restrict__ lvl, int32_t n, float u, float v) {
  const float hi = (float)(n - 1);
  const float x = fminf(fmaxf(u * (float)n - 0.5f, 0.f), hi), y = fminf(fmaxf((1.f - v) * (float)n - 0.5f, 0.f), hi);
  const int x0 = (int)x, y0 = (int)y;                                  // x, y >= 0: truncation is floor
  const int x1 = min(x0 + 1, n - 1), y1 = min(y0 + 1, n - 1);
  const float fx = x - (float)x0, fy = y - (float)y0;
  const float4 a = lvl[(int64_t)y0 * n + x0], b = lvl[(int64_t)y0 * n + x1], c = lvl[(int64_t)y1 * n + x0], d = lvl[(int64_t)y1 * n + x1];
  const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy), w10 = (1.f - fx) * fy, w11 = fx * fy;
  return make_float4(w00 * a.x + w01 * b.x + w10 * c.x + w11 * d.x, w00 * a.y + w01 * b.y + w10 * c.y + w11 * d.y,
                     w00 * a.z + w01 * b.z + w10 * c.z + w11 * d.z, w00 * a.w + w01 * b.w + w10 * c.w + w11 * d.w);
}

// thread per pixel; one 16-byte store of (r, g, b, alpha)
__global__ __launch_bounds__(256) void shade_textured(const int64_t* __restrict__ pix_to_face, const float* __restrict__ bary, int64_t N, int64_t F,
                                                       int64_t HW, const int64_t* __restrict__ ft, const float* __restrict__ vt, int64_t Vt,
                                                       const float4* __restrict__ mips, MipLayout lay, const float* __restrict__ lod,
                                                       ShadeColours col, const float* __restrict__ bg_image, float4* __restrict__ rgba,
                                                       float* __restrict__ coverage) {
  __shared__ int32_t s_side[MIP_MAX_LEVELS];
  __shared__ int64_t s_off[MIP_MAX_LEVELS];
  if (threadIdx.x == 0)
    for (int l = 0; l < MIP_MAX_LEVELS; ++l) { s_side[l] = lay.side[l]; s_off[l] = lay.off[l]; }
  __syncthreads();
  const float top = (float)(lay.L - 1);
  const int64_t total = N * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = pix_to_face[i];
    float4 o = bg_image ? make_float4(bg_image[i * 3], bg_image[i * 3 + 1], bg_image[i * 3 + 2], 0.f) : make_float4(col.bg[0], col.bg[1], col.bg[2], 0.f);
    float cov = 0.f;
    if (p >= 0 && p < N * F) {
      const int64_t f = p % F;
      const int64_t ta = ft[f * 3], tb = ft[f * 3 + 1], tc = ft[f * 3 + 2];
      if (sr_face_ok(ta, tb, tc, Vt)) {
        const float b0 = bary[i * 3], b1 = bary[i * 3 + 1], b2 = bary[i * 3 + 2];
        const float2* T = (const float2*)vt;
        const float2 t0 = T[ta], t1 = T[tb], t2 = T[tc];
        const float u = b0 * t0.x + b1 * t1.x + b2 * t2.x, v = b0 * t0.y + b1 * t1.y + b2 * t2.y;
        const float l = fminf(fmaxf(lod[p], 0.f), top);                 // (already clamped by face_lod; NaN -> 0)
        const int l0 = (int)l, l1 = min(l0 + 1, lay.L - 1);
        const float t = l - (float)l0;
        const float4 s0 = sample_level(mips + s_off[l0], s_side[l0], u, v), s1 = sample_level(mips + s_off[l1], s_side[l1], u, v);
        const float px = (1.f - t) * s0.x + t * s1.x, py = (1.f - t) * s0.y + t * s1.y, pz = (1.f - t) * s0.z + t * s1.z;
        cov = (1.f - t) * s0.w + t * s1.w;
        o = cov > 0.f ? make_float4(px / cov, py / cov, pz / cov, 1.f) : make_float4(col.hole[0], col.hole[1], col.hole[2], 1.f);
      }
    }
    rgba[i] = o;
    if (coverage) coverage[i] = cov;
  }
}
}  // namespace

extern "C" int sr_texture_mips(const void* texture, int32_t is_u8, const uint8_t* valid, int32_t R, float* mips, void* stream) {
  if (!texture || !mips || R <= 0 || R > 32768 || ((uintptr_t)mips & 15)) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const MipLayout lay = mip_layout(R);
  float4* out = (float4*)mips;
  const int64_t total = (int64_t)R * R;
  if (is_u8)
    sr_launch_stream(mips_first<uint8_t>, total, 256, st, (const uint8_t*)texture, valid, total, out);
  else
    sr_launch_stream(mips_first<float>, total, 256, st, (const float*)texture, valid, total, out);
  for (int l = 1; l < lay.L; ++l)
    sr_launch_stream(mips_next, (int64_t)lay.side[l] * lay.side[l], 256, st, (const float4*)(out + lay.off[l - 1]), lay.side[l - 1], lay.side[l],
                     out + lay.off[l]);
  return sr_launch_status();
}

extern "C" int sr_texture_face_lod(const float* xy_pix, const int64_t* faces, const float* vt, const int64_t* ft, int64_t N, int64_t V, int64_t F,
                                   int64_t Vt, int32_t R, float bias, int32_t L, float* lod, void* stream) {
  if (!xy_pix || !faces || !vt || !ft || !lod || N <= 0 || V <= 0 || F <= 0 || Vt <= 0 || R <= 0 || R > 32768 || L != mip_layout(R).L ||
      ((uintptr_t)xy_pix & 7) || ((uintptr_t)vt & 7))
    return SR_EINVAL;
  sr_launch_stream(face_lod, N * F, 256, stream, xy_pix, faces, vt, ft, N, V, F, Vt, (float)R, bias, (float)(L - 1), lod);
  return sr_launch_status();
}

extern "C" int sr_shade_textured(const int64_t* pix_to_face, const float* bary, int64_t N, int64_t F, int32_t H, int32_t W, const int64_t* ft,
                                 const float* vt, int64_t Vt, const float* mips, int32_t R, int32_t L, const float* lod, const float* host_background,
                                 const float* host_hole, const float* bg_image, float* rgba, float* coverage, void* stream) {
  if (!pix_to_face || !bary || !ft || !vt || !mips || !lod || !host_background || !host_hole || !rgba || N <= 0 || F <= 0 || H <= 0 || W <= 0 ||
      Vt <= 0 || R <= 0 || R > 32768 || L != mip_layout(R).L || ((uintptr_t)rgba & 15) || ((uintptr_t)mips & 15) || ((uintptr_t)vt & 7))
    return SR_EINVAL;
  ShadeColours col;
  for (int k = 0; k < 3; ++k) { col.bg[k] = host_background[k]; col.hole[k] = host_hole[k]; }
  const int64_t HW = (int64_t)H * W;
  sr_launch_stream(shade_textured, N * HW, 256, stream, pix_to_face, bary, N, F, HW, ft, vt, Vt, (const float4*)mips, mip_layout(R), lod, col, bg_image,
                   (float4*)rgba, coverage);
  return sr_launch_status();
}
