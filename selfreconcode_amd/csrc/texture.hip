// Texture baking: UV-space multi-view aggregation for a UV-mapped template -- the GPU form of the reference's
// texture_mesh_prepare.py + texture_mesh_extract.py.  The reference leaves the UV unwrap and the per-view partial textures to opendr and
// VideoAvatar's Isomapper (third-party code that is not in the reference repository); what they compute is restated here from the
// script's use of them (restated, unpinned):
//
//  * sr_uv_rasterize: texel -> (UV face, UV barycentrics), once per template.  A wavefront per face walks the face's texel bounding box
//    and claims the texels whose centre it contains with an integer atomicMin on the face index (lowest index wins: identical bits
//    call to call); a second pass over the texels writes the barycentrics of the winner.  Edge functions in double: it runs once.
//  * sr_face_visibility / sr_view_alpha: per view, the faces that own a pixel of the rasterisation and have their three vertices in the
//    mask, and the per-vertex cosine between the viewing ray and the inward normal.
//  * sr_texture_accumulate: thread per covered texel, any number of views in frame order inside the thread.  The agg_num best-seen
//    candidates of a texel live slot-major ([agg_num][T]) in HBM, so a wavefront's accesses to one slot coalesce; the per-texel fill
//    count and the running minimum stay in registers over the views of a launch.
//  * sr_texture_resolve: count / mask_final / best view / per-channel median (rank counting over the filled slots).
//  * sr_texture_fill: push-pull fill of the unseen texels around the atlas (NOT cv2's Telea inpainting: see DESIGN.md 3.10).
//
// All of it is gather / stream work bound by HBM and L2: no LDS tiling, no MFMA.  No float atomics, and "empty" is the view id -1, never
// a NaN.
#include "sr_common.h"
#include "mesh_device.h"
#include "uv_device.h"

namespace {

constexpr int32_t UV_NONE = 0x7f7f7f7f;        // what hipMemsetAsync(0x7f) leaves: larger than every face index

// wavefront per face: lanes stride over the face's texel bounding box (one texel wider than the exact box; the inside test decides)
__global__ __launch_bounds__(256) void uv_claim(const float* __restrict__ vt, const int64_t* __restrict__ ft, int64_t Vt, int64_t F, int32_t R,
                                                 int32_t* __restrict__ face) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / SR_WAVE, nwaves = (int64_t)gridDim.x * blockDim.x / SR_WAVE;
  for (int64_t f = wave; f < F; f += nwaves) {
    const UvTri t = uv_tri(vt, ft, Vt, f);
    if (!t.ok) continue;
    const double umin = fmin(t.ax, fmin(t.bx, t.cx)), umax = fmax(t.ax, fmax(t.bx, t.cx));
    const double vmin = fmin(t.ay, fmin(t.by, t.cy)), vmax = fmax(t.ay, fmax(t.by, t.cy));
    if (!(umax >= 0. && umin <= 1. && vmax >= 0. && vmin <= 1.)) continue;
    const int c0 = clampi((int)floor(fmax(umin, 0.) * R - 0.5) - 1, 0, R - 1), c1 = clampi((int)ceil(fmin(umax, 1.) * R - 0.5) + 1, 0, R - 1);
    const int r0 = clampi((int)floor((1. - fmin(vmax, 1.)) * R - 0.5) - 1, 0, R - 1), r1 = clampi((int)ceil((1. - fmax(vmin, 0.)) * R - 0.5) + 1, 0, R - 1);
    const int bw = c1 - c0 + 1;
    const int64_t n = (int64_t)bw * (r1 - r0 + 1);
    const double s = t.area2 > 0. ? 1. : -1.;
    for (int64_t i = lane; i < n; i += SR_WAVE) {
      const int r = r0 + (int)(i / bw), c = c0 + (int)(i % bw);
      const double u = (c + 0.5) / R, v = 1. - (r + 0.5) / R;
      double e0, e1, e2;
      uv_edges(t, u, v, e0, e1, e2);
      if (s * e0 >= 0. && s * e1 >= 0. && s * e2 >= 0.) atomicMin(face + (int64_t)r * R + c, (int32_t)f);
    }
  }
}

__global__ __launch_bounds__(256) void uv_finish(const float* __restrict__ vt, const int64_t* __restrict__ ft, int64_t Vt, int64_t F, int32_t R,
                                                  int32_t* __restrict__ face, float* __restrict__ bary) {
  const int64_t total = (int64_t)R * R;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t f = face[i];
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    if (f >= 0 && f < F) {
      const UvTri t = uv_tri(vt, ft, Vt, f);
      const int r = (int)(i / R), c = (int)(i % R);
      double e0, e1, e2;
      uv_edges(t, (c + 0.5) / R, 1. - (r + 0.5) / R, e0, e1, e2);
      b0 = (float)(e0 / t.area2); b1 = (float)(e1 / t.area2); b2 = (float)(e2 / t.area2);
    } else {
      face[i] = -1;
    }
    bary[i * 3] = b0; bary[i * 3 + 1] = b1; bary[i * 3 + 2] = b2;
  }
}

// visible[p] = 1 for every packed face index p = view * F + face that owns a pixel (plain byte stores of the same value: benign)
__global__ __launch_bounds__(256) void vis_mark(const int64_t* __restrict__ pix_to_face, int64_t npix, int64_t NF, uint8_t* __restrict__ visible) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = pix_to_face[i];
    if (p >= 0 && p < NF) visible[p] = 1;
  }
}

// round-half-even of the pixel position (numpy's round), inside the viewport, and the mask set there
__device__ __forceinline__ bool vertex_in_mask(const float* __restrict__ xy, const uint8_t* __restrict__ mask, int32_t H, int32_t W) {
  const float rx = rintf(xy[0]), ry = rintf(xy[1]);
  if (!(rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H)) return false;       // (NaN fails too)
  return mask[(int64_t)ry * W + (int64_t)rx] != 0;
}

__global__ __launch_bounds__(256) void vis_finish(const int64_t* __restrict__ faces, int64_t N, int64_t V, int64_t F, const float* __restrict__ xy,
                                                   const uint8_t* __restrict__ mask, int32_t H, int32_t W, uint8_t* __restrict__ visible) {
  const int64_t total = N * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (!visible[i]) continue;
    const int64_t n = i / F, f = i - n * F;
    const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    bool ok = sr_face_ok(a, b, c, V);
    if (ok) {
      const float* P = xy + n * V * 2;
      const uint8_t* M = mask + n * (int64_t)H * W;
      ok = vertex_in_mask(P + a * 2, M, H, W) && vertex_in_mask(P + b * 2, M, H, W) && vertex_in_mask(P + c * 2, M, H, W);
    }
    visible[i] = ok ? 1 : 0;
  }
}

// alpha[n, v] = max(0, dot(normalize(p - cam), -normal))
__global__ __launch_bounds__(256) void view_alpha(const float* __restrict__ verts, const float* __restrict__ normals, const float* __restrict__ cam,
                                                   int64_t N, int64_t V, float* __restrict__ alpha) {
  const int64_t total = N * V;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / V;
    const float dx = verts[i * 3] - cam[n * 3], dy = verts[i * 3 + 1] - cam[n * 3 + 1], dz = verts[i * 3 + 2] - cam[n * 3 + 2];
    const float d = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-20f);
    const float a = -(dx * normals[i * 3] + dy * normals[i * 3 + 1] + dz * normals[i * 3 + 2]) / d;
    alpha[i] = a > 0.f ? a : 0.f;                                                        // (a NaN normal gives 0)
  }
}

// first slot holding the minimum of slot_cos[0 .. A) of texel t
__device__ __forceinline__ void slot_min(const float* slot_cos, int64_t T, int64_t t, int32_t A, float& mc, int32_t& mi) {
  mc = slot_cos[t]; mi = 0;
  for (int32_t j = 1; j < A; ++j) {
    const float v = slot_cos[(int64_t)j * T + t];
    if (v < mc) { mc = v; mi = j; }
  }
}

// thread per covered texel; the views of the launch in order.  While a texel has empty slots (count < A) the minimum is cosv0 and the first
// slot holding it is slot `count` (every accepted cosine is > cosv0 and slots fill front to back), so the slots are scanned only once they
// are full, and then only after a replacement.
__global__ __launch_bounds__(256) void tex_accumulate(int64_t T, const int32_t* __restrict__ tface, const float* __restrict__ tbary,
                                                       const int64_t* __restrict__ faces, int64_t F, int64_t V, int32_t N,
                                                       const uint8_t* __restrict__ visible, const float* __restrict__ alpha, const float* __restrict__ xy,
                                                       const float* __restrict__ images, int32_t H, int32_t W, const int32_t* __restrict__ fids, int32_t A,
                                                       float cosv0, float* slot_cos, float* __restrict__ slot_rgb, int32_t* __restrict__ slot_view,
                                                       int32_t* __restrict__ count, float* __restrict__ min_cos, int32_t* __restrict__ min_idx) {
  const float xmax = (float)(W - 1), ymax = (float)(H - 1);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = tface[t];
    if (f < 0 || f >= F) continue;
    const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (!sr_face_ok(a, b, c, V)) continue;
    const float b0 = tbary[t * 3], b1 = tbary[t * 3 + 1], b2 = tbary[t * 3 + 2];
    int32_t n = count[t], mi = min_idx[t];
    float mc = min_cos[t];
    n = n < 0 ? 0 : (n > A ? A : n);
    if (n == A && (mi < 0 || mi >= A)) slot_min(slot_cos, T, t, A, mc, mi);            // (a state this kernel did not write)
    for (int32_t k = 0; k < N; ++k) {
      if (!visible[(int64_t)k * F + f]) continue;
      const float* al = alpha + (int64_t)k * V;
      const float cosv = b0 * al[a] + b1 * al[b] + b2 * al[c];
      const float cur = n < A ? cosv0 : mc;
      if (!(cosv > cur)) continue;
      const int32_t slot = n < A ? n : mi;
      const float* P = xy + (int64_t)k * V * 2;
      float px = b0 * P[a * 2] + b1 * P[b * 2] + b2 * P[c * 2];
      float py = b0 * P[a * 2 + 1] + b1 * P[b * 2 + 1] + b2 * P[c * 2 + 1];
      px = fminf(fmaxf(px, 0.f), xmax); py = fminf(fmaxf(py, 0.f), ymax);              // clamped to the image (NaN -> 0)
      const int x0 = (int)floorf(px), y0 = (int)floorf(py);
      const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
      const float wx = px - (float)x0, wy = py - (float)y0;
      const float* I = images + (int64_t)k * H * W * 3;
      const float* q00 = I + ((int64_t)y0 * W + x0) * 3; const float* q01 = I + ((int64_t)y0 * W + x1) * 3;
      const float* q10 = I + ((int64_t)y1 * W + x0) * 3; const float* q11 = I + ((int64_t)y1 * W + x1) * 3;
      const int64_t o = (int64_t)slot * T + t;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float top = q00[ch] + wx * (q01[ch] - q00[ch]), bot = q10[ch] + wx * (q11[ch] - q10[ch]);
        slot_rgb[((int64_t)slot * 3 + ch) * T + t] = top + wy * (bot - top);
      }
      slot_cos[o] = cosv;
      slot_view[o] = fids[k];
      if (n < A) ++n;
      if (n == A) slot_min(slot_cos, T, t, A, mc, mi);
    }
    count[t] = n; min_cos[t] = mc; min_idx[t] = mi;
  }
}

constexpr int RANK_CHUNK = 8;

// thread per covered texel.  The filled slots of a texel are its first `count` slots (sr_texture_accumulate fills front to back and never
// empties one).  Median of channel ch: the values of rank (n - 1) / 2 and n / 2 in the order (value, slot), found by counting, eight
// candidates at a time held in registers against one pass over the slots.
__global__ __launch_bounds__(256) void tex_resolve(int64_t T, const int32_t* __restrict__ texel, int32_t A, float cosv0, int32_t check_num,
                                                    const float* __restrict__ slot_cos, const float* __restrict__ slot_rgb,
                                                    const int32_t* __restrict__ slot_view, int32_t* __restrict__ count, uint8_t* __restrict__ mask_final,
                                                    int32_t* __restrict__ view_id, float* __restrict__ median) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = texel[t];
    int32_t n = 0, best = 0;
    float bestc = slot_cos[t];
    for (int32_t j = 0; j < A; ++j) {
      const float c = slot_cos[(int64_t)j * T + t];
      n += c > cosv0 ? 1 : 0;
      if (c > bestc) { bestc = c; best = j; }                                           // first slot with the maximum
    }
    const bool fin = n >= check_num;
    count[o] = n;
    mask_final[o] = fin ? 1 : 0;
    view_id[o] = fin ? slot_view[(int64_t)best * T + t] : -1;
    float med[3] = {0.f, 0.f, 0.f};
    if (fin) {
      const int32_t lo = (n - 1) / 2, hi = n / 2;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float mlo = 0.f, mhi = 0.f;
        for (int32_t i0 = 0; i0 < n; i0 += RANK_CHUNK) {
          float x[RANK_CHUNK];
          int32_t rank[RANK_CHUNK];
#pragma unroll
          for (int q = 0; q < RANK_CHUNK; ++q) {
            const int32_t i = i0 + q < n ? i0 + q : n - 1;
            x[q] = slot_rgb[((int64_t)i * 3 + ch) * T + t];
            rank[q] = 0;
          }
          for (int32_t j = 0; j < n; ++j) {
            const float y = slot_rgb[((int64_t)j * 3 + ch) * T + t];
#pragma unroll
            for (int q = 0; q < RANK_CHUNK; ++q) rank[q] += (y < x[q] || (y == x[q] && j < i0 + q)) ? 1 : 0;
          }
#pragma unroll
          for (int q = 0; q < RANK_CHUNK; ++q) {
            if (i0 + q < n && rank[q] == lo) mlo = x[q];
            if (i0 + q < n && rank[q] == hi) mhi = x[q];
          }
        }
        med[ch] = 0.5f * (mlo + mhi);
      }
    }
    median[o * 3] = med[0]; median[o * 3 + 1] = med[1]; median[o * 3 + 2] = med[2];
  }
}

// ---------------------------------------------------------------------------------------------- fill (push-pull)
// square dilation by k (window i - k / 2 .. i - k / 2 + k - 1 on both axes, cv2.dilate's anchor), as a row pass and a column pass
__global__ __launch_bounds__(256) void dilate_axis(const uint8_t* __restrict__ src, int32_t R, int32_t k, int32_t along_rows, uint8_t* __restrict__ dst) {
  const int64_t total = (int64_t)R * R;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / R), c = (int)(i % R);
    const int p = along_rows ? r : c;
    int lo = p - k / 2, hi = lo + k - 1;
    if (k <= 0) { lo = p; hi = p; }
    lo = lo < 0 ? 0 : lo; hi = hi > R - 1 ? R - 1 : hi;
    uint8_t m = 0;
    for (int j = lo; j <= hi && !m; ++j) m = src[along_rows ? (int64_t)j * R + c : (int64_t)r * R + j] != 0;
    dst[i] = m;
  }
}

// level 1 from the texture: a coarse cell is the mean of its known (mask_final) children; .w = 1 when it has one
__global__ __launch_bounds__(256) void push_first(const float* __restrict__ tex, const uint8_t* __restrict__ known, int32_t R, int32_t n,
                                                   float4* __restrict__ out) {
  const int64_t total = (int64_t)n * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / n), c = (int)(i % n);
    float sx = 0.f, sy = 0.f, sz = 0.f, w = 0.f;
    for (int dr = 0; dr < 2; ++dr)
      for (int dc = 0; dc < 2; ++dc) {
        const int rr = 2 * r + dr, cc = 2 * c + dc;
        if (rr < R && cc < R && known[(int64_t)rr * R + cc]) {
          const float* p = tex + ((int64_t)rr * R + cc) * 3;
          sx += p[0]; sy += p[1]; sz += p[2]; w += 1.f;
        }
      }
    out[i] = w > 0.f ? make_float4(sx / w, sy / w, sz / w, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__global__ __launch_bounds__(256) void push_level(const float4* __restrict__ fine, int32_t nf, int32_t n, float4* __restrict__ out) {
  const int64_t total = (int64_t)n * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / n), c = (int)(i % n);
    float sx = 0.f, sy = 0.f, sz = 0.f, w = 0.f;
    for (int dr = 0; dr < 2; ++dr)
      for (int dc = 0; dc < 2; ++dc) {
        const int rr = 2 * r + dr, cc = 2 * c + dc;
        if (rr < nf && cc < nf) {
          const float4 p = fine[(int64_t)rr * nf + cc];
          if (p.w > 0.f) { sx += p.x; sy += p.y; sz += p.z; w += 1.f; }
        }
      }
    out[i] = w > 0.f ? make_float4(sx / w, sy / w, sz / w, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// bilinear sample of the (fully known) coarse level at the centre of fine cell (r, c): weights 9/16, 3/16, 3/16, 1/16, neighbours clamped
__device__ __forceinline__ float4 pull_sample(const float4* __restrict__ coarse, int32_t nc, int r, int c) {
  const int pr = r >> 1, pc = c >> 1;
  const int qr = clampi(pr + ((r & 1) ? 1 : -1), 0, nc - 1), qc = clampi(pc + ((c & 1) ? 1 : -1), 0, nc - 1);
  const float4 a = coarse[(int64_t)pr * nc + pc], b = coarse[(int64_t)pr * nc + qc], d = coarse[(int64_t)qr * nc + pc], e = coarse[(int64_t)qr * nc + qc];
  return make_float4(0.5625f * a.x + 0.1875f * b.x + 0.1875f * d.x + 0.0625f * e.x, 0.5625f * a.y + 0.1875f * b.y + 0.1875f * d.y + 0.0625f * e.y,
                     0.5625f * a.z + 0.1875f * b.z + 0.1875f * d.z + 0.0625f * e.z, 1.f);
}

// unknown cells of `fine` take the coarse level's value
__global__ __launch_bounds__(256) void pull_level(const float4* __restrict__ coarse, int32_t nc, float4* __restrict__ fine, int32_t nf) {
  const int64_t total = (int64_t)nf * nf;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (fine[i].w > 0.f) continue;
    fine[i] = pull_sample(coarse, nc, (int)(i / nf), (int)(i % nf));
  }
}

// the texture: mask_final texels copied bit for bit, region texels pulled from level 1, everything else 0
__global__ __launch_bounds__(256) void pull_final(const float* __restrict__ tex, const uint8_t* __restrict__ known, const uint8_t* __restrict__ region,
                                                   const float4* __restrict__ coarse, int32_t nc, int32_t R, float* __restrict__ out) {
  const int64_t total = (int64_t)R * R;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float x = 0.f, y = 0.f, z = 0.f;
    if (known[i]) {
      x = tex[i * 3]; y = tex[i * 3 + 1]; z = tex[i * 3 + 2];
    } else if (region[i]) {                             // (nothing known anywhere: every level is 0)
      const float4 p = pull_sample(coarse, nc, (int)(i / R), (int)(i % R));
      x = p.x; y = p.y; z = p.z;
    }
    out[i * 3] = x; out[i * 3 + 1] = y; out[i * 3 + 2] = z;
  }
}

constexpr int FILL_MAX_LEVELS = 32;

// sizes of levels 1 .. L (halved, rounded up, down to 1 x 1); returns L
int fill_levels(int32_t R, int32_t* n) {
  int L = 0;
  int32_t s = R;
  while (s > 1 && L < FILL_MAX_LEVELS) { s = (s + 1) / 2; n[L++] = s; }
  if (L == 0) n[L++] = 1;                            // R = 1: one level of one cell
  return L;
}
}  // namespace

extern "C" int sr_uv_rasterize(const float* vt, const int64_t* ft, int64_t Vt, int64_t F, int32_t R, int32_t* face, float* bary, void* stream) {
  if (!vt || !ft || !face || !bary || Vt <= 0 || F <= 0 || F >= UV_NONE || R <= 0 || R > 32768) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t texels = (int64_t)R * R;
  if (hipMemsetAsync(face, 0x7f, (size_t)texels * 4, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(uv_claim, F * SR_WAVE, 256, st, vt, ft, Vt, F, R, face);
  sr_launch_stream(uv_finish, texels, 256, st, vt, ft, Vt, F, R, face, bary);
  return sr_launch_status();
}

extern "C" int sr_face_visibility(const int64_t* pix_to_face, const int64_t* faces, int64_t N, int64_t V, int64_t F, const float* xy_pix,
                                  const uint8_t* mask, int32_t H, int32_t W, uint8_t* visible, void* stream) {
  if (!pix_to_face || !faces || !xy_pix || !mask || !visible || N <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(visible, 0, (size_t)(N * F), st) != hipSuccess) return SR_ELAUNCH;
  const int64_t npix = N * (int64_t)H * W;
  sr_launch_stream(vis_mark, npix, 256, st, pix_to_face, npix, N * F, visible);
  sr_launch_stream(vis_finish, N * F, 256, st, faces, N, V, F, xy_pix, mask, H, W, visible);
  return sr_launch_status();
}

extern "C" int sr_view_alpha(const float* verts, const float* normals, const float* cam_pos, int64_t N, int64_t V, float* alpha, void* stream) {
  if (!verts || !normals || !cam_pos || !alpha || N <= 0 || V <= 0) return SR_EINVAL;
  sr_launch_stream(view_alpha, N * V, 256, stream, verts, normals, cam_pos, N, V, alpha);
  return sr_launch_status();
}

extern "C" int sr_texture_accumulate(int64_t T, const int32_t* tface, const float* tbary, const int64_t* faces, int64_t F, int64_t V, int32_t N,
                                     const uint8_t* visible, const float* alpha, const float* xy_pix, const float* images, int32_t H, int32_t W,
                                     const int32_t* fids, int32_t agg_num, float cosv0, float* slot_cos, float* slot_rgb, int32_t* slot_view,
                                     int32_t* count, float* min_cos, int32_t* min_idx, void* stream) {
  if (!tface || !tbary || !faces || !visible || !alpha || !xy_pix || !images || !fids || !slot_cos || !slot_rgb || !slot_view || !count || !min_cos ||
      !min_idx || T <= 0 || F <= 0 || V <= 0 || N <= 0 || H <= 0 || W <= 0 || agg_num <= 0 || !(cosv0 >= 0.f))
    return SR_EINVAL;
  sr_launch_stream(tex_accumulate, T, 256, stream, T, tface, tbary, faces, F, V, N, visible, alpha, xy_pix, images, H, W, fids, agg_num, cosv0, slot_cos,
                   slot_rgb, slot_view, count, min_cos, min_idx);
  return sr_launch_status();
}

extern "C" int sr_texture_resolve(int64_t T, const int32_t* texel, int32_t agg_num, float cosv0, int32_t check_num, const float* slot_cos,
                                  const float* slot_rgb, const int32_t* slot_view, int32_t* count, uint8_t* mask_final, int32_t* view_id,
                                  float* tex_median, void* stream) {
  if (!texel || !slot_cos || !slot_rgb || !slot_view || !count || !mask_final || !view_id || !tex_median || T <= 0 || agg_num <= 0 || check_num <= 0)
    return SR_EINVAL;
  sr_launch_stream(tex_resolve, T, 256, stream, T, texel, agg_num, cosv0, check_num, slot_cos, slot_rgb, slot_view, count, mask_final, view_id, tex_median);
  return sr_launch_status();
}

extern "C" int64_t sr_texture_fill_workspace_bytes(int32_t R) {
  if (R <= 0 || R > 32768) return -1;
  int32_t n[FILL_MAX_LEVELS];
  const int L = fill_levels(R, n);
  int64_t cells = 0;
  for (int l = 0; l < L; ++l) cells += (int64_t)n[l] * n[l];
  return cells * 16 + 2 * (int64_t)R * R;
}

extern "C" int sr_texture_fill(const float* tex_median, const uint8_t* mask_final, const uint8_t* tex_mask, int32_t R, int32_t dilate,
                               float* texture, void* workspace, void* stream) {
  if (!tex_median || !mask_final || !tex_mask || !texture || !workspace || R <= 0 || R > 32768 || dilate < 0 || ((uintptr_t)workspace & 15))
    return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int32_t n[FILL_MAX_LEVELS];
  const int L = fill_levels(R, n);
  float4* level[FILL_MAX_LEVELS];
  float4* p = (float4*)workspace;
  for (int l = 0; l < L; ++l) { level[l] = p; p += (int64_t)n[l] * n[l]; }
  uint8_t* rows = (uint8_t*)p;
  uint8_t* region = rows + (int64_t)R * R;
  const int64_t texels = (int64_t)R * R;
  const int g = sr_stream_grid(texels, 256);
  hipLaunchKernelGGL(dilate_axis, dim3(g), dim3(256), 0, st, tex_mask, R, dilate, 1, rows);
  hipLaunchKernelGGL(dilate_axis, dim3(g), dim3(256), 0, st, (const uint8_t*)rows, R, dilate, 0, region);
  sr_launch_stream(push_first, (int64_t)n[0] * n[0], 256, st, tex_median, mask_final, R, n[0], level[0]);
  for (int l = 1; l < L; ++l)
    sr_launch_stream(push_level, (int64_t)n[l] * n[l], 256, st, (const float4*)level[l - 1], n[l - 1], n[l], level[l]);
  for (int l = L - 2; l >= 0; --l)
    sr_launch_stream(pull_level, (int64_t)n[l] * n[l], 256, st, (const float4*)level[l + 1], n[l + 1], level[l], n[l]);
  hipLaunchKernelGGL(pull_final, dim3(g), dim3(256), 0, st, tex_median, mask_final, (const uint8_t*)region, (const float4*)level[0], n[0], R, texture);
  return sr_launch_status();
}
