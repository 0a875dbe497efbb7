// Template preparation for the texture stage: vertex-clustering simplification and a box-projection chart unwrap of the marching-cubes
// template, plus the contested-texel count of an atlas (semantics stated there, unpinned -- the reference leaves this
// step to MeshLab / Blender).  Sorting, unique and compaction are torch's; everything per element is here.
//
//  * simplify: sr_meshprep_bounds (box of the vertices by min / max atomics on ordered integers, and a non-finite flag),
//    sr_meshprep_cell_keys (grid cell of a vertex: float32 subtraction and IEEE float32 division), sr_meshprep_cell_mean (thread per
//    occupied cell, its members summed in ascending original index in double), sr_meshprep_face_keys (remapped corners, the sorted
//    triple as a two-part key, -1 for a collapsed face) and sr_meshprep_face_first (first of every run of equal keys after two stable
//    sorts = the lowest original index).
//  * quadric placement (optional): sr_meshprep_cell_faces (cell-face incidence as sortable slots), sr_meshprep_cell_quadric (16 lanes
//    per cell: the cell's summed plane quadrics, the regularised 3 x 3 solve about the cell mean, the clamp to the cell's box) and
//    sr_meshprep_face_flips (surviving faces whose normal turned over or vanished).
//  * unwrap: sr_chart_classify (dominant axis and sign of the float64 normal, every product and difference rounded on its own),
//    sr_chart_edge_keys (half-edge keys that carry the class, so equal keys = same edge and same class), sr_chart_hook / sr_chart_jump
//    (connected components by min-label hooking of roots and pointer doubling, both double-buffered: the number of passes is a function
//    of the input alone), sr_chart_bbox (per-chart box of the projected corners) and sr_chart_uv.
//  * sr_uv_overlap_count: texel centres strictly inside two or more UV triangles, with sr_uv_rasterize's texel convention.
//
// Stream / gather work bound by HBM and by atomics on a few addresses; no float atomics anywhere: sums are sequential per thread (the
// quadric sums: per lane, then a butterfly of fixed shape), the atomics are integer adds and min / max, so two calls give identical bits.
// Shared with mesh_collapse.hip and stated once elsewhere: which rows are faces, half-edge corners, the face remap, the pointer jump and
// the counter flush (mesh_device.h), the wave butterflies (sr_wave.h), the face normal and the plane quadric (quadric_device.h).
#include "sr_common.h"
#include "uv_device.h"
#include "mesh_device.h"
#include "quadric_device.h"

namespace {

// float <-> int32 with the same order (-0 counts as +0), for atomicMin / atomicMax
__device__ __forceinline__ int32_t ordered(float x) {
  const int32_t b = __float_as_int(x + 0.f);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float unordered(int32_t o) { return __int_as_float(o ^ ((o >> 31) & 0x7fffffff)); }

// ---------------------------------------------------------------------------------------------- simplify
__global__ void bounds_init(int32_t* __restrict__ box) {
  if (threadIdx.x < 3) box[threadIdx.x] = INT32_MAX;
  else if (threadIdx.x < 6) box[threadIdx.x] = INT32_MIN;
  else if (threadIdx.x < 8) box[threadIdx.x] = 0;
}

// box[0..3) = min, box[3..6) = max (ordered integers), box[6] = a coordinate is not finite
__global__ __launch_bounds__(256) void bounds_reduce(const float* __restrict__ verts, int64_t V, int32_t* __restrict__ box) {
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = verts[i * 3 + k];
      if (!isfinite(x)) { bad = 1; continue; }
      const int32_t o = ordered(x);
      lo[k] = min(lo[k], o); hi[k] = max(hi[k], o);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = sr_wave_min(lo[k]); hi[k] = sr_wave_max(hi[k]); }
  bad = sr_wave_max(bad);
  if ((threadIdx.x & (SR_WAVE - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { atomicMin(box + k, lo[k]); atomicMax(box + 3 + k, hi[k]); }
    if (bad) atomicOr(box + 6, 1);
  }
}

__global__ void bounds_finish(int32_t* __restrict__ box) {
  if (threadIdx.x < 6) box[threadIdx.x] = __float_as_int(unordered(box[threadIdx.x]));
}

__global__ __launch_bounds__(256) void cell_keys(const float* __restrict__ verts, int64_t V, const float* __restrict__ lo, float cell, int64_t nx,
                                                  int64_t ny, int64_t nz, int64_t* __restrict__ key) {
  const float lx = lo[0], ly = lo[1], lz = lo[2];
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    int64_t i = (int64_t)floorf(__fdiv_rn(__fsub_rn(verts[v * 3], lx), cell));
    int64_t j = (int64_t)floorf(__fdiv_rn(__fsub_rn(verts[v * 3 + 1], ly), cell));
    int64_t k = (int64_t)floorf(__fdiv_rn(__fsub_rn(verts[v * 3 + 2], lz), cell));
    i = i < 0 ? 0 : (i >= nx ? nx - 1 : i); j = j < 0 ? 0 : (j >= ny ? ny - 1 : j); k = k < 0 ? 0 : (k >= nz ? nz - 1 : k);   // (no-ops for the box's own vertices)
    key[v] = (k * ny + j) * nx + i;
  }
}

// thread per occupied cell: members order[offsets[c] .. offsets[c + 1]) are in ascending original index (a stable sort made them)
__global__ __launch_bounds__(256) void cell_mean(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ order,
                                                  const int64_t* __restrict__ offsets, int64_t C, float* __restrict__ out) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = offsets[c], e = offsets[c + 1];
    double x = 0., y = 0., z = 0.;
    int64_t n = 0;
    for (int64_t m = s; m < e; ++m) {
      const int64_t v = order[m];
      if (v < 0 || v >= V) continue;
      x += (double)verts[v * 3]; y += (double)verts[v * 3 + 1]; z += (double)verts[v * 3 + 2]; ++n;
    }
    const double d = n > 0 ? (double)n : 1.;
    out[c * 3] = (float)(x / d); out[c * 3 + 1] = (float)(y / d); out[c * 3 + 2] = (float)(z / d);
  }
}

__global__ __launch_bounds__(256) void face_keys(const int64_t* __restrict__ faces, int64_t F, const int64_t* __restrict__ vmap, int64_t V, int64_t Vn,
                                                  int64_t* __restrict__ out_faces, int64_t* __restrict__ key_hi, int64_t* __restrict__ key_lo) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    int64_t x, y, z;
    sr_face_remap(faces, f, vmap, V, x, y, z);
    out_faces[f * 3] = x; out_faces[f * 3 + 1] = y; out_faces[f * 3 + 2] = z;
    const bool dead = x < 0 || y < 0 || z < 0 || x >= Vn || y >= Vn || z >= Vn || x == y || y == z || x == z;
    const int64_t lo = min(x, min(y, z)), hi = max(x, max(y, z)), mid = x + y + z - lo - hi;
    key_hi[f] = dead ? -1 : lo * Vn + mid;
    key_lo[f] = dead ? -1 : hi;
  }
}

// position i of the faces sorted by (key_hi, key_lo), ties in original order: the first of a run of equal keys survives
__global__ __launch_bounds__(256) void face_first(const int64_t* __restrict__ key_hi, const int64_t* __restrict__ key_lo, const int64_t* __restrict__ perm,
                                                   int64_t F, uint8_t* __restrict__ keep) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < F; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = perm[i];
    if (p < 0 || p >= F) continue;
    keep[p] = key_hi[i] >= 0 && (i == 0 || key_hi[i] != key_hi[i - 1] || key_lo[i] != key_lo[i - 1]) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------- quadric placement
// slot[3 f + k] = the cell of corner k, or C (an empty slot) when an earlier corner of the face has that cell already or the row is not
// a face: sorted by cell (stable), every cell's list holds each face that touches it once, in ascending face index
__global__ __launch_bounds__(256) void cell_face_slots(const int64_t* __restrict__ faces, int64_t F, const int64_t* __restrict__ vmap, int64_t V, int64_t C,
                                                        int64_t* __restrict__ slot) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    int64_t x = C, y = C, z = C;
    if (sr_face_ok(a, b, c, V)) {
      x = vmap[a]; y = vmap[b]; z = vmap[c];
      if (x < 0 || x > C) x = C;
      if (y < 0 || y > C || y == x) y = C;
      if (z < 0 || z > C || z == x || z == y) z = C;
    }
    slot[f * 3] = x; slot[f * 3 + 1] = y; slot[f * 3 + 2] = z;
  }
}

#define SR_QUADRIC_LANES 16                            // lanes per cell: part of the stated order of the sums, not a tuning knob

__device__ __forceinline__ double group_sum(double v) { return sr_wave_sum<double, SR_QUADRIC_LANES>(v); }

// 16 lanes per occupied cell.  Lane l sums the plane quadrics of entries l, l + 16, ... of the cell's face list in that order, the 16
// partial sums meet in a butterfly of fixed shape, and every lane then holds A (6 numbers) and b (3).  The mean is summed by every
// lane on its own in cell_mean's order (the loads are broadcasts), the 3 x 3 system is solved by Cholesky, lane 0 stores.  The order of
// every sum depends on the lists alone, not on the grid.
__global__ __launch_bounds__(256) void cell_quadric(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                                                     const int64_t* __restrict__ face_slots, const int64_t* __restrict__ face_offsets,
                                                     const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                     const int64_t* __restrict__ cells, int64_t C, const float* __restrict__ lo, float cell, int64_t nx,
                                                     int64_t ny, double reg, float* __restrict__ out, int32_t* __restrict__ flags,
                                                     float* __restrict__ shift) {
  const int lane = threadIdx.x & (SR_QUADRIC_LANES - 1);
  const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / SR_QUADRIC_LANES;
  const int64_t groups = (int64_t)gridDim.x * blockDim.x / SR_QUADRIC_LANES;
  const double l0[3] = {(double)lo[0], (double)lo[1], (double)lo[2]}, h = (double)cell;
  for (int64_t c = group; c < C; c += groups) {
    double xx = 0., xy = 0., xz = 0., yy = 0., yz = 0., zz = 0., bx = 0., by = 0., bz = 0.;
    const int64_t fs = max(face_offsets[c], (int64_t)0), fe = min(face_offsets[c + 1], 3 * F);
    for (int64_t e = fs + lane; e < fe; e += SR_QUADRIC_LANES) {
      const int64_t s = face_slots[e];
      if (s < 0 || s >= 3 * F) continue;
      const int64_t f = s / 3, i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
      if (!sr_face_ok(i0, i1, i2, V)) continue;
      PlaneQuadric p;
      if (!plane_quadric(verts + i0 * 3, verts + i1 * 3, verts + i2 * 3, p)) continue;
      xx += p.w0 * p.n0; xy += p.w0 * p.n1; xz += p.w0 * p.n2; yy += p.w1 * p.n1; yz += p.w1 * p.n2; zz += p.w2 * p.n2;
      bx += p.wd * p.n0; by += p.wd * p.n1; bz += p.wd * p.n2;
    }
    xx = group_sum(xx); xy = group_sum(xy); xz = group_sum(xz); yy = group_sum(yy); yz = group_sum(yz); zz = group_sum(zz);
    bx = group_sum(bx); by = group_sum(by); bz = group_sum(bz);

    double m[3] = {0., 0., 0.};
    int64_t n = 0;
    const int64_t ms = max(offsets[c], (int64_t)0), me = min(offsets[c + 1], V);
    for (int64_t k = ms; k < me; ++k) {
      const int64_t v = order[k];
      if (v < 0 || v >= V) continue;
      m[0] += (double)verts[v * 3]; m[1] += (double)verts[v * 3 + 1]; m[2] += (double)verts[v * 3 + 2]; ++n;
    }
    const double cnt = n > 0 ? (double)n : 1.;
    m[0] /= cnt; m[1] /= cnt; m[2] /= cnt;

    int32_t flag = 0;
    double x[3];
    if (!quadric_optimum(xx, xy, xz, yy, yz, zz, bx, by, bz, m, reg, x)) flag |= SR_QUADRIC_NO_PLANES;
    const int64_t key = cells[c];
    const int64_t ijk[3] = {key % nx, (key / nx) % ny, key / (nx * ny)};
    double s2 = 0.;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double wlo = l0[k] + (double)ijk[k] * h, whi = l0[k] + (double)(ijk[k] + 1) * h;
      if (x[k] < wlo) { x[k] = wlo; flag |= SR_QUADRIC_CLAMPED; }
      if (x[k] > whi) { x[k] = whi; flag |= SR_QUADRIC_CLAMPED; }
      s2 += (x[k] - m[k]) * (x[k] - m[k]);
    }
    if (lane == 0) {
      out[c * 3] = (float)x[0]; out[c * 3 + 1] = (float)x[1]; out[c * 3 + 2] = (float)x[2];
      flags[c] = flag;
      shift[c] = (float)(sqrt(s2) / h);
    }
  }
}

// per surviving face: the normal at the new positions against the normal of the face it comes from (both unnormalised, in double).
// counts[0] += the dot product is negative, counts[1] += the new normal is zero.
__global__ __launch_bounds__(256) void face_flips(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                                                   const float* __restrict__ new_verts, int64_t Vn, const int64_t* __restrict__ new_faces,
                                                   const int64_t* __restrict__ source, int64_t Fn, unsigned long long* __restrict__ counts) {
  int32_t flipped = 0, flat = 0;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < Fn; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = source[g];
    if (f < 0 || f >= F) continue;
    double N[2][3];
    bool ok = true;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const float* __restrict__ p = side ? new_verts : verts;
      const int64_t* __restrict__ t = side ? new_faces + g * 3 : faces + f * 3;
      const int64_t lim = side ? Vn : V, a = t[0], b = t[1], c = t[2];
      if (!sr_face_ok(a, b, c, lim)) { ok = false; break; }
      face_normal(p + a * 3, p + b * 3, p + c * 3, N[side]);
    }
    if (!ok) continue;
    if (N[1][0] == 0. && N[1][1] == 0. && N[1][2] == 0.) ++flat;
    else if (N[0][0] * N[1][0] + N[0][1] * N[1][1] + N[0][2] * N[1][2] < 0.) ++flipped;
  }
  sr_record_add(counts, flipped);
  sr_record_add(counts + 1, flat);
}

// ---------------------------------------------------------------------------------------------- unwrap
// class = 2 axis + (negative ? 1 : 0) of the unnormalised normal (b - a) x (c - a) in double, no contraction: the restatement rounds
// every product and every difference on its own and must agree on ties
__device__ int32_t face_class(const float* __restrict__ pa, const float* __restrict__ pb, const float* __restrict__ pc) {
  double n[3];
  face_normal(pa, pb, pc, n);
  int k = 0;
  if (fabs(n[1]) > fabs(n[k])) k = 1;
  if (fabs(n[2]) > fabs(n[k])) k = 2;                 // (strict: the lowest axis wins a tie, and a zero normal stays +x)
  return 2 * k + (n[k] < 0. ? 1 : 0);
}

__global__ __launch_bounds__(256) void chart_classify(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                                                       int32_t* __restrict__ cls) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    const bool ok = sr_face_ok(a, b, c, V);
    cls[f] = ok ? face_class(verts + a * 3, verts + b * 3, verts + c * 3) : 0;
  }
}

// half-edge h = 3 f + corner: (min V + max) 6 + class; -1 for an edge between a vertex and itself
__global__ __launch_bounds__(256) void chart_edge_keys(const int64_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ cls,
                                                        int64_t* __restrict__ key) {
  for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < 3 * F; h += (int64_t)gridDim.x * blockDim.x) {
    const SrHalfEdge e = sr_half_edge(faces, h);
    key[h] = sr_edge_ok(e.from, e.to, V) ? (min(e.from, e.to) * V + max(e.from, e.to)) * 6 + cls[h / 3] : -1;
  }
}

// neighbouring half-edges of the sorted list with one key join their faces: the larger of the two roots takes the smaller as parent
// (atomicMin: the least of all offers).  P is a forest of stars here, so P[face] is its root; Q starts as a copy of P.
__global__ __launch_bounds__(256) void chart_hook(const int64_t* __restrict__ skey, const int64_t* __restrict__ perm, int64_t n, const int32_t* __restrict__ P,
                                                   int32_t* __restrict__ Q, int64_t F, int32_t* __restrict__ changed) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (skey[i] < 0 || skey[i] != skey[i - 1]) continue;
    const int64_t a = perm[i - 1] / 3, b = perm[i] / 3;
    if (a < 0 || b < 0 || a >= F || b >= F) continue;
    const int32_t ra = P[a], rb = P[b];
    if (ra == rb || ra < 0 || rb < 0 || ra >= F || rb >= F) continue;
    atomicMin(Q + max(ra, rb), min(ra, rb));
    *changed = 1;
  }
}

__global__ __launch_bounds__(256) void chart_jump(const int32_t* __restrict__ P, int64_t F, int32_t* __restrict__ Q, int32_t* __restrict__ changed) {
  sr_forest_jump(P, F, Q, changed);
}

// (u, v) of a point under class `c`: the two axes after the dominant one, swapped for a negative sign
__device__ __forceinline__ void project(const float* __restrict__ p, int32_t c, float& u, float& v) {
  const int k = c >> 1;
  const float s = p[(k + 1) % 3], t = p[(k + 2) % 3];
  u = (c & 1) ? t : s; v = (c & 1) ? s : t;
}

__global__ __launch_bounds__(256) void box_init(int32_t* __restrict__ box, int64_t C) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 4 * C; i += (int64_t)gridDim.x * blockDim.x)
    box[i] = (i & 3) < 2 ? INT32_MAX : INT32_MIN;
}

__global__ __launch_bounds__(256) void chart_box(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                                                  const int32_t* __restrict__ cls, const int64_t* __restrict__ chart, int64_t C, int32_t* __restrict__ box) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = chart[f];
    if (c < 0 || c >= C) continue;
    int32_t u0 = INT32_MAX, v0 = INT32_MAX, u1 = INT32_MIN, v1 = INT32_MIN;
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      const int64_t a = faces[f * 3 + k];
      if (a < 0 || a >= V) { ok = false; break; }
      float u, v;
      project(verts + a * 3, cls[f], u, v);
      const int32_t ou = ordered(u), ov = ordered(v);
      u0 = min(u0, ou); u1 = max(u1, ou); v0 = min(v0, ov); v1 = max(v1, ov);
    }
    if (!ok) continue;
    atomicMin(box + c * 4, u0); atomicMin(box + c * 4 + 1, v0); atomicMax(box + c * 4 + 2, u1); atomicMax(box + c * 4 + 3, v1);
  }
}

__global__ __launch_bounds__(256) void box_finish(const int32_t* __restrict__ box, int64_t C, float* __restrict__ bbox_min, float* __restrict__ extent) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * C; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i >> 1, k = i & 1;
    const int32_t lo = box[c * 4 + k], hi = box[c * 4 + 2 + k];
    const bool any = lo <= hi;                          // (a chart always has a face; an untouched box gives 0, 0)
    bbox_min[i] = any ? unordered(lo) : 0.f;
    extent[i] = any ? __fsub_rn(unordered(hi), unordered(lo)) : 0.f;
  }
}

// vt[3 f + corner] = (origin + padding + 0.5 + (p - bbox_min) scale) / R in double, rounded once
__global__ __launch_bounds__(256) void chart_uv(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                                                 const int32_t* __restrict__ cls, const int64_t* __restrict__ chart, int64_t C,
                                                 const float* __restrict__ bbox_min, const int64_t* __restrict__ origin, double scale, int32_t padding,
                                                 int32_t R, float* __restrict__ vt) {
  for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < 3 * F; h += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = h / 3, a = faces[h], c = chart[f];
    float u = 0.f, v = 0.f;
    if (a >= 0 && a < V && c >= 0 && c < C) {
      float pu, pv;
      project(verts + a * 3, cls[f], pu, pv);
      u = (float)(((double)origin[c * 2] + (double)padding + 0.5 + ((double)pu - (double)bbox_min[c * 2]) * scale) / (double)R);
      v = (float)(((double)origin[c * 2 + 1] + (double)padding + 0.5 + ((double)pv - (double)bbox_min[c * 2 + 1]) * scale) / (double)R);
    }
    vt[h * 2] = u; vt[h * 2 + 1] = v;
  }
}

// ---------------------------------------------------------------------------------------------- contested texels
// wavefront per face over the face's texel box (uv_claim's walk in texture.hip); a texel centre counts for the face when every
// barycentric exceeds eps
__global__ __launch_bounds__(256) void overlap_mark(const float* __restrict__ vt, const int64_t* __restrict__ ft, int64_t Vt, int64_t F, int32_t R,
                                                     double eps, int32_t* __restrict__ count) {
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
    for (int64_t i = lane; i < n; i += SR_WAVE) {
      const int r = r0 + (int)(i / bw), c = c0 + (int)(i % bw);
      double e0, e1, e2;
      uv_edges(t, (c + 0.5) / R, 1. - (r + 0.5) / R, e0, e1, e2);
      if (e0 / t.area2 > eps && e1 / t.area2 > eps && e2 / t.area2 > eps) atomicAdd(count + (int64_t)r * R + c, 1);
    }
  }
}

__global__ __launch_bounds__(256) void overlap_total(const int32_t* __restrict__ count, int64_t texels, unsigned long long* __restrict__ total) {
  int32_t n = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < texels; i += (int64_t)gridDim.x * blockDim.x) n += count[i] >= 2 ? 1 : 0;
  sr_record_add(total, n);
}
}  // namespace

extern "C" int sr_meshprep_bounds(const float* verts, int64_t V, int32_t* box, void* stream) {
  if (!verts || !box || V <= 0) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bounds_init, dim3(1), dim3(64), 0, st, box);
  sr_launch_stream(bounds_reduce, V, 256, st, verts, V, box);
  hipLaunchKernelGGL(bounds_finish, dim3(1), dim3(64), 0, st, box);
  return sr_launch_status();
}

extern "C" int sr_meshprep_cell_keys(const float* verts, int64_t V, const float* lo, float cell, int64_t nx, int64_t ny, int64_t nz, int64_t* key,
                                     void* stream) {
  if (!verts || !lo || !key || V <= 0 || !(cell > 0.f) || nx <= 0 || ny <= 0 || nz <= 0) return SR_EINVAL;
  const __int128 lim = (__int128)1 << 62;                                                 // the keys need nx ny nz < 2^62
  if ((__int128)nx * ny >= lim || (__int128)nx * ny * nz >= lim) return SR_EINVAL;
  sr_launch_stream(cell_keys, V, 256, stream, verts, V, lo, cell, nx, ny, nz, key);
  return sr_launch_status();
}

extern "C" int sr_meshprep_cell_mean(const float* verts, int64_t V, const int64_t* order, const int64_t* offsets, int64_t C, float* out, void* stream) {
  if (!verts || !order || !offsets || !out || V <= 0 || C <= 0) return SR_EINVAL;
  sr_launch_stream(cell_mean, C, 256, stream, verts, V, order, offsets, C, out);
  return sr_launch_status();
}

extern "C" int sr_meshprep_face_keys(const int64_t* faces, int64_t F, const int64_t* vertex_map, int64_t V, int64_t Vn, int64_t* out_faces,
                                     int64_t* key_hi, int64_t* key_lo, void* stream) {
  if (!faces || !vertex_map || !out_faces || !key_hi || !key_lo || F <= 0 || V <= 0 || Vn <= 0 || Vn > ((int64_t)1 << 31)) return SR_EINVAL;
  sr_launch_stream(face_keys, F, 256, stream, faces, F, vertex_map, V, Vn, out_faces, key_hi, key_lo);
  return sr_launch_status();
}

extern "C" int sr_meshprep_face_first(const int64_t* key_hi, const int64_t* key_lo, const int64_t* perm, int64_t F, uint8_t* keep, void* stream) {
  if (!key_hi || !key_lo || !perm || !keep || F <= 0) return SR_EINVAL;
  sr_launch_stream(face_first, F, 256, stream, key_hi, key_lo, perm, F, keep);
  return sr_launch_status();
}

extern "C" int sr_meshprep_cell_faces(const int64_t* faces, int64_t F, const int64_t* vertex_map, int64_t V, int64_t C, int64_t* slot, void* stream) {
  if (!faces || !vertex_map || !slot || F <= 0 || V <= 0 || C <= 0) return SR_EINVAL;
  sr_launch_stream(cell_face_slots, F, 256, stream, faces, F, vertex_map, V, C, slot);
  return sr_launch_status();
}

extern "C" int sr_meshprep_cell_quadric(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* face_slots,
                                        const int64_t* face_offsets, const int64_t* order, const int64_t* offsets, const int64_t* cells, int64_t C,
                                        const float* lo, float cell, int64_t nx, int64_t ny, double reg, float* out, int32_t* flags, float* shift,
                                        void* stream) {
  if (!verts || !faces || !face_slots || !face_offsets || !order || !offsets || !cells || !lo || !out || !flags || !shift || V <= 0 || F <= 0 ||
      C <= 0 || !(cell > 0.f) || nx <= 0 || ny <= 0 || !(reg > 0.) || !(reg < INFINITY))
    return SR_EINVAL;
  if (F > INT64_MAX / 3 || C > INT64_MAX / SR_QUADRIC_LANES || (__int128)nx * ny >= ((__int128)1 << 62)) return SR_EINVAL;
  sr_launch_stream(cell_quadric, C * SR_QUADRIC_LANES, 256, stream, verts, V, faces, F, face_slots, face_offsets, order, offsets, cells, C, lo, cell, nx, ny,
                   reg, out, flags, shift);
  return sr_launch_status();
}

extern "C" int sr_meshprep_face_flips(const float* verts, int64_t V, const int64_t* faces, int64_t F, const float* new_verts, int64_t Vn,
                                      const int64_t* new_faces, const int64_t* source, int64_t Fn, int64_t* counts, void* stream) {
  if (!verts || !faces || !new_verts || !new_faces || !source || !counts || V <= 0 || F <= 0 || Vn <= 0 || Fn <= 0) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 16, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(face_flips, Fn, 256, st, verts, V, faces, F, new_verts, Vn, new_faces, source, Fn, (unsigned long long*)counts);
  return sr_launch_status();
}

extern "C" int sr_chart_classify(const float* verts, int64_t V, const int64_t* faces, int64_t F, int32_t* cls, void* stream) {
  if (!verts || !faces || !cls || V <= 0 || F <= 0) return SR_EINVAL;
  sr_launch_stream(chart_classify, F, 256, stream, verts, V, faces, F, cls);
  return sr_launch_status();
}

extern "C" int sr_chart_edge_keys(const int64_t* faces, int64_t F, int64_t V, const int32_t* cls, int64_t* key, void* stream) {
  if (!faces || !cls || !key || F <= 0 || V <= 0 || V > ((int64_t)1 << 30)) return SR_EINVAL;       // (V V 6 < 2^63)
  sr_launch_stream(chart_edge_keys, 3 * F, 256, stream, faces, F, V, cls, key);
  return sr_launch_status();
}

extern "C" int sr_chart_hook(const int64_t* sorted_key, const int64_t* perm, int64_t n, const int32_t* parent, int32_t* next, int64_t F, int32_t* changed,
                             void* stream) {
  if (!sorted_key || !perm || !parent || !next || !changed || F <= 0 || F >= INT32_MAX || n != 3 * F) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(changed, 0, 4, st) != hipSuccess) return SR_ELAUNCH;
  if (hipMemcpyAsync(next, parent, (size_t)F * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(chart_hook, n, 256, st, sorted_key, perm, n, parent, next, F, changed);
  return sr_launch_status();
}

extern "C" int sr_chart_jump(const int32_t* parent, int64_t F, int32_t* next, int32_t* changed, void* stream) {
  if (!parent || !next || !changed || F <= 0 || F >= INT32_MAX) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(changed, 0, 4, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(chart_jump, F, 256, st, parent, F, next, changed);
  return sr_launch_status();
}

extern "C" int sr_chart_bbox(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int32_t* cls, const int64_t* chart, int64_t C,
                             int32_t* box, float* bbox_min, float* extent, void* stream) {
  if (!verts || !faces || !cls || !chart || !box || !bbox_min || !extent || V <= 0 || F <= 0 || C <= 0) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  sr_launch_stream(box_init, 4 * C, 256, st, box, C);
  sr_launch_stream(chart_box, F, 256, st, verts, V, faces, F, cls, chart, C, box);
  sr_launch_stream(box_finish, 2 * C, 256, st, (const int32_t*)box, C, bbox_min, extent);
  return sr_launch_status();
}

extern "C" int sr_chart_uv(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int32_t* cls, const int64_t* chart, int64_t C,
                           const float* bbox_min, const int64_t* origin, double scale, int32_t padding, int32_t R, float* vt, void* stream) {
  if (!verts || !faces || !cls || !chart || !bbox_min || !origin || !vt || V <= 0 || F <= 0 || C <= 0 || !(scale >= 0.) || padding < 0 || R <= 0)
    return SR_EINVAL;
  sr_launch_stream(chart_uv, 3 * F, 256, stream, verts, V, faces, F, cls, chart, C, bbox_min, origin, scale, padding, R, vt);
  return sr_launch_status();
}

extern "C" int sr_uv_overlap_count(const float* vt, const int64_t* ft, int64_t Vt, int64_t F, int32_t R, double eps, int32_t* count, int64_t* total,
                                   void* stream) {
  if (!vt || !ft || !count || !total || Vt <= 0 || F <= 0 || R <= 0 || R > 32768 || !(eps >= 0.)) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t texels = (int64_t)R * R;
  if (hipMemsetAsync(count, 0, (size_t)texels * 4, st) != hipSuccess || hipMemsetAsync(total, 0, 8, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(overlap_mark, F * SR_WAVE, 256, st, vt, ft, Vt, F, R, eps, count);
  sr_launch_stream(overlap_total, texels, 256, st, (const int32_t*)count, texels, (unsigned long long*)total);
  return sr_launch_status();
}
