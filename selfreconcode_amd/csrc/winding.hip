// Generalized winding number of points against a triangle mesh: w(p) = 1 / (4 pi) sum_f Omega_f(p), Omega_f the signed
// solid angle of face f seen from p.  1 inside and 0 outside a closed mesh with outward faces; a hole moves it smoothly.
//
//  * sr_winding_brute: the exact sum, faces in ascending index staged through the LDS in tiles of 256: method "brute" and the witness.
//  * sr_winding_keys / sr_winding_leaves / sr_winding_fold: a dense octree pyramid over a cube (layout: winding_abi.h).  A face belongs
//    to the leaf that holds its float32 centroid; torch sorts the keys stably and makes the run starts (winding_ops.py); a leaf sums its
//    run in ascending face order in double, and one launch per level folds eight children into their parent.  No atomics.
//  * sr_winding_query: one lane per point, depth first from the root with the children in index order.  A node without area is skipped
//    with its subtree; one with |p - c| > beta r contributes the dipole -N . (p - c) / |p - c|^3; otherwise a leaf contributes its faces
//    exactly and an inner node is opened.  The successor of a node follows from (level, index), so the walk keeps no stack.
//
// The solid angle and the acceptance test are float32 without contraction, as tests/_winding_ref.py restates them; the terms of a
// point are summed in double in the order of the walk, which depends on the point alone: two calls, and any order of the points, give
// identical bits.  Every loop runs over an integer range fixed before it starts; a float comparison chooses between a node's three
// treatments and never the length of a loop; a non-finite point enters none.
#include "surfdist_device.h"
#include "winding_abi.h"

namespace {
using namespace srsd;

#define WN_INV_4PI 0.07957747154594767                /* 1 / (4 pi) */

__device__ __forceinline__ int64_t level_offset(int32_t level) { return ((((int64_t)1) << (3 * level)) - 1) / 7; }

// bits 0 .. 9 of x to bits 0, 3, 6, ...
__device__ __forceinline__ int32_t spread3(int32_t x) {
  x &= 0x3FF;
  x = (x | (x << 16)) & 0x030000FF;
  x = (x | (x << 8)) & 0x0300F00F;
  x = (x | (x << 4)) & 0x030C30C3;
  x = (x | (x << 2)) & 0x09249249;
  return x;
}

// Omega of the triangle seen from p (van Oosterom and Strackee): 0 for p at a corner (atan2f(0, 0)), and for a face without area
__device__ __forceinline__ float solid_angle(float px, float py, float pz, const Tri& t) {
#pragma clang fp contract(off)
  const float ax = t.ax - px, ay = t.ay - py, az = t.az - pz;
  const float bx = t.bx - px, by = t.by - py, bz = t.bz - pz;
  const float cx = t.cx - px, cy = t.cy - py, cz = t.cz - pz;
  const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz), lc = sqrtf(cx * cx + cy * cy + cz * cz);
  const float det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
  const float ab = ax * bx + ay * by + az * bz, bc = bx * cx + by * cy + bz * cz, ca = cx * ax + cy * ay + cz * az;
  const float den = la * lb * lc + ab * lc + bc * la + ca * lb;
  return 2.f * atan2f(det, den);
}

// ---------------------------------------------------------------------------------------------- tree build
__global__ __launch_bounds__(256) void leaf_keys(const float* __restrict__ src, int64_t n, int32_t faces, const float* __restrict__ lo, float cell,
                                                  int32_t levels, int64_t* __restrict__ key) {
#pragma clang fp contract(off)
  const int32_t cells = 1 << levels;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float x, y, z;
    if (faces) {
      const Tri t = load_tri((const float4*)src, i);
      x = ((t.ax + t.bx) + t.cx) / 3.f; y = ((t.ay + t.by) + t.cy) / 3.f; z = ((t.az + t.bz) + t.cz) / 3.f;
    } else {
      x = src[i * 3]; y = src[i * 3 + 1]; z = src[i * 3 + 2];
    }
    key[i] = (int64_t)(spread3(cell_of(x, lo[0], cell, cells)) | (spread3(cell_of(y, lo[1], cell, cells)) << 1) |
                       (spread3(cell_of(z, lo[2], cell, cells)) << 2));
  }
}

__device__ __forceinline__ void store_node(float4* __restrict__ nodes, int64_t node, double nx, double ny, double nz, const float (&c)[3], double area,
                                           double radius) {
  nodes[node * 2] = make_float4((float)nx, (float)ny, (float)nz, c[0]);
  nodes[node * 2 + 1] = make_float4(c[1], c[2], (float)area, (float)radius);
}

__global__ __launch_bounds__(256) void leaf_nodes(const float4* __restrict__ tri, int64_t F, const int64_t* __restrict__ leaf_start,
                                                   const int32_t* __restrict__ leaf_faces, int32_t levels, float4* __restrict__ nodes) {
#pragma clang fp contract(off)
  const int64_t leaves = (int64_t)1 << (3 * levels), base = level_offset(levels);
  for (int64_t leaf = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; leaf < leaves; leaf += (int64_t)gridDim.x * blockDim.x) {
    int64_t s = leaf_start[leaf], e = leaf_start[leaf + 1];
    s = s < 0 ? 0 : s; e = e > F ? F : e;
    double nx = 0., ny = 0., nz = 0., area = 0., mx = 0., my = 0., mz = 0.;
    for (int64_t m = s; m < e; ++m) {
      const int32_t f = leaf_faces[m];
      if (f < 0 || f >= F) continue;
      const Tri t = load_tri(tri, f);
      const double ux = (double)t.bx - (double)t.ax, uy = (double)t.by - (double)t.ay, uz = (double)t.bz - (double)t.az;
      const double vx = (double)t.cx - (double)t.ax, vy = (double)t.cy - (double)t.ay, vz = (double)t.cz - (double)t.az;
      const double fx = 0.5 * (uy * vz - uz * vy), fy = 0.5 * (uz * vx - ux * vz), fz = 0.5 * (ux * vy - uy * vx);
      const double a = sqrt(fx * fx + fy * fy + fz * fz);
      nx += fx; ny += fy; nz += fz; area += a;
      mx += a * ((((double)t.ax + (double)t.bx) + (double)t.cx) / 3.);
      my += a * ((((double)t.ay + (double)t.by) + (double)t.cy) / 3.);
      mz += a * ((((double)t.az + (double)t.bz) + (double)t.cz) / 3.);
    }
    const bool any = area > 0.;
    const float c[3] = {any ? (float)(mx / area) : 0.f, any ? (float)(my / area) : 0.f, any ? (float)(mz / area) : 0.f};
    double r2 = 0.;
    for (int64_t m = s; m < e; ++m) {
      const int32_t f = leaf_faces[m];
      if (f < 0 || f >= F) continue;
      const Tri t = load_tri(tri, f);
      const double q[9] = {t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double dx = q[k * 3] - (double)c[0], dy = q[k * 3 + 1] - (double)c[1], dz = q[k * 3 + 2] - (double)c[2];
        r2 = fmax(r2, dx * dx + dy * dy + dz * dz);
      }
    }
    store_node(nodes, base + leaf, nx, ny, nz, c, area, any ? sqrt(r2) : 0.);
  }
}

__global__ __launch_bounds__(256) void fold_nodes(float4* __restrict__ nodes, int32_t level) {
#pragma clang fp contract(off)
  const int64_t count = (int64_t)1 << (3 * level), base = level_offset(level), child = level_offset(level + 1);
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < count; m += (int64_t)gridDim.x * blockDim.x) {
    double nx = 0., ny = 0., nz = 0., area = 0., mx = 0., my = 0., mz = 0.;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float4 n0 = nodes[(child + m * 8 + k) * 2], n1 = nodes[(child + m * 8 + k) * 2 + 1];
      const double a = n1.z > 0.f ? (double)n1.z : 0.;
      nx += (double)n0.x; ny += (double)n0.y; nz += (double)n0.z; area += a;
      mx += a * (double)n0.w; my += a * (double)n1.x; mz += a * (double)n1.y;
    }
    const bool any = area > 0.;
    const float c[3] = {any ? (float)(mx / area) : 0.f, any ? (float)(my / area) : 0.f, any ? (float)(mz / area) : 0.f};
    double r = 0.;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float4 n0 = nodes[(child + m * 8 + k) * 2], n1 = nodes[(child + m * 8 + k) * 2 + 1];
      if (!(n1.z > 0.f)) continue;
      const double dx = (double)n0.w - (double)c[0], dy = (double)n1.x - (double)c[1], dz = (double)n1.y - (double)c[2];
      r = fmax(r, sqrt(dx * dx + dy * dy + dz * dz) + (double)n1.w);
    }
    store_node(nodes, base + m, nx, ny, nz, c, area, r);
  }
}

// ---------------------------------------------------------------------------------------------- queries
__global__ __launch_bounds__(256) void tree_query(const float* __restrict__ points, int64_t P, const float4* __restrict__ tri, int64_t F,
                                                   const float4* __restrict__ nodes, int32_t levels, const int64_t* __restrict__ leaf_start,
                                                   const int32_t* __restrict__ leaf_faces, float beta, int32_t open_all, float* __restrict__ w) {
#pragma clang fp contract(off)
  const int64_t total = level_offset(levels + 1);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const float px = points[i * 3], py = points[i * 3 + 1], pz = points[i * 3 + 2];
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) { w[i] = NAN; continue; }
    double sum = 0.;
    int32_t l = 0, m = 0;                                 // the node: index m of level l
    for (int64_t it = 0; it < total; ++it) {              // (every node is visited at most once)
      const int64_t node = level_offset(l) + m;
      const float4 n0 = nodes[node * 2], n1 = nodes[node * 2 + 1];
      if (n1.z > 0.f) {
        const float dx = px - n0.w, dy = py - n1.x, dz = pz - n1.y;
        const float d2 = dx * dx + dy * dy + dz * dz, br = beta * n1.w;
        if (!open_all && d2 > br * br) {
          sum += (double)(-(n0.x * dx + n0.y * dy + n0.z * dz) / (d2 * sqrtf(d2)));
        } else if (l < levels) {
          ++l; m <<= 3;                                   // open: the first child
          continue;
        } else {
          int64_t s = leaf_start[m], e = leaf_start[m + 1];
          s = s < 0 ? 0 : s; e = e > F ? F : e;
          for (int64_t k = s; k < e; ++k) {
            const int32_t f = leaf_faces[k];
            if (f < 0 || f >= F) continue;
            sum += (double)solid_angle(px, py, pz, load_tri(tri, f));
          }
        }
      }
      // the successor: the next sibling, of the nearest ancestor that has one (a last child's index ends in the digit 7)
      const int32_t up = min(__builtin_ctz(~m) / 3, l);
      m >>= 3 * up; l -= up;
      if (l == 0) break;
      ++m;
    }
    w[i] = (float)(sum * WN_INV_4PI);
  }
}

__global__ __launch_bounds__(256) void brute_winding(const float* __restrict__ points, int64_t P, const float4* __restrict__ tri, int64_t F,
                                                      float* __restrict__ w) {
  __shared__ float4 tile[256 * 3];
  for (int64_t base = (int64_t)blockIdx.x * 256; base < P; base += (int64_t)gridDim.x * 256) {      // (uniform over the block)
    const int64_t i = base + threadIdx.x;
    const bool live = i < P;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = points[i * 3]; py = points[i * 3 + 1]; pz = points[i * 3 + 2]; }
    const bool finite = live && isfinite(px) && isfinite(py) && isfinite(pz);
    double sum = 0.;
    for (int64_t f0 = 0; f0 < F; f0 += 256) {
      const int32_t n = (int32_t)min((int64_t)256, F - f0);
      __syncthreads();
      for (int32_t s = threadIdx.x; s < n * 3; s += 256) tile[s] = tri[f0 * 3 + s];
      __syncthreads();
      if (finite)
        for (int32_t s = 0; s < n; ++s) {
          const float4 t0 = tile[s * 3], t1 = tile[s * 3 + 1], t2 = tile[s * 3 + 2];
          sum += (double)solid_angle(px, py, pz, Tri{t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x});
        }
    }
    if (live) w[i] = finite ? (float)(sum * WN_INV_4PI) : NAN;
  }
}

inline bool bad_levels(int32_t levels) { return levels < 0 || levels > SR_WINDING_MAX_LEVELS; }

}  // namespace

extern "C" int sr_winding_keys(const float* src, int64_t n, int32_t faces, const float* lo, float cell, int32_t levels, int64_t* key, void* stream) {
  if (!src || !lo || !key || n <= 0 || (faces && n >= INT32_MAX) || (faces != 0 && faces != 1) || bad_levels(levels) || !(cell > 0.f) || !isfinite(cell) ||
      (faces && misaligned(src)))
    return SR_EINVAL;
  sr_launch_stream(leaf_keys, n, 256, stream, src, n, faces, lo, cell, levels, key);
  return sr_launch_status();
}

extern "C" int sr_winding_leaves(const float* tri, int64_t F, const int64_t* leaf_start, const int32_t* leaf_faces, int32_t levels, float* nodes,
                                 void* stream) {
  if (!tri || !leaf_start || !leaf_faces || !nodes || F <= 0 || F >= INT32_MAX || bad_levels(levels) || misaligned(tri) || misaligned(nodes)) return SR_EINVAL;
  sr_launch_stream(leaf_nodes, (int64_t)1 << (3 * levels), 256, stream, (const float4*)tri, F, leaf_start, leaf_faces, levels, (float4*)nodes);
  return sr_launch_status();
}

extern "C" int sr_winding_fold(float* nodes, int32_t level, int32_t levels, void* stream) {
  if (!nodes || bad_levels(levels) || level < 0 || level >= levels || misaligned(nodes)) return SR_EINVAL;
  sr_launch_stream(fold_nodes, (int64_t)1 << (3 * level), 256, stream, (float4*)nodes, level);
  return sr_launch_status();
}

extern "C" int sr_winding_query(const float* points, int64_t P, const float* tri, int64_t F, const float* nodes, int32_t levels,
                                const int64_t* leaf_start, const int32_t* leaf_faces, float beta, int32_t open_all, float* w, void* stream) {
  if (!points || !tri || !nodes || !leaf_start || !leaf_faces || !w || P <= 0 || F <= 0 || F >= INT32_MAX || bad_levels(levels) || misaligned(tri) ||
      misaligned(nodes) || !(beta >= 1.f))
    return SR_EINVAL;
  sr_launch_stream(tree_query, P, 256, stream, points, P, (const float4*)tri, F, (const float4*)nodes, levels, leaf_start, leaf_faces, beta, open_all, w);
  return sr_launch_status();
}

extern "C" int sr_winding_brute(const float* points, int64_t P, const float* tri, int64_t F, float* w, void* stream) {
  if (!points || !tri || !w || P <= 0 || F <= 0 || F >= INT32_MAX || misaligned(tri)) return SR_EINVAL;
  sr_launch_stream(brute_winding, P, 256, stream, points, P, (const float4*)tri, F, w);
  return sr_launch_status();
}
