// Per-point core of the surface-distance evaluation, shared by surfdist.hip and icp.hip: the packed triangle, the
// grid coordinate, the distance of a point to one closed triangle, the tie rule, and the walk over Chebyshev rings of grid cells.
//
// Every candidate's squared distance comes from tri_closest, compiled without contraction, and ties go to the lower face index: the
// result does not depend on the order of the visits.  Every loop runs over an integer range fixed before it starts; a float
// comparison only ever leaves a loop early, and a non-finite point must not enter grid_search (the callers test it first).
#pragma once
#include "sr_common.h"
#include <math.h>

#define SD_TRI 12                                      /* floats per packed triangle: a, b, c, 3 of padding (three float4) */
#define SD_MAX_CELLS ((int64_t)1 << 24)
#define SD_SHRINK 0.99993896484375f                    /* 1 - 2^-14: the factor on the lower bound of the unvisited cells */
#define SD_SLACK 9.5367431640625e-7f                   /* 2^-20 (|lo| + n cell + |p|): the rounding of the cell boundaries */

namespace srsd {

struct Tri { float ax, ay, az, bx, by, bz, cx, cy, cz; };

__device__ __forceinline__ Tri load_tri(const float4* __restrict__ tri, int64_t f) {
  const float4 t0 = tri[f * 3], t1 = tri[f * 3 + 1], t2 = tri[f * 3 + 2];
  return Tri{t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x};
}

// grid coordinate of x on an axis with n cells: floor((x - lo) / cell) in float32, clamped to [0, n - 1]; monotone in x
__device__ __forceinline__ int32_t cell_of(float x, float lo, float cell, int32_t n) {
#pragma clang fp contract(off)
  float t = floorf((x - lo) / cell);
  t = t > 0.f ? t : 0.f;                                // (NaN -> 0)
  const float top = (float)(n - 1);
  t = t < top ? t : top;
  return (int32_t)t;
}

// candidate on the segment s -> e: a zero-length edge is its start point
__device__ __forceinline__ void seg_try(float px, float py, float pz, float sx, float sy, float sz, float ex, float ey, float ez, float& d2, float& qx,
                                        float& qy, float& qz) {
#pragma clang fp contract(off)
  const float dx = ex - sx, dy = ey - sy, dz = ez - sz;
  const float wx = px - sx, wy = py - sy, wz = pz - sz;
  const float dd = dx * dx + dy * dy + dz * dz, dw = wx * dx + wy * dy + wz * dz;
  float t = dd > 0.f ? dw / dd : 0.f;
  t = t > 0.f ? t : 0.f;
  const bool end = t >= 1.f;
  const float x = end ? ex : sx + t * dx, y = end ? ey : sy + t * dy, z = end ? ez : sz + t * dz;
  const float rx = px - x, ry = py - y, rz = pz - z;
  const float c = rx * rx + ry * ry + rz * rz;
  if (c < d2) { d2 = c; qx = x; qy = y; qz = z; }
}

// squared distance from p to the closed triangle and the closest point q: the least of the orthogonal projection (when the triangle
// has a positive area and the projection's barycentrics are all >= 0) and the three clamped edges, the first of equal candidates.
// The distance is that of the difference vector p - q.
__device__ __forceinline__ float tri_closest(float px, float py, float pz, const Tri& t, float& qx, float& qy, float& qz) {
#pragma clang fp contract(off)
  float d2 = INFINITY;
  qx = t.ax; qy = t.ay; qz = t.az;
  const float ux = t.bx - t.ax, uy = t.by - t.ay, uz = t.bz - t.az;
  const float vx = t.cx - t.ax, vy = t.cy - t.ay, vz = t.cz - t.az;
  const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const float nn = nx * nx + ny * ny + nz * nz;
  if (nn > 0.f) {
    const float wx = px - t.ax, wy = py - t.ay, wz = pz - t.az;
    const float gx = uy * wz - uz * wy, gy = uz * wx - ux * wz, gz = ux * wy - uy * wx;               // u x w
    const float bx = wy * vz - wz * vy, by = wz * vx - wx * vz, bz = wx * vy - wy * vx;               // w x v
    const float gamma = (gx * nx + gy * ny + gz * nz) / nn, beta = (bx * nx + by * ny + bz * nz) / nn;
    const float alpha = 1.f - beta - gamma;
    if (alpha >= 0.f && beta >= 0.f && gamma >= 0.f) {
      const float x = t.ax + beta * ux + gamma * vx, y = t.ay + beta * uy + gamma * vy, z = t.az + beta * uz + gamma * vz;
      const float rx = px - x, ry = py - y, rz = pz - z;
      d2 = rx * rx + ry * ry + rz * rz; qx = x; qy = y; qz = z;
    }
  }
  seg_try(px, py, pz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, d2, qx, qy, qz);
  seg_try(px, py, pz, t.bx, t.by, t.bz, t.cx, t.cy, t.cz, d2, qx, qy, qz);
  seg_try(px, py, pz, t.cx, t.cy, t.cz, t.ax, t.ay, t.az, d2, qx, qy, qz);
  return d2;
}

struct Best { float d2, qx, qy, qz; int32_t f; };       // f == INT32_MAX: nothing seen yet

__device__ __forceinline__ Best no_best() { return Best{INFINITY, NAN, NAN, NAN, INT32_MAX}; }

__device__ __forceinline__ void consider(Best& b, float px, float py, float pz, const Tri& t, int32_t f) {
  float qx, qy, qz;
  const float d2 = tri_closest(px, py, pz, t, qx, qy, qz);
  if (d2 < b.d2 || (d2 == b.d2 && f < b.f)) { b.d2 = d2; b.qx = qx; b.qy = qy; b.qz = qz; b.f = f; }
}

// the grid as the query kernels take it: cell_start [cells + 1] / cell_faces [pairs], every cell's faces
struct Grid {
  const float4* __restrict__ tri;
  int64_t F;
  const float* __restrict__ lo;
  float cell;
  int32_t nx, ny, nz;
  const int64_t* __restrict__ cell_start;
  const int32_t* __restrict__ cell_faces;
  int64_t pairs;
};

__device__ __forceinline__ void visit_cell(Best& b, float px, float py, float pz, int32_t c, const Grid& g) {
  int64_t s = g.cell_start[c], e = g.cell_start[c + 1];
  s = s < 0 ? 0 : s; e = e > g.pairs ? g.pairs : e;
  for (int64_t m = s; m < e; ++m) {
    const int32_t f = g.cell_faces[m];
    if (f < 0 || f >= g.F) continue;
    consider(b, px, py, pz, load_tri(g.tri, f), f);
  }
}

// squared lower bound of the distance from p to the cells beyond one side of the visited cube: `d` to the side's plane, ex / ey the
// distances from p to the grid's box along the other two axes (0 inside); nothing when the bound is not positive
__device__ __forceinline__ float side_bound2(float d, float ex, float ey) {
#pragma clang fp contract(off)
  if (!(d > 0.f)) return 0.f;
  return d * d + ex * ex + ey * ey;
}

// The nearest face of the grid's mesh to the finite point p: Chebyshev rings of cells round the cell nearest p; it stops when the
// best squared distance is below the shrunk lower bound of everything unvisited, or when nothing is unvisited.
__device__ __forceinline__ Best grid_search(const float (&p)[3], const Grid& g) {
#pragma clang fp contract(off)
  const int32_t nx = g.nx, ny = g.ny, nz = g.nz;
  const int32_t n[3] = {nx, ny, nz};
  const int32_t rings = max(nx, max(ny, nz));
  const float* __restrict__ lo = g.lo;
  const float cell = g.cell;
  Best b = no_best();
  int32_t c[3];
  float slack[3], out[3];                                // out: distance from p to the grid's box along the axis, less the slack
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c[a] = cell_of(p[a], lo[a], cell, n[a]);
    const float hi = lo[a] + (float)n[a] * cell;
    slack[a] = SD_SLACK * (fabsf(lo[a]) + (float)n[a] * cell + fabsf(p[a]));
    const float below = lo[a] - p[a] - slack[a], above = p[a] - hi - slack[a];
    out[a] = fmaxf(0.f, fmaxf(below, above));
  }
  for (int32_t r = 0; r < rings; ++r) {
    const int32_t k0 = max(c[2] - r, 0), k1 = min(c[2] + r, nz - 1), j0 = max(c[1] - r, 0), j1 = min(c[1] + r, ny - 1);
    const int32_t i0 = max(c[0] - r, 0), i1 = min(c[0] + r, nx - 1);
    for (int32_t k = k0; k <= k1; ++k)
      for (int32_t j = j0; j <= j1; ++j) {
        const int32_t row = (k * ny + j) * nx;
        if (k - c[2] == r || c[2] - k == r || j - c[1] == r || c[1] - j == r) {
          for (int32_t x = i0; x <= i1; ++x) visit_cell(b, p[0], p[1], p[2], row + x, g);
        } else {
          if (c[0] - r >= 0) visit_cell(b, p[0], p[1], p[2], row + c[0] - r, g);
          if (c[0] + r < nx) visit_cell(b, p[0], p[1], p[2], row + c[0] + r, g);   // (r > 0 here)
        }
      }
    // the cells not visited yet lie beyond the sides of the cube of rings 0 .. r that still have cells behind them
    bool any = false;
    float bound2 = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float e1 = out[(a + 1) % 3], e2 = out[(a + 2) % 3];
      if (c[a] - r > 0) {
        any = true;
        bound2 = fminf(bound2, side_bound2(p[a] - (lo[a] + (float)(c[a] - r) * cell) - slack[a], e1, e2));
      }
      if (c[a] + r + 1 < n[a]) {
        any = true;
        bound2 = fminf(bound2, side_bound2(lo[a] + (float)(c[a] + r + 1) * cell - p[a] - slack[a], e1, e2));
      }
    }
    if (!any) break;
    if (b.d2 < bound2 * (SD_SHRINK * SD_SHRINK)) break;
  }
  return b;
}

// what the host entries refuse
static inline bool bad_grid(float cell, int32_t nx, int32_t ny, int32_t nz) {
  return !(cell > 0.f) || !isfinite(cell) || nx <= 0 || ny <= 0 || nz <= 0 || (int64_t)nx * ny > SD_MAX_CELLS || (int64_t)nx * ny * nz > SD_MAX_CELLS;
}
static inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
}  // namespace srsd
