// Surface-distance evaluation (semantics stated there, this package's own, held to a float64 restatement): the exact
// Euclidean distance from points to a triangle mesh taken as a set of closed triangles, through a uniform grid over the mesh, and a
// stratified area-weighted surface sampler.  Sorting, cumulative sums and the cell table are torch's (surfdist_ops.py).
//
//  * sr_surfdist_face_cells / sr_surfdist_emit_pairs: per face the cells its box overlaps (conservative), counted and then written as
//    (cell key, face) pairs at the offsets of a cumulative sum: ascending face order, so a stable sort by key leaves every cell's faces
//    ascending.  No atomics.
//  * sr_surfdist_query: one lane per point.  Chebyshev rings of cells round the cell nearest the point; it stops when the best squared
//    distance is below the shrunk lower bound of everything unvisited, or when nothing is unvisited.
//  * sr_surfdist_brute: the same device function over all faces, staged through the LDS in tiles: method "brute" and the witness.
//  * sr_mesh_sample: sample i at the stratified position (i + xi) / n of the cumulative area, splitmix64 of (seed, 3 i + {0, 1, 2}).
//
// The distance function, the tie rule and the ring walk are surfdist_device.h's (shared with icp.hip): the result does not depend on
// the order of the visits, so grid and brute agree bit for bit.  Every loop runs over an integer range fixed before it starts; a
// float comparison only ever leaves a loop early, and a non-finite point never enters one.
#include "surfdist_device.h"

namespace {
using namespace srsd;

__device__ __forceinline__ void write_result(const Best& b, bool finite, int64_t i, float* __restrict__ dist, int64_t* __restrict__ face,
                                             float* __restrict__ closest) {
  const bool ok = finite && b.f != INT32_MAX;
  dist[i] = ok ? sqrtf(b.d2) : NAN;
  face[i] = ok ? (int64_t)b.f : -1;
  closest[i * 3] = ok ? b.qx : NAN; closest[i * 3 + 1] = ok ? b.qy : NAN; closest[i * 3 + 2] = ok ? b.qz : NAN;
}

// ---------------------------------------------------------------------------------------------- grid build
__device__ __forceinline__ void face_range(const Tri& t, const float* __restrict__ lo, float cell, int32_t nx, int32_t ny, int32_t nz, int32_t r[6]) {
  r[0] = cell_of(fminf(t.ax, fminf(t.bx, t.cx)), lo[0], cell, nx); r[1] = cell_of(fmaxf(t.ax, fmaxf(t.bx, t.cx)), lo[0], cell, nx);
  r[2] = cell_of(fminf(t.ay, fminf(t.by, t.cy)), lo[1], cell, ny); r[3] = cell_of(fmaxf(t.ay, fmaxf(t.by, t.cy)), lo[1], cell, ny);
  r[4] = cell_of(fminf(t.az, fminf(t.bz, t.cz)), lo[2], cell, nz); r[5] = cell_of(fmaxf(t.az, fmaxf(t.bz, t.cz)), lo[2], cell, nz);
}

__global__ __launch_bounds__(256) void face_cells(const float4* __restrict__ tri, int64_t F, const float* __restrict__ lo, float cell, int32_t nx,
                                                   int32_t ny, int32_t nz, int64_t* __restrict__ count) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    int32_t r[6];
    face_range(load_tri(tri, f), lo, cell, nx, ny, nz, r);
    count[f] = (int64_t)(r[1] - r[0] + 1) * (r[3] - r[2] + 1) * (r[5] - r[4] + 1);
  }
}

// face f writes its pairs at offset[f] .. offset[f] + count(f), cells in ascending key; nothing beyond `pairs`
__global__ __launch_bounds__(256) void emit_pairs(const float4* __restrict__ tri, int64_t F, const float* __restrict__ lo, float cell, int32_t nx,
                                                   int32_t ny, int32_t nz, const int64_t* __restrict__ offset, int64_t pairs,
                                                   int64_t* __restrict__ key, int32_t* __restrict__ pair_face) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    int32_t r[6];
    face_range(load_tri(tri, f), lo, cell, nx, ny, nz, r);
    int64_t o = offset[f];
    if (o < 0) continue;
    for (int32_t k = r[4]; k <= r[5]; ++k)
      for (int32_t j = r[2]; j <= r[3]; ++j)
        for (int32_t i = r[0]; i <= r[1]; ++i, ++o) {
          if (o >= pairs) continue;
          key[o] = ((int64_t)k * ny + j) * nx + i;
          pair_face[o] = (int32_t)f;
        }
  }
}

// ---------------------------------------------------------------------------------------------- queries
__global__ __launch_bounds__(256) void grid_query(const float* __restrict__ points, int64_t P, const float4* __restrict__ tri, int64_t F,
                                                   const float* __restrict__ lo, float cell, int32_t nx, int32_t ny, int32_t nz,
                                                   const int64_t* __restrict__ cell_start, const int32_t* __restrict__ cell_faces, int64_t pairs,
                                                   float* __restrict__ dist, int64_t* __restrict__ face, float* __restrict__ closest) {
  const Grid g{tri, F, lo, cell, nx, ny, nz, cell_start, cell_faces, pairs};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
    const bool finite = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    if (!finite) { write_result(no_best(), false, i, dist, face, closest); continue; }
    write_result(grid_search(p, g), true, i, dist, face, closest);
  }
}

__global__ __launch_bounds__(256) void brute_query(const float* __restrict__ points, int64_t P, const float4* __restrict__ tri, int64_t F,
                                                    float* __restrict__ dist, int64_t* __restrict__ face, float* __restrict__ closest) {
  __shared__ float4 tile[256 * 3];
  for (int64_t base = (int64_t)blockIdx.x * 256; base < P; base += (int64_t)gridDim.x * 256) {      // (uniform over the block)
    const int64_t i = base + threadIdx.x;
    const bool live = i < P;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = points[i * 3]; py = points[i * 3 + 1]; pz = points[i * 3 + 2]; }
    const bool finite = live && isfinite(px) && isfinite(py) && isfinite(pz);
    Best b = no_best();
    for (int64_t f0 = 0; f0 < F; f0 += 256) {
      const int32_t m = (int32_t)min((int64_t)256, F - f0);
      __syncthreads();
      for (int32_t s = threadIdx.x; s < m * 3; s += 256) tile[s] = tri[f0 * 3 + s];
      __syncthreads();
      if (finite)
        for (int32_t s = 0; s < m; ++s) {
          const float4 t0 = tile[s * 3], t1 = tile[s * 3 + 1], t2 = tile[s * 3 + 2];
          consider(b, px, py, pz, Tri{t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x}, (int32_t)(f0 + s));
        }
    }
    if (live) write_result(b, finite, i, dist, face, closest);
  }
}

// ---------------------------------------------------------------------------------------------- sampler
__device__ __forceinline__ double splitmix_unit(uint64_t idx, uint64_t seed_term) {
  uint64_t h = idx + seed_term;
  h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27; h *= 0x94D049BB133111EBull;
  h ^= h >> 31;
  return (double)(h >> 11) * 0x1p-53;
}

__global__ __launch_bounds__(256) void mesh_sample(const float4* __restrict__ tri, const double* __restrict__ cum_area, int64_t F, int64_t n,
                                                    uint64_t seed_term, float* __restrict__ points, int64_t* __restrict__ face,
                                                    float* __restrict__ normals) {
#pragma clang fp contract(off)
  const double A = cum_area[F - 1];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double xi = splitmix_unit(3 * (uint64_t)i, seed_term), u = splitmix_unit(3 * (uint64_t)i + 1, seed_term),
                 v = splitmix_unit(3 * (uint64_t)i + 2, seed_term);
    const double r = ((double)i + xi) / (double)n * A;
    // the first face whose cumulative area exceeds r; when none does (r rounded up to A), the first that reaches A
    const bool top = !(r < A);
    int64_t lo = 0, hi = F - 1;                          // cum_area[F - 1] = A satisfies either condition
    for (int it = 0; it < 64 && lo < hi; ++it) {
      const int64_t mid = lo + (hi - lo) / 2;
      const double cm = cum_area[mid];
      if (top ? cm >= A : cm > r) hi = mid; else lo = mid + 1;
    }
    const Tri t = load_tri(tri, lo);
    const double su = sqrt(u), w0 = 1. - su, w1 = su * (1. - v), w2 = su * v;
    points[i * 3] = (float)(w0 * (double)t.ax + w1 * (double)t.bx + w2 * (double)t.cx);
    points[i * 3 + 1] = (float)(w0 * (double)t.ay + w1 * (double)t.by + w2 * (double)t.cy);
    points[i * 3 + 2] = (float)(w0 * (double)t.az + w1 * (double)t.bz + w2 * (double)t.cz);
    const double ux = (double)t.bx - (double)t.ax, uy = (double)t.by - (double)t.ay, uz = (double)t.bz - (double)t.az;
    const double vx = (double)t.cx - (double)t.ax, vy = (double)t.cy - (double)t.ay, vz = (double)t.cz - (double)t.az;
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double len = sqrt(nx * nx + ny * ny + nz * nz), inv = len > 0. ? 1. / len : 0.;
    normals[i * 3] = (float)(nx * inv); normals[i * 3 + 1] = (float)(ny * inv); normals[i * 3 + 2] = (float)(nz * inv);
    face[i] = lo;
  }
}

}  // namespace

extern "C" int sr_surfdist_face_cells(const float* tri, int64_t F, const float* lo, float cell, int32_t nx, int32_t ny, int32_t nz, int64_t* count,
                                      void* stream) {
  if (!tri || !lo || !count || F <= 0 || F >= INT32_MAX || misaligned(tri) || bad_grid(cell, nx, ny, nz)) return SR_EINVAL;
  sr_launch_stream(face_cells, F, 256, stream, (const float4*)tri, F, lo, cell, nx, ny, nz, count);
  return sr_launch_status();
}

extern "C" int sr_surfdist_emit_pairs(const float* tri, int64_t F, const float* lo, float cell, int32_t nx, int32_t ny, int32_t nz,
                                      const int64_t* offset, int64_t pairs, int64_t* key, int32_t* pair_face, void* stream) {
  if (!tri || !lo || !offset || !key || !pair_face || F <= 0 || F >= INT32_MAX || pairs < F || misaligned(tri) || bad_grid(cell, nx, ny, nz))
    return SR_EINVAL;
  sr_launch_stream(emit_pairs, F, 256, stream, (const float4*)tri, F, lo, cell, nx, ny, nz, offset, pairs, key, pair_face);
  return sr_launch_status();
}

extern "C" int sr_surfdist_query(const float* points, int64_t P, const float* tri, int64_t F, const float* lo, float cell, int32_t nx, int32_t ny,
                                 int32_t nz, const int64_t* cell_start, const int32_t* cell_faces, int64_t pairs, float* dist, int64_t* face,
                                 float* closest, void* stream) {
  if (!points || !tri || !lo || !cell_start || !cell_faces || !dist || !face || !closest || P <= 0 || F <= 0 || F >= INT32_MAX || pairs < 0 ||
      misaligned(tri) || bad_grid(cell, nx, ny, nz))
    return SR_EINVAL;
  sr_launch_stream(grid_query, P, 256, stream, points, P, (const float4*)tri, F, lo, cell, nx, ny, nz, cell_start, cell_faces, pairs, dist, face, closest);
  return sr_launch_status();
}

extern "C" int sr_surfdist_brute(const float* points, int64_t P, const float* tri, int64_t F, float* dist, int64_t* face, float* closest,
                                 void* stream) {
  if (!points || !tri || !dist || !face || !closest || P <= 0 || F <= 0 || F >= INT32_MAX || misaligned(tri)) return SR_EINVAL;
  sr_launch_stream(brute_query, P, 256, stream, points, P, (const float4*)tri, F, dist, face, closest);
  return sr_launch_status();
}

extern "C" int sr_mesh_sample(const float* tri, const double* cum_area, int64_t F, int64_t n, int64_t seed, float* points, int64_t* face,
                              float* normals, void* stream) {
  if (!tri || !cum_area || !points || !face || !normals || F <= 0 || F >= INT32_MAX || n <= 0 || n > ((int64_t)1 << 40) || misaligned(tri))
    return SR_EINVAL;
  const uint64_t seed_term = (uint64_t)seed * 0x9E3779B97F4A7C15ull;
  sr_launch_stream(mesh_sample, n, 256, stream, (const float4*)tri, cum_area, F, n, seed_term, points, face, normals);
  return sr_launch_status();
}
