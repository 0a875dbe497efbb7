// Device helpers shared by the kernels that walk an indexed triangle list faces [F,3] int64 (mesh_prep.hip, mesh_collapse.hip, shade.hip,
// texture.hip, texrender.hip): which rows are faces, the corners of a half-edge, a face sent through a vertex map, pointer jumping
// over a forest, and the flush of a per-thread integer counter into a record.  What is about plane quadrics is in quadric_device.h.
#pragma once
#include "sr_common.h"
#include "sr_wave.h"

// a row of a face list is a face when its three indices lie in [0, V): marching cubes pads its list with -1 rows, and they are skipped
static __device__ __forceinline__ bool sr_face_ok(int64_t a, int64_t b, int64_t c, int64_t V) {
  return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

// half-edge h = 3 f + corner runs from that corner to the next one; `opp` is the third corner.  The caller has h in [0, 3 F) and
// checks the indices it uses (sr_edge_ok, or a range test of opp): a member that is not used is not loaded.
struct SrHalfEdge { int64_t from, to, opp; };
static __device__ __forceinline__ SrHalfEdge sr_half_edge(const int64_t* __restrict__ faces, int64_t h) {
  const int64_t f = h / 3, c = h - 3 * f;
  return {faces[h], faces[f * 3 + (c + 1) % 3], faces[f * 3 + (c + 2) % 3]};
}
static __device__ __forceinline__ bool sr_edge_ok(int64_t a, int64_t b, int64_t V) { return a >= 0 && b >= 0 && a < V && b < V && a != b; }

// (x, y, z) = map[the corners of face f], or (-1, -1, -1) for a row that is not a face of V vertices
static __device__ __forceinline__ void sr_face_remap(const int64_t* __restrict__ faces, int64_t f, const int64_t* __restrict__ map, int64_t V, int64_t& x,
                                                     int64_t& y, int64_t& z) {
  const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  x = -1; y = -1; z = -1;
  if (sr_face_ok(a, b, c, V)) { x = map[a]; y = map[b]; z = map[c]; }
}

// one pass of pointer doubling over the forest P [n] (P[i] = i for a root), double-buffered: Q[i] = P[P[i]], *changed = 1 when some
// Q[i] differs from P[i].  An entry outside [0, n) is copied as it is.  The whole body of a grid-stride kernel.
template <typename T>
static __device__ __forceinline__ void sr_forest_jump(const T* __restrict__ P, int64_t n, T* __restrict__ Q, int32_t* __restrict__ changed) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const T p = P[i];
    const T g = p >= 0 && p < n ? P[p] : p;
    Q[i] = g;
    if (g != p) *changed = 1;
  }
}

// record += the sum of `n` over the workgroup's threads: a wave sum, then one integer atomic per wave with something to add.  Every
// thread of the workgroup calls it.
static __device__ __forceinline__ void sr_record_add(unsigned long long* __restrict__ record, int32_t n) {
  n = sr_wave_sum(n);
  if ((threadIdx.x & (SR_WAVE - 1)) == 0 && n) atomicAdd(record, (unsigned long long)n);
}
