// Topology-preserving decimation of the texture template by parallel edge collapse (semantics stated there, unpinned --
// the reference leaves this step to MeshLab / Blender).  One round = the edges of the current mesh, a candidate test and a cost per edge,
// an independent set of candidates, and the collapses of that set; the host (mesh_prep_ops.py) sorts, compacts and loops.
//
//  * sr_collapse_vertex_quadrics   thread per vertex: the plane quadrics of its faces, summed in ascending face index in double.
//  * sr_collapse_edge_keys         half-edge keys min V + max; sr_collapse_edge_heads: thread per unique key -- the endpoints, the face
//                                  count, the two opposite vertices, the lock of both endpoints when the count is not 2, and the two
//                                  directed keys whose sort is the neighbour list of every vertex.
//  * sr_collapse_candidates        thread per edge: Q_a + Q_b, the regularised optimum (quadric_device.h), its float32 rounding, the
//                                  cost there, the link / valence / flip tests, and the key (cost bits, hashed edge index).
//  * sr_collapse_min1 / _min2      m1[v] = the least key at v; m2[v] = the least m1 over v and its neighbours (64-bit integer atomicMin).
//  * sr_collapse_select            key == m2[a] == m2[b], and the round's record (selected, candidates).
//  * sr_collapse_apply_vertices    verts[a] = x, Q_a += Q_b, target[b] = a for the selected; sr_collapse_apply_faces remaps one level.
//  * sr_collapse_map_jump          target[target[v]], double-buffered, for the final vertex map.
//
// Gather- and latency-bound work on at most a few million elements: a thread walks two short CSR lists.  No float atomics anywhere:
// every sum is sequential in one thread, the atomics are integer or / add / min, so two calls give identical bits.  Every list range is
// clamped to its array and every index read from memory is checked before it is used.  The face and half-edge helpers, the face remap,
// the pointer jump and the record flush are mesh_device.h's (shared with mesh_prep.hip); the plane quadric is quadric_device.h's.
#include "sr_common.h"
#include "mesh_device.h"
#include "quadric_device.h"

namespace {

#define SR_COLLAPSE_Q 10                              // doubles per vertex quadric: xx xy xz yy yz zz, bx by bz, c

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {         // murmur3's finaliser: a bijection of the 32-bit integers
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

__device__ __forceinline__ void atomic_min64(int64_t* p, int64_t v) {       // (the keys are non-negative: the unsigned order is theirs)
  atomicMin((unsigned long long*)p, (unsigned long long)v);
}

__global__ __launch_bounds__(256) void vertex_quadrics(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                                                        const int64_t* __restrict__ slots, const int64_t* __restrict__ offsets, double* __restrict__ Q) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    double q[SR_COLLAPSE_Q] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
    const int64_t s = max(offsets[v], (int64_t)0), e = min(offsets[v + 1], 3 * F);
    for (int64_t k = s; k < e; ++k) {
      const int64_t h = slots[k];
      if (h < 0 || h >= 3 * F) continue;
      const int64_t f = h / 3, i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
      if (!sr_face_ok(i0, i1, i2, V)) continue;
      PlaneQuadric p;
      if (!plane_quadric(verts + i0 * 3, verts + i1 * 3, verts + i2 * 3, p)) continue;
      q[0] += p.w0 * p.n0; q[1] += p.w0 * p.n1; q[2] += p.w0 * p.n2; q[3] += p.w1 * p.n1; q[4] += p.w1 * p.n2; q[5] += p.w2 * p.n2;
      q[6] += p.wd * p.n0; q[7] += p.wd * p.n1; q[8] += p.wd * p.n2; q[9] += p.wd * p.d;
    }
#pragma unroll
    for (int k = 0; k < SR_COLLAPSE_Q; ++k) Q[v * SR_COLLAPSE_Q + k] = q[k];
  }
}

// half-edge h = 3 f + corner, from that corner to the next: min V + max; -1 for a row that is not a face
__global__ __launch_bounds__(256) void edge_keys(const int64_t* __restrict__ faces, int64_t F, int64_t V, int64_t* __restrict__ key) {
  for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < 3 * F; h += (int64_t)gridDim.x * blockDim.x) {
    const SrHalfEdge e = sr_half_edge(faces, h);
    const bool ok = sr_face_ok(e.from, e.to, e.opp, V) && e.from != e.to && e.from != e.opp && e.to != e.opp;
    key[h] = ok ? min(e.from, e.to) * V + max(e.from, e.to) : -1;
  }
}

// the vertex opposite half-edge h, or -1
__device__ __forceinline__ int64_t opposite(const int64_t* __restrict__ faces, int64_t F, int64_t V, int64_t h) {
  if (h < 0 || h >= 3 * F) return -1;
  const int64_t o = sr_half_edge(faces, h).opp;
  return o >= 0 && o < V ? o : -1;
}

// thread per unique key: its half-edges are perm[offsets[e] .. offsets[e + 1]) of the sorted list
__global__ __launch_bounds__(256) void edge_heads(const int64_t* __restrict__ ukey, const int64_t* __restrict__ offsets, int64_t E,
                                                   const int64_t* __restrict__ perm, const int64_t* __restrict__ faces, int64_t F, int64_t V,
                                                   int64_t* __restrict__ edges, int32_t* __restrict__ count, int64_t* __restrict__ opp,
                                                   int32_t* __restrict__ locked, int64_t* __restrict__ nkey) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = ukey[e];
    const int64_t s = min(max(offsets[e], (int64_t)0), 3 * F), t = min(max(offsets[e + 1], s), 3 * F);
    const int64_t a = k >= 0 ? k / V : -1, b = k >= 0 ? k - a * V : -1;
    const bool ok = k >= 0 && a < b && b < V;
    const int64_t n = ok ? t - s : 0;
    edges[e * 2] = ok ? a : -1; edges[e * 2 + 1] = ok ? b : -1;
    count[e] = (int32_t)min(n, (int64_t)INT32_MAX);
    opp[e * 2] = n >= 1 ? opposite(faces, F, V, perm[s]) : -1;
    opp[e * 2 + 1] = n >= 2 ? opposite(faces, F, V, perm[s + 1]) : -1;
    nkey[e] = ok ? a * V + b : INT64_MAX;
    nkey[E + e] = ok ? b * V + a : INT64_MAX;
    if (ok && n != 2) { atomicOr(locked + a, 1); atomicOr(locked + b, 1); }
  }
}

// whether the faces at `end` that do not hold `other` keep their side when `end` moves to x: slots[offsets[end] .. offsets[end + 1]) are
// the corners 3 f + c that hold `end`
__device__ bool keeps_normals(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                              const int64_t* __restrict__ slots, const int64_t* __restrict__ offsets, int64_t end, int64_t other,
                              const float x[3], double flip_cos) {
  const int64_t s = max(offsets[end], (int64_t)0), e = min(offsets[end + 1], 3 * F);
  for (int64_t k = s; k < e; ++k) {
    const int64_t h = slots[k];
    if (h < 0 || h >= 3 * F) continue;
    const int64_t f = h / 3, c = h - 3 * f;
    const int64_t i[3] = {faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2]};
    if (!sr_face_ok(i[0], i[1], i[2], V)) continue;
    if (i[0] == other || i[1] == other || i[2] == other) continue;
    double N0[3], N1[3];
    face_normal(verts + i[0] * 3, verts + i[1] * 3, verts + i[2] * 3, N0);
    face_normal(c == 0 ? x : verts + i[0] * 3, c == 1 ? x : verts + i[1] * 3, c == 2 ? x : verts + i[2] * 3, N1);
    const double l0 = sqrt(N0[0] * N0[0] + N0[1] * N0[1] + N0[2] * N0[2]), l1 = sqrt(N1[0] * N1[0] + N1[1] * N1[1] + N1[2] * N1[2]);
    const double dot = N0[0] * N1[0] + N0[1] * N1[1] + N0[2] * N1[2];
    if (!(l1 > 0.) || !(dot > flip_cos * l0 * l1)) return false;
  }
  return true;
}

// thread per edge.  nbr [2E] are the sorted directed keys a V + b: the neighbours of v, ascending, are nbr[noff[v] .. noff[v + 1]) - v V.
__global__ __launch_bounds__(256) void candidates(const float* __restrict__ verts, int64_t V, const int64_t* __restrict__ faces, int64_t F,
                                                   const double* __restrict__ Q, const int64_t* __restrict__ slots, const int64_t* __restrict__ offsets,
                                                   const int64_t* __restrict__ nbr, const int64_t* __restrict__ noff, const int64_t* __restrict__ edges,
                                                   const int32_t* __restrict__ count, const int64_t* __restrict__ opp, const int32_t* __restrict__ locked,
                                                   int64_t E, double reg, double flip_cos, float* __restrict__ pos, int64_t* __restrict__ key) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = edges[e * 2], b = edges[e * 2 + 1];
    if (!sr_edge_ok(a, b, V)) {
      pos[e * 3] = 0.f; pos[e * 3 + 1] = 0.f; pos[e * 3 + 2] = 0.f; key[e] = INT64_MAX;
      continue;
    }
    double q[SR_COLLAPSE_Q];
#pragma unroll
    for (int k = 0; k < SR_COLLAPSE_Q; ++k) q[k] = Q[a * SR_COLLAPSE_Q + k] + Q[b * SR_COLLAPSE_Q + k];
    const double m[3] = {0.5 * ((double)verts[a * 3] + (double)verts[b * 3]), 0.5 * ((double)verts[a * 3 + 1] + (double)verts[b * 3 + 1]),
                         0.5 * ((double)verts[a * 3 + 2] + (double)verts[b * 3 + 2])};
    double xd[3];
    quadric_optimum(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], m, reg, xd);
    const float x[3] = {(float)xd[0], (float)xd[1], (float)xd[2]};          // rounded before the cost and the flip test: what a collapse stores
    pos[e * 3] = x[0]; pos[e * 3 + 1] = x[1]; pos[e * 3 + 2] = x[2];
    const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
    const double value = x0 * (q[0] * x0 + q[1] * x1 + q[2] * x2) + x1 * (q[1] * x0 + q[3] * x1 + q[4] * x2) + x2 * (q[2] * x0 + q[4] * x1 + q[5] * x2)
                         - 2. * (q[6] * x0 + q[7] * x1 + q[8] * x2) + q[9];
    const float cost = (float)(value > 0. ? value : 0.);

    const int64_t o0 = opp[e * 2], o1 = opp[e * 2 + 1];
    bool ok = count[e] == 2 && !locked[a] && !locked[b] && o0 >= 0 && o1 >= 0 && o0 < V && o1 < V && o0 != o1;
    if (ok) {                                                                // valences: both opposite vertices lose one edge, a gains val(b) - 4 + 1
      const int64_t va = noff[a + 1] - noff[a], vb = noff[b + 1] - noff[b];
      ok = va + vb - 4 >= 3 && noff[o0 + 1] - noff[o0] - 1 >= 3 && noff[o1 + 1] - noff[o1] - 1 >= 3;
    }
    if (ok) {                                                                // link condition: a merge of the two ascending neighbour lists
      int64_t i = max(noff[a], (int64_t)0), j = max(noff[b], (int64_t)0), common = 0;
      const int64_t ie = min(noff[a + 1], 2 * E), je = min(noff[b + 1], 2 * E);
      while (i < ie && j < je) {
        const int64_t u = nbr[i] - a * V, w = nbr[j] - b * V;
        if (u == w) { ++common; ++i; ++j; }
        else if (u < w) ++i;
        else ++j;
      }
      ok = common == 2;                                                      // (both opposite vertices are common neighbours: exactly those)
    }
    ok = ok && keeps_normals(verts, V, faces, F, slots, offsets, a, b, x, flip_cos) && keeps_normals(verts, V, faces, F, slots, offsets, b, a, x, flip_cos);
    key[e] = ok ? ((int64_t)__float_as_int(cost) << 32) | (int64_t)fmix32((uint32_t)e) : INT64_MAX;
  }
}

__global__ __launch_bounds__(256) void fill64(int64_t* __restrict__ p, int64_t n, int64_t value) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = value;
}

__global__ __launch_bounds__(256) void min1(const int64_t* __restrict__ edges, const int64_t* __restrict__ key, int64_t E, int64_t V, int64_t* __restrict__ m1) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = edges[e * 2], b = edges[e * 2 + 1], k = key[e];
    if (a < 0 || b < 0 || a >= V || b >= V || k < 0 || k == INT64_MAX) continue;
    atomic_min64(m1 + a, k); atomic_min64(m1 + b, k);
  }
}

// m2 starts as a copy of m1
__global__ __launch_bounds__(256) void min2(const int64_t* __restrict__ edges, int64_t E, int64_t V, const int64_t* __restrict__ m1, int64_t* __restrict__ m2) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = edges[e * 2], b = edges[e * 2 + 1];
    if (a < 0 || b < 0 || a >= V || b >= V) continue;
    const int64_t ka = m1[a], kb = m1[b];
    if (kb >= 0 && kb != INT64_MAX) atomic_min64(m2 + a, kb);
    if (ka >= 0 && ka != INT64_MAX) atomic_min64(m2 + b, ka);
  }
}

// record[0] += selected edges, record[1] += candidates
__global__ __launch_bounds__(256) void select(const int64_t* __restrict__ edges, const int64_t* __restrict__ key, int64_t E, int64_t V,
                                               const int64_t* __restrict__ m2, uint8_t* __restrict__ selected, unsigned long long* __restrict__ record) {
  int32_t ns = 0, nc = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = edges[e * 2], b = edges[e * 2 + 1], k = key[e];
    const bool cand = a >= 0 && b >= 0 && a < V && b < V && k >= 0 && k != INT64_MAX;
    const bool sel = cand && m2[a] == k && m2[b] == k;
    selected[e] = sel ? 1 : 0;
    ns += sel ? 1 : 0; nc += cand ? 1 : 0;
  }
  sr_record_add(record, ns);
  sr_record_add(record + 1, nc);
}

// the selected edges share no endpoint, so every write below has one writer and Q[b] no writer at all
__global__ __launch_bounds__(256) void apply_vertices(const int64_t* __restrict__ edges, const float* __restrict__ pos, const uint8_t* __restrict__ selected,
                                                       int64_t E, float* __restrict__ verts, int64_t V, double* __restrict__ Q, int64_t* __restrict__ target) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    if (!selected[e]) continue;
    const int64_t a = edges[e * 2], b = edges[e * 2 + 1];
    if (!sr_edge_ok(a, b, V)) continue;
    verts[a * 3] = pos[e * 3]; verts[a * 3 + 1] = pos[e * 3 + 1]; verts[a * 3 + 2] = pos[e * 3 + 2];
#pragma unroll
    for (int k = 0; k < SR_COLLAPSE_Q; ++k) Q[a * SR_COLLAPSE_Q + k] += Q[b * SR_COLLAPSE_Q + k];
    target[b] = a;
  }
}

__global__ __launch_bounds__(256) void apply_faces(const int64_t* __restrict__ faces, int64_t F, const int64_t* __restrict__ target, int64_t V,
                                                    int64_t* __restrict__ out_faces, uint8_t* __restrict__ keep) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    int64_t x, y, z;
    sr_face_remap(faces, f, target, V, x, y, z);
    out_faces[f * 3] = x; out_faces[f * 3 + 1] = y; out_faces[f * 3 + 2] = z;
    keep[f] = sr_face_ok(x, y, z, V) && x != y && y != z && x != z ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void map_jump(const int64_t* __restrict__ P, int64_t V, int64_t* __restrict__ N, int32_t* __restrict__ changed) {
  sr_forest_jump(P, V, N, changed);
}
}  // namespace

#define SR_COLLAPSE_MAX_V ((int64_t)1 << 31)          // V V <= 2^62: the edge keys are int64
#define SR_COLLAPSE_MAX_F ((int64_t)1 << 30)          // 3 F < 2^32: the hash takes the edge index as 32 bits

extern "C" int sr_collapse_vertex_quadrics(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* slots, const int64_t* offsets,
                                           double* quadrics, void* stream) {
  if (!verts || !faces || !slots || !offsets || !quadrics || V <= 0 || F <= 0 || V > SR_COLLAPSE_MAX_V || F > SR_COLLAPSE_MAX_F) return SR_EINVAL;
  sr_launch_stream(vertex_quadrics, V, 256, stream, verts, V, faces, F, slots, offsets, quadrics);
  return sr_launch_status();
}

extern "C" int sr_collapse_edge_keys(const int64_t* faces, int64_t F, int64_t V, int64_t* key, void* stream) {
  if (!faces || !key || F <= 0 || V <= 0 || V > SR_COLLAPSE_MAX_V || F > SR_COLLAPSE_MAX_F) return SR_EINVAL;
  sr_launch_stream(edge_keys, 3 * F, 256, stream, faces, F, V, key);
  return sr_launch_status();
}

extern "C" int sr_collapse_edge_heads(const int64_t* unique_key, const int64_t* offsets, int64_t E, const int64_t* perm, const int64_t* faces, int64_t F,
                                      int64_t V, int64_t* edges, int32_t* count, int64_t* opposite, int32_t* locked, int64_t* directed, void* stream) {
  if (!unique_key || !offsets || !perm || !faces || !edges || !count || !opposite || !locked || !directed || E <= 0 || F <= 0 || V <= 0 ||
      V > SR_COLLAPSE_MAX_V || F > SR_COLLAPSE_MAX_F || E > 3 * F)
    return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(locked, 0, (size_t)V * 4, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(edge_heads, E, 256, st, unique_key, offsets, E, perm, faces, F, V, edges, count, opposite, locked, directed);
  return sr_launch_status();
}

extern "C" int sr_collapse_candidates(const float* verts, int64_t V, const int64_t* faces, int64_t F, const double* quadrics, const int64_t* slots,
                                      const int64_t* offsets, const int64_t* neighbours, const int64_t* neighbour_offsets, const int64_t* edges,
                                      const int32_t* count, const int64_t* opposite, const int32_t* locked, int64_t E, double reg, double flip_cos,
                                      float* positions, int64_t* key, void* stream) {
  if (!verts || !faces || !quadrics || !slots || !offsets || !neighbours || !neighbour_offsets || !edges || !count || !opposite || !locked || !positions ||
      !key || V <= 0 || F <= 0 || E <= 0 || V > SR_COLLAPSE_MAX_V || F > SR_COLLAPSE_MAX_F || E > 3 * F || !(reg > 0.) || !(reg < INFINITY) ||
      !(flip_cos >= -1.) || !(flip_cos < 1.))
    return SR_EINVAL;
  sr_launch_stream(candidates, E, 256, stream, verts, V, faces, F, quadrics, slots, offsets, neighbours, neighbour_offsets, edges, count, opposite, locked, E,
                   reg, flip_cos, positions, key);
  return sr_launch_status();
}

extern "C" int sr_collapse_min1(const int64_t* edges, const int64_t* key, int64_t E, int64_t V, int64_t* m1, void* stream) {
  if (!edges || !key || !m1 || E <= 0 || V <= 0) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  sr_launch_stream(fill64, V, 256, st, m1, V, (int64_t)INT64_MAX);
  sr_launch_stream(min1, E, 256, st, edges, key, E, V, m1);
  return sr_launch_status();
}

extern "C" int sr_collapse_min2(const int64_t* edges, int64_t E, int64_t V, const int64_t* m1, int64_t* m2, void* stream) {
  if (!edges || !m1 || !m2 || m1 == m2 || E <= 0 || V <= 0) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(m2, m1, (size_t)V * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(min2, E, 256, st, edges, E, V, m1, m2);
  return sr_launch_status();
}

extern "C" int sr_collapse_select(const int64_t* edges, const int64_t* key, int64_t E, int64_t V, const int64_t* m2, uint8_t* selected, int64_t* record,
                                  void* stream) {
  if (!edges || !key || !m2 || !selected || !record || E <= 0 || V <= 0) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(record, 0, 16, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(select, E, 256, st, edges, key, E, V, m2, selected, (unsigned long long*)record);
  return sr_launch_status();
}

extern "C" int sr_collapse_apply_vertices(const int64_t* edges, const float* positions, const uint8_t* selected, int64_t E, float* verts, int64_t V,
                                          double* quadrics, int64_t* target, void* stream) {
  if (!edges || !positions || !selected || !verts || !quadrics || !target || E <= 0 || V <= 0) return SR_EINVAL;
  sr_launch_stream(apply_vertices, E, 256, stream, edges, positions, selected, E, verts, V, quadrics, target);
  return sr_launch_status();
}

extern "C" int sr_collapse_apply_faces(const int64_t* faces, int64_t F, const int64_t* target, int64_t V, int64_t* out_faces, uint8_t* keep, void* stream) {
  if (!faces || !target || !out_faces || !keep || F <= 0 || V <= 0) return SR_EINVAL;
  sr_launch_stream(apply_faces, F, 256, stream, faces, F, target, V, out_faces, keep);
  return sr_launch_status();
}

extern "C" int sr_collapse_map_jump(const int64_t* parent, int64_t V, int64_t* next, int32_t* changed, void* stream) {
  if (!parent || !next || !changed || parent == next || V <= 0) return SR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(changed, 0, 4, st) != hipSuccess) return SR_ELAUNCH;
  sr_launch_stream(map_jump, V, 256, st, parent, V, next, changed);
  return sr_launch_status();
}
