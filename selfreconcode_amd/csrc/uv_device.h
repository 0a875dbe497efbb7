// UV triangles and their edge functions in double, shared by the texel map (texture.hip) and the contested-texel count (mesh_prep.hip):
// both must agree on which texel centres a UV triangle contains.
#pragma once
#include "sr_common.h"

namespace {

struct UvTri { double ax, ay, bx, by, cx, cy, area2; bool ok; };

__device__ __forceinline__ UvTri uv_tri(const float* __restrict__ vt, const int64_t* __restrict__ ft, int64_t Vt, int64_t f) {
  UvTri t;
  const int64_t a = ft[f * 3], b = ft[f * 3 + 1], c = ft[f * 3 + 2];
  t.ok = a >= 0 && b >= 0 && c >= 0 && a < Vt && b < Vt && c < Vt;
  if (!t.ok) return t;
  t.ax = vt[a * 2]; t.ay = vt[a * 2 + 1]; t.bx = vt[b * 2]; t.by = vt[b * 2 + 1]; t.cx = vt[c * 2]; t.cy = vt[c * 2 + 1];
  t.area2 = (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax);
  t.ok = fabs(t.area2) > 1e-14;                 // degenerate (or NaN): owns nothing
  return t;
}

// edge functions of (u, v): e0 + e1 + e2 = area2, barycentric k = e_k / area2
__device__ __forceinline__ void uv_edges(const UvTri& t, double u, double v, double& e0, double& e1, double& e2) {
  e0 = (t.cx - t.bx) * (v - t.by) - (t.cy - t.by) * (u - t.bx);
  e1 = (t.ax - t.cx) * (v - t.cy) - (t.ay - t.cy) * (u - t.cx);
  e2 = (t.bx - t.ax) * (v - t.ay) - (t.by - t.ay) * (u - t.ax);
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

}  // namespace
