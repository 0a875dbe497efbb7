// Device functions shared by the quadric placement of the vertex clustering (mesh_prep.hip) and the edge-collapse decimation
// (mesh_collapse.hip): the face normal, the plane quadric of a face that both sum, and the regularised 3 x 3 solve.
#pragma once
#include "sr_common.h"

// n = (b - a) x (c - a) in double from float32 corners with every product and every difference rounded on its own (no contraction: a
// fused a b - round(c d) would turn the exact zero of a degenerate face into a rounding error, and a numpy restatement into a stranger)
static __device__ __forceinline__ void face_normal(const float* __restrict__ pa, const float* __restrict__ pb, const float* __restrict__ pc, double n[3]) {
#pragma clang fp contract(off)                      // (plain operators under this pragma: __dmul_rn / __dsub_rn are inline functions that contract)
  const double ux = (double)pb[0] - (double)pa[0], uy = (double)pb[1] - (double)pa[1], uz = (double)pb[2] - (double)pa[2];
  const double vx = (double)pc[0] - (double)pa[0], vy = (double)pc[1] - (double)pa[1], vz = (double)pc[2] - (double)pa[2];
  const double yz = uy * vz, zy = uz * vy, zx = uz * vx, xz = ux * vz, xy = ux * vy, yx = uy * vx;
  n[0] = yz - zy; n[1] = zx - xz; n[2] = xy - yx;
}

// The area-weighted plane quadric of the face (pa, pb, pc), as the factors of its terms: n the unit normal, w = area, d = n . pa, and
// w0 w1 w2 wd = w (n0 n1 n2 d).  The quadric is A = w n n^T (xx = w0 n0, xy = w0 n1, xz = w0 n2, yy = w1 n1, yz = w1 n2, zz = w2 n2),
// b = w d n (wd n0, wd n1, wd n2) and c = w d^2 (wd d).  The caller forms each product inside its own `+=`, so that the compiler
// contracts product and sum as it did when every kernel spelled this out.  false for a face without area or with a non-finite one.
struct PlaneQuadric { double n0, n1, n2, d, w0, w1, w2, wd; };
static __device__ __forceinline__ bool plane_quadric(const float* __restrict__ pa, const float* __restrict__ pb, const float* __restrict__ pc, PlaneQuadric& p) {
  double N[3];
  face_normal(pa, pb, pc, N);
  const double L = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
  if (!(L > 0.) || !isfinite(L)) return false;
  const double w = 0.5 * L;
  p.n0 = N[0] / L; p.n1 = N[1] / L; p.n2 = N[2] / L;
  p.d = p.n0 * (double)pa[0] + p.n1 * (double)pa[1] + p.n2 * (double)pa[2];
  p.w0 = w * p.n0; p.w1 = w * p.n1; p.w2 = w * p.n2; p.wd = w * p.d;
  return true;
}

// x = m + (A + lam I)^-1 (b - A m), lam = reg trace(A) / 3, for the symmetric A = (xx xy xz; xy yy yz; xz yz zz), by Cholesky: the
// pivots are at least lam.  false, and x = m, when lam > 0 does not hold or the result is not finite.
static __device__ __forceinline__ bool quadric_optimum(double xx, double xy, double xz, double yy, double yz, double zz, double bx, double by, double bz,
                                                const double m[3], double reg, double x[3]) {
  x[0] = m[0]; x[1] = m[1]; x[2] = m[2];
  const double lam = reg * (xx + yy + zz) / 3.;
  if (!(lam > 0.)) return false;
  const double r0 = bx - (xx * m[0] + xy * m[1] + xz * m[2]), r1 = by - (xy * m[0] + yy * m[1] + yz * m[2]),
               r2 = bz - (xz * m[0] + yz * m[1] + zz * m[2]);
  const double g00 = sqrt(xx + lam), g10 = xy / g00, g20 = xz / g00;
  const double g11 = sqrt(yy + lam - g10 * g10), g21 = (yz - g20 * g10) / g11;
  const double g22 = sqrt(zz + lam - g20 * g20 - g21 * g21);
  const double t0 = r0 / g00, t1 = (r1 - g10 * t0) / g11, t2 = (r2 - g20 * t0 - g21 * t1) / g22;
  const double y2 = t2 / g22, y1 = (t1 - g21 * y2) / g11, y0 = (t0 - g10 * y1 - g20 * y2) / g00;
  x[0] += y0; x[1] += y1; x[2] += y2;
  if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) { x[0] = m[0]; x[1] = m[1]; x[2] = m[2]; return false; }
  return true;
}
