/* Entry points of the skin fit (csrc/skinfit.hip): declared here, once, in the style of include/selfrecon_hip.h --
 * plain C99 that _abi.parse reads -- and bound by skinfit_ops.py through _lib.bind_header.  The main header and the table read from it
 * are not touched.
 *
 * Conventions as there: every pointer is a device pointer, `stream` is a hipStream_t; 0 = SR_OK, SR_EINVAL for a bad size (a count
 * <= 0, a count >= 2^31, C outside [1, SR_SKINFIT_MAX_CANDS], K outside [1, C]), a `reg` or `lambda_floor` that is not finite, a
 * negative `reg`, a `lambda_floor` that is not positive, or a null pointer that is not marked optional.
 *
 * A vertex has C candidate joints cands[v, 0 .. C-1].  Its normal matrix H is symmetric C x C and is stored as its lower triangle,
 * entry-major: entry e = k (k + 1) / 2 + l (l <= k) of vertex v is H[e * V + v]; there are SR_SKINFIT_TRI rows whatever C is, and the
 * rows past C (C + 1) / 2 are neither read nor written. */
#ifndef SELFRECON_SKINFIT_ABI_H_
#define SELFRECON_SKINFIT_ABI_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SR_SKINFIT_MAX_CANDS 8
#define SR_SKINFIT_TRI 36
#define SR_SKINFIT_JOINTS 24
#define SR_SKINFIT_SLAB 16

/* H += sum_t D_t^T D_t over the T frames of a batch, in double: row k of D_t (a 3-vector) is
 *   d_tk = A[t, cands[v,k]] [q[t,v]; 1] - (y[t,v] - trans[t]),
 * q, y [T,V,3], A [T,24,12] (the top three rows of the posed transforms, row major), trans [T,3], cands [V,C] with entries in
 * [0, 24) (others are clamped).  Every float is widened first; a row of A [q; 1] is summed x, y, z, then the translation; an entry of
 * D^T D x, y, z.  The frames go through the LDS in slabs of SR_SKINFIT_SLAB; wave w of a workgroup takes the frames w, w + 8, ... of a
 * slab in ascending order and the waves' partial sums are added in ascending w, then to H.  No atomics: two calls give equal bits. */
int sr_skinfit_accumulate(const float* q, const float* y, const float* A, const float* trans, int64_t T, int64_t V, const int32_t* cands,
                          int32_t C, double* H, void* stream);
/* Per vertex the minimiser of x^T H x + lambda |x - xbar|^2 over x >= 0, sum x = 1 with at most K non-zeros, lambda =
 * reg trace(H) / C + lambda_floor, by enumeration: every support (bit mask over the C candidates, ascending) of at most K
 * candidates, the equality-constrained minimiser on it by Cholesky, rejected when an entry is negative; the lowest objective wins, a
 * tie goes to the smaller support, then to the lower mask.  xbar [C,V] double, entry-major.  Outputs: joints / weights [V,K] -- the
 * chosen candidates' joints in ascending candidate order with float32 weights whose sum is 1 (the largest takes the rounding
 * residue), unused slots joint 0, weight 0 --, objective [V], mask [V] (optional), lambda [V] (optional).  A vertex whose H or xbar
 * is not finite gets no search: the K largest xbar (ties: the lower candidate) renormalised, and a NaN objective. */
int sr_skinfit_solve(const double* H, const double* xbar, const int32_t* cands, int64_t V, int32_t C, int32_t K, double reg,
                     double lambda_floor, int32_t* joints, float* weights, double* objective, int32_t* mask, double* lambda, void* stream);

#ifdef __cplusplus
}
#endif
#endif
