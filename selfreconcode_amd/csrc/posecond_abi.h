/* Entry points of the pose-conditioning extension (csrc/posecond.hip): declared here, once, in the style of
 * include/selfrecon_hip.h -- plain C99 that _abi.parse reads -- and bound by posecond_ops.py through _lib.bind_header.  The main header
 * and the table read from it are not touched.
 *
 * Conventions as there: every pointer is a device pointer, `stream` is a hipStream_t; 0 = SR_OK, SR_EINVAL for a bad size (a count
 * <= 0, a count >= 2^31, a leading dimension below its count, K outside [1, SR_POSE_MAX_K]) or a null pointer that is not marked
 * optional.
 *
 * A pose feature is SMPL's own pose feature without the root joint: the SR_POSE_FEATS = 23 * 9 entries of R_j - I, joints j = 1 .. 23,
 * row major within a joint.  Features are stored feature-major: entry e of pose n is feat_t[e * ld + n]. */
#ifndef SELFRECON_POSECOND_ABI_H_
#define SELFRECON_POSECOND_ABI_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SR_POSE_JOINTS 23
#define SR_POSE_FEATS 207
#define SR_POSE_MAX_K 8

/* feat_t [207, ld] from theta [N,24,3] (axis-angle): (R_j - I) scale[j - 1], R_j the body model's rodrigues (+1e-8 included); `scale`
 * [23] is optional (null: ones).  Columns n >= N are not written. */
int sr_pose_features(const float* theta, int64_t N, const float* scale, float* feat_t, int64_t ld, void* stream);
/* idx / d2 [Q,K]: the K candidates n < N with the smallest d2(q, n) = sum_e (featq_t[e, q] - feat_t[e, n])^2 (float32, e ascending,
 * fused multiply-add), in ascending (d2, n) order.  With `query_frames` [Q] (optional) and exclude >= 0 the candidates with
 * |n - query_frames[q]| <= exclude are skipped; a candidate with a non-finite d2 is skipped always.  Unfilled slots: idx -1, d2 +inf. */
int sr_pose_neighbors(const float* featq_t, int64_t ldq, int64_t Q, const float* feat_t, int64_t ld, int64_t N, int32_t K,
                      const int32_t* query_frames, int32_t exclude, int32_t* idx, float* d2, void* stream);
/* D [Q,N]: every d2(q, n), by the device function sr_pose_neighbors uses (the witness) */
int sr_pose_dist(const float* featq_t, int64_t ldq, int64_t Q, const float* feat_t, int64_t ld, int64_t N, float* D, void* stream);
/* out [Q,L] = sum_k w_k codes[idx[q,k], l] (k ascending, fused multiply-add) and weights [Q,K] = w: w_k = expf(-(d2_k - d2_0)
 * inv_two_sigma2) over the slots with 0 <= idx < N, 0 for the others, divided by their sum taken in ascending k; d2_0 is the first
 * such slot's.  A row without such a slot gives zeros.  inv_two_sigma2 is finite and >= 0. */
int sr_code_blend(const int32_t* idx, const float* d2, int64_t Q, int32_t K, float inv_two_sigma2, const float* codes, int64_t N, int64_t L,
                  float* out, float* weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif
