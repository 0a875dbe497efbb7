/* Entry points of the winding-number extension (csrc/winding.hip): declared here, once, in the style of
 * include/selfrecon_hip.h -- plain C99 that _abi.parse reads -- and bound by winding_ops.py through _lib.bind_header.  The main header
 * and the table read from it are not touched.
 *
 * Conventions as there: every pointer is a device pointer, `stream` is a hipStream_t; 0 = SR_OK, SR_EINVAL for a bad size, a null
 * pointer, a level outside [0, SR_WINDING_MAX_LEVELS] or a `tri` / `nodes` that is not 16-byte aligned.
 *
 * The tree is a dense octree pyramid over the cube [lo, lo + 2^levels cell)^3: level l holds 8^l nodes in Morton order (bit 3 b + a
 * of the index is bit b of the cell coordinate on axis a), at offset (8^l - 1) / 7, so the children of node m of level l are nodes
 * 8 m .. 8 m + 7 of level l + 1.  A node is SR_WINDING_NODE_FLOATS floats: the area vector N, the area-weighted centroid c, the area
 * A and the radius r.  `leaf_start` [8^levels + 1] / `leaf_faces` [F] list every leaf's faces in ascending index. */
#ifndef SELFRECON_WINDING_ABI_H_
#define SELFRECON_WINDING_ABI_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SR_WINDING_MAX_LEVELS 7
#define SR_WINDING_NODE_FLOATS 8

/* key [n] = the Morton index of the leaf that holds row i of `src`: a point [n,3] (faces = 0) or the float32 centroid
 * ((a + b) + c) / 3 of a packed triangle [n,12] (faces = 1).  Coordinates are clamped into the cube. */
int sr_winding_keys(const float* src, int64_t n, int32_t faces, const float* lo, float cell, int32_t levels, int64_t* key, void* stream);
/* the nodes of the leaf level from each leaf's run of faces, summed in ascending face order in double */
int sr_winding_leaves(const float* tri, int64_t F, const int64_t* leaf_start, const int32_t* leaf_faces, int32_t levels, float* nodes,
                      void* stream);
/* the nodes of `level` (< levels) from their eight children each, in child order, in double */
int sr_winding_fold(float* nodes, int32_t level, int32_t levels, void* stream);
/* w [P]: depth first from the root; a node with |p - c| > beta r is taken as one dipole, a leaf otherwise as its faces.  open_all != 0
 * accepts no node (beta = inf).  NaN for a non-finite point. */
int sr_winding_query(const float* points, int64_t P, const float* tri, int64_t F, const float* nodes, int32_t levels,
                     const int64_t* leaf_start, const int32_t* leaf_faces, float beta, int32_t open_all, float* w, void* stream);
/* w [P]: the exact sum over all faces in ascending index */
int sr_winding_brute(const float* points, int64_t P, const float* tri, int64_t F, float* w, void* stream);

#ifdef __cplusplus
}
#endif
#endif
