/* selfrecon_hip.h -- flat C ABI of libselfrecon_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of the SelfRecon per-frame SDF-optimisation hot path: every entry
 * point replaces one pybind/CUDA surface of the reference (cited per function, paths
 * relative to the reference repository).  Conventions, all functions:
 *   - return 0 on success, a negative SR_E* code otherwise; nothing is allocated inside;
 *     the caller owns every buffer; all pointers are DEVICE pointers unless named host_*;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are
 *     asynchronous and re-entrant per stream; no global mutable state except explicit
 *     workspaces passed by the caller;
 *   - tensors are dense row-major unless strides are passed explicitly (in ELEMENTS).
 * The Python host (selfreconcode_amd/) maps non-zero codes to the reference's own error
 * convention (exception; empty list for mc_gpu -- MCGpu/MCGpu.cpp:41-48).
 */
#ifndef SELFRECON_HIP_H_
#define SELFRECON_HIP_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_OK 0
#define SR_EINVAL (-1)   /* bad argument (null pointer, non-positive size, unsupported mode) */
#define SR_ELAUNCH (-2)  /* hipGetLastError() after launch != hipSuccess */
#define SR_ENOSPC (-3)   /* caller-provided workspace / output capacity too small */

int sr_abi_version(void);            /* bumps when a signature below changes */
const char* sr_build_arch(void);     /* "gfx950" */
const char* sr_build_digest(void);   /* sha256 of the sources the library was built from (selfreconcode_amd/build.py) */

/* ---------------------------------------------------------------- FastMinv (a7)
 * Replaces FastMinv/M3x3Inv.cpp:12-38 Fast3x3Minv -> Matrix3x3InvKernels.cu:22-61 and
 * M3x3Inv.cpp:40-58 Fast3x3Minv_backward -> Matrix3x3InvKernels.cu:64-104.
 * ms/invs/grads/outs: [n,3,3]; checks: [n] bytes (0/1).  Singular rule: |det| < 1e-4
 * -> inverse = 0, check = 0.  backward: out = -(C^T G C^T), C = saved inverse. */
int sr_minv3x3_fwd_f32(const float* ms, float* invs, uint8_t* checks, int64_t n, void* stream);
int sr_minv3x3_fwd_f64(const double* ms, double* invs, uint8_t* checks, int64_t n, void* stream);
int sr_minv3x3_bwd_f32(const float* grads, const float* invs, float* outs, int64_t n, void* stream);
int sr_minv3x3_bwd_f64(const double* grads, const double* invs, double* outs, int64_t n, void* stream);

/* ---------------------------------------------------------------- GridSamplerMine (a6)
 * Replaces MCAcc/cuda/GridSamplerMine.cpp:73-104 (forward / backward / dbackward) ->
 * GridSamplerMineKernel.cu:162-328, 333-570, 575-914.  Trilinear, border padding,
 * align_corners=False only (the only mode the reference accepts, GridSamplerMine.cpp:59-64).
 * A tensor is described by its 5 sizes / strides in elements: input [N,C,D,H,W];
 * grid [N,Do,Ho,Wo,3]; output-like tensors [N,C,Do,Ho,Wo].  grad_grid is dense [N,Do,Ho,Wo,3]
 * (the reference assumes the same, Kernel.cu:538-545).  grad_input may be NULL (skip it: the
 * skinning-weight volume is a buffer) -- when given it must be ZERO-FILLED by the caller and has
 * the input's sizes with its own strides. */
typedef struct {
  int64_t size[5];
  int64_t stride[5];
} sr_tensor5;

int sr_gridsample3d_fwd_f32(const float* input, sr_tensor5 in_d, const float* grid, sr_tensor5 grid_d,
                            float* output, sr_tensor5 out_d, void* stream);
int sr_gridsample3d_fwd_f64(const double* input, sr_tensor5 in_d, const double* grid, sr_tensor5 grid_d,
                            double* output, sr_tensor5 out_d, void* stream);
int sr_gridsample3d_bwd_f32(const float* input, sr_tensor5 in_d, const float* grid, sr_tensor5 grid_d,
                            const float* grad_output, sr_tensor5 gout_d,
                            float* grad_input /*nullable*/, sr_tensor5 gin_d, float* grad_grid, void* stream);
int sr_gridsample3d_bwd_f64(const double* input, sr_tensor5 in_d, const double* grid, sr_tensor5 grid_d,
                            const double* grad_output, sr_tensor5 gout_d,
                            double* grad_input /*nullable*/, sr_tensor5 gin_d, double* grad_grid, void* stream);
/* fp16 (IEEE binary16 storage, `void*` here; the reference dispatches AT_DISPATCH_FLOATING_TYPES_AND_HALF at
 * GridSamplerMineKernel.cu:931,963,1001): same kernels on the native half type, every arithmetic step rounded to half as
 * at::Half arithmetic is; grad_input accumulates with a 16-bit CAS add. */
int sr_gridsample3d_fwd_f16(const void* input, sr_tensor5 in_d, const void* grid, sr_tensor5 grid_d, void* output, sr_tensor5 out_d,
                            void* stream);
int sr_gridsample3d_bwd_f16(const void* input, sr_tensor5 in_d, const void* grid, sr_tensor5 grid_d, const void* grad_output,
                            sr_tensor5 gout_d, void* grad_input /*nullable*/, sr_tensor5 gin_d, void* grad_grid, void* stream);
int sr_gridsample3d_dbwd_f16(const void* gO_input /*nullable*/, sr_tensor5 goi_d, const void* gO_grid, sr_tensor5 gog_d,
                             const void* input, sr_tensor5 in_d, const void* grid, sr_tensor5 grid_d, const void* grad_output,
                             sr_tensor5 gout_d, void* grad_input /*nullable*/, sr_tensor5 gin_d, void* grad_grid,
                             void* grad_grad_output, void* stream);
/* double backward: cotangents (gO_input [like input] nullable = zeros, gO_grid [N,Do,Ho,Wo,3]
 * with strides) of the backward's two outputs -> grad_input (nullable, zero-filled by caller),
 * grad_grid (dense), grad_grad_output (dense [N,C,Do,Ho,Wo]). */
int sr_gridsample3d_dbwd_f32(const float* gO_input /*nullable*/, sr_tensor5 goi_d, const float* gO_grid, sr_tensor5 gog_d,
                             const float* input, sr_tensor5 in_d, const float* grid, sr_tensor5 grid_d,
                             const float* grad_output, sr_tensor5 gout_d,
                             float* grad_input /*nullable*/, sr_tensor5 gin_d, float* grad_grid, float* grad_grad_output,
                             void* stream);
int sr_gridsample3d_dbwd_f64(const double* gO_input /*nullable*/, sr_tensor5 goi_d, const double* gO_grid, sr_tensor5 gog_d,
                             const double* input, sr_tensor5 in_d, const double* grid, sr_tensor5 grid_d,
                             const double* grad_output, sr_tensor5 gout_d,
                             double* grad_input /*nullable*/, sr_tensor5 gin_d, double* grad_grid, double* grad_grad_output,
                             void* stream);


/* ---------------------------------------------------------------- MLP layer kernels (a2, a3, a4, a10)
 * Replace the per-layer nn.Linear (cuBLAS) + activation + torch.cat launches of
 * model/network.py:83-95 (ImplicitNetwork.forward), model/Deformer.py:66-71 (MLPTranslator),
 * model/RenderNet.py:80-88, and their autograd backward / double-backward passes
 * (network.py:102-114, utils/utils.py:106-120).  Exact fp32 on the MFMA pipe
 * (v_mfma_f32_32x32x2_f32); rows are "tangent-interleaved": each sample owns `group` (1, 2 or 4)
 * consecutive rows = primal + forward-mode tangents.
 *
 * sr_mlp_gemm_nt:  C[M, N(+naux_fwd)] = epilogue( A[M,K] * B[N,K]^T )
 *   SR_EPI_FWD : primal rows  c = act(acc + bias) * out_scale
 *                tangent rows c = act'(primal pre-activation) * acc * out_scale
 *                columns [N, N+naux_fwd) = aux[:, 0:naux_fwd] * out_scale       (skip concat, network.py:88-89)
 *   SR_EPI_BWD : acc is the cotangent of the STORED activations `aux` (= aux_scale * act(z), same row layout)
 *                columns < nact_bwd: primal  c = act' * aux_scale * acc + (act''/act') * sum_t aux_t * acc_t
 *                                    tangent c = act' * aux_scale * acc
 *                columns >= nact_bwd: c = acc * out_scale                       (cotangent of the skip filler)
 * Requirements: lda, ldb multiples of 4 floats and A, B 16-byte aligned; M % group == 0. */
#define SR_ACT_NONE 0
#define SR_ACT_SOFTPLUS100 1   /* torch.nn.Softplus(beta=100, threshold=20), network.py:70 */
#define SR_ACT_RELU 2
#define SR_EPI_FWD 0
#define SR_EPI_BWD 1
typedef struct {
  const float* A; int64_t lda;
  const float* B; int64_t ldb;
  float* C; int64_t ldc;
  int32_t M, N, K;
  const float* bias;      /* [N] or NULL; primal rows only */
  int32_t group, act, mode;
  float out_scale;
  const float* aux; int64_t ldaux;
  int32_t naux_fwd;       /* FWD: number of filler columns appended after N */
  int32_t nact_bwd;       /* BWD: leading columns that go through the activation derivative */
  float aux_scale;        /* BWD: scale the stored activations carry */
} sr_gemm_args;
int sr_mlp_gemm_nt(const sr_gemm_args* host_args, void* stream);
/* Tile shape (rows x columns of C per workgroup) sr_mlp_gemm_nt launches for M rows and ncols = N (+ naux_fwd in SR_EPI_FWD) output
 * columns: one of 32x32, 64x32, 256x32 (ncols <= 32), 64x64, 64x128, 128x128.  Host only, needs no device.  A tile takes the
 * straight-line epilogue when it lies inside the M rows and inside the first N (SR_EPI_FWD) / min(N, nact_bwd) (SR_EPI_BWD) columns. */
int sr_mlp_gemm_nt_tile(int32_t M, int32_t ncols, int32_t* bm_out, int32_t* bn_out);

/* Layer chain: up to SR_CHAIN_MAX_LAYERS consecutive layer GEMMs of one or two independent networks (layer l of both side
 * by side in one grid) on a row count read from DEVICE memory: rows = *m_dev * m_mul <= m_cap * m_mul (every g[l][p].M is
 * ignored; g[l][p].group must equal m_mul).  g[l+1][p].A may be g[l][p].C.  One launch per layer, grids sized for m_cap,
 * workgroups beyond the live tiles return at once; no host synchronisation.
 * This is the MLP half of the reference's utils/FindSurfacePs.py:129-162 loop body on whatever number of rays is still
 * unfinished, without the host ever learning that number. */
#define SR_CHAIN_MAX_LAYERS 10
typedef struct {
  int32_t nlayers;
  int32_t nprob[SR_CHAIN_MAX_LAYERS];
  sr_gemm_args g[SR_CHAIN_MAX_LAYERS][2];
  const int32_t* m_dev; int32_t m_mul;
  int32_t m_cap;                   /* upper bound of *m_dev (sizes the grids) */
} sr_chain_args;
int sr_mlp_chain(const sr_chain_args* host_args, void* stream);

/* Weight gradient: dW[N, lddw] (+)= sum_r Z[r, 0:N]^T A[r, 0:K], all rows (primal and tangent).
 * Split over r into `splits` slabs in `partial` (>= splits*N*lddw floats, see _workspace_floats),
 * reduced in a fixed order (deterministic).  accumulate != 0 adds into dW.  lddw % 4 == 0, dW and partial 16-byte aligned
 * (the reduction moves float4); columns [K, lddw) of dW are written as 0. */
typedef struct {
  const float* Z; int64_t ldz;
  const float* A; int64_t lda;
  float* dW; int64_t lddw;
  float* partial;
  int32_t R, N, K, splits, accumulate;
  /* optional fused bias gradient: db[n] = sum over primal rows (r % group == 0) of Z[r][n];
   * db_partial: workspace of splits*N floats.  Both NULL to skip. */
  float* db; float* db_partial; int32_t group;
} sr_gemm_tn_args;
int64_t sr_mlp_gemm_tn_workspace_floats(int32_t R, int32_t N, int64_t lddw, int32_t* host_splits_out);
int sr_mlp_gemm_tn(const sr_gemm_tn_args* host_args, void* stream);
/* Up to SR_TN_GROUP_MAX independent weight gradients of the general tile shape (not the K <= 64 & N >= 256 first-layer shape) in ONE
 * launch + one launch for their slab reductions: the reverse sweep of a network on a few thousand rows (the ray branch, the
 * implicit-gradient pass: network.py:599-639, 702-814) leaves one weight gradient per layer, each too small to fill the machine.
 * Every problem is computed exactly as sr_mlp_gemm_tn would compute it alone (same tiles, same slabs, same reduction order: bit-identical);
 * no two problems of a call may share dW / db / partial. */
#define SR_TN_GROUP_MAX 12
typedef struct {
  int32_t n;
  sr_gemm_tn_args p[SR_TN_GROUP_MAX];
} sr_gemm_tn_group_args;
int sr_mlp_gemm_tn_group(const sr_gemm_tn_group_args* host_args, void* stream);

/* Positional encoding (a1) fused with the first-layer input assembly: replaces the 13 elementwise
 * launches + torch.cat of model/Embedder.py:34-41 and the conds[batch_inds] concat of
 * model/Deformer.py:58-61.  out[p*group, :] = [x | w sin/cos bands | extra[extra_index[p] or p] | 0];
 * group == 4 also writes the three d/dx_t seed-tangent rows.  band_weights: 2*L floats (device). */
int sr_pe_embed(const float* x, int64_t P, int32_t L, const float* band_weights, const float* extra, int64_t ldextra,
                int32_t E, const int64_t* extra_index /*nullable*/, int32_t group, float* out, int64_t ldo, void* stream);
/* Reverse of sr_pe_embed w.r.t. x: gA0 = cotangent of the embed rows (same row layout, pitch ldg) -> xbar [P,3].
 * Covers the second-derivative term of the group-4 seed-tangent rows. */
int sr_pe_embed_bwd(const float* x, int64_t P, int32_t L, const float* band_weights, int32_t group, const float* gA0,
                    int64_t ldg, float* xbar, void* stream);

/* ---------------------------------------------------------------- fused LBS (a5, a8/a9 LBS part)
 * Replaces, for the no-autograd callers (ray refiner, inference), LBSkinner.forward's
 * GridSamplerMine.forward + per-frame blend loop (model/Deformer.py:207-233) and, when `jac` is
 * given, the three reverse passes of utils/utils.py:106-120 for the LBS factor of dd/dp.
 * vol: skinning weights, channel-last [D,H,W,24] fp32, 16-byte aligned.  A: posed joint transforms
 * (already times init_pose^-1) as [nframes,24,3,4] row-major.  Frame of point i = batch_inds[i], or
 * i / points_per_frame when batch_inds == NULL.  tp (nullable): points used for the weight lookup when
 * they differ from p (Deformer.py:168-171); jac requires tp == NULL. */
typedef struct {
  const float* p; const float* tp; int64_t P;
  const float* A; const float* trans; int32_t nframes;
  const int64_t* batch_inds; int64_t points_per_frame;
  const float* vol; int32_t D, H, W;
  float bmin[3], bmax[3];
  float* y;        /* [P,3] */
  float* jac;      /* [P,3,3] dy/dp, nullable */
} sr_lbs_args;
int sr_lbs_fwd(const sr_lbs_args* host_args, void* stream);
/* Reverse sweep of sr_lbs_fwd for a cotangent ybar [P,3] (replaces the autograd backward of the K3/K4 sampler +
 * per-frame blend, model/Deformer.py:207-233): pbar = (dy/dp)^T ybar, Abar [nframes,24,12] = sum w_j ybar (x) [p;1],
 * transbar [nframes,3] = sum ybar.  Abar / transbar are WRITTEN (no zero fill); each output is nullable.  The per-frame sums are
 * deterministic (segmented wave reductions, per-workgroup partials in `partials`, folded in double precision in a fixed order):
 * bit-reproducible run to run.  `partials`: sr_lbs_bwd_workspace_floats(P, nframes) floats of scratch. */
int64_t sr_lbs_bwd_workspace_floats(int64_t P, int32_t nframes);
int sr_lbs_bwd(const sr_lbs_args* host_args, const float* ybar, float* pbar, float* Abar, float* transbar, float* partials, void* stream);
/* Reverse sweep of sr_lbs_fwd WITH its Jacobian output: cotangents ybar [P,3] (nullable) and Jbar [P,3,3] of (y, jac) ->
 * pbar (includes the mixed second derivatives of the trilinear sampler), Abar, transbar (written as in sr_lbs_bwd; same scratch).
 * Backward of the value + Jacobian form of the deformer that replaces compute_Jacobian's three reverse passes with
 * create_graph (utils/utils.py:106-120) in the colour / normal branch and in propagateTmpPsGrad. */
int sr_lbs_jac_bwd(const sr_lbs_args* host_args, const float* ybar, const float* Jbar, float* pbar, float* Abar, float* transbar, float* partials,
                   void* stream);

/* SMPL kinematic chain of LBSkinner.forward / posedSkeleton (model/Deformer.py:144-203, smpl_pytorch/util.py:35-78):
 * poses [B,24,3] axis-angle (device) -> G [B,24,4,4] posed chain and A = G * init_pose [B,24,4,4].
 * Js [24,3], parents [24] (parents[i] < i), init_pose [24,4,4] are HOST arrays (passed by value to the kernel).
 * _bwd: posebar [B,24,3] from the cotangents Abar and/or Gbar (nullable). */
int sr_lbs_chain_fwd(const float* poses, int32_t B, const float* host_Js, const int32_t* host_parents, const float* host_init_pose,
                     float* G, float* A, void* stream);
int sr_lbs_chain_bwd(const float* poses, int32_t B, const float* host_Js, const int32_t* host_parents, const float* host_init_pose,
                     const float* Abar, const float* Gbar, float* posebar, void* stream);

/* ---------------------------------------------------------------- ray/surface refiner step (a12)
 * One iteration body of utils/FindSurfacePs.py::OptimizeSurfacePs (:115-126 check, :135-151 step)
 * for M live rays.  sdf4: output rows of the sdf-only SDF MLP, `group` rows per ray (row 0 = f,
 * rows 1..3 = df/dp_t), pitch ld_sdf.  off4: output rows of the deformation MLP (row 0 = offset,
 * rows 1..3 = d offset / d p_t), pitch ld_off.  y / jlbs: LBS output d(p) and dLBS/dq from sr_lbs_fwd.
 * converged[i] = |f| < dthreshold && asin(|(d-c) x v| / |d-c|) * 180/pi < athreshold.
 * group == 4 and p_out != NULL: p_out = converged ? p : p - L g / |g|^2.  group == 1: check only. */
typedef struct {
  int64_t M; int32_t group;
  const float* sdf4; int64_t ld_sdf;
  const float* off4; int64_t ld_off;
  const float* y; const float* jlbs;
  const float* rays; const float* cam;   /* [M,3], [3] (device) */
  const float* p; float* p_out;          /* [M,3] */
  uint8_t* converged;                    /* [M] */
  float dthreshold, athreshold, w1, w2;
} sr_newton_args;
int sr_newton_update(const sr_newton_args* host_args, void* stream);

/* Reverse-mode form of the same refiner step (utils/FindSurfacePs.py:135-151): `sr_newton_prepare` tests convergence and
 * emits t = J_lbs^T (d sin-angle / d y) as the cotangent rows of the deformation offset ([M, ld_t], columns >= 3 zeroed;
 * t_out == NULL: convergence test only); after the two reverse sweeps `sr_newton_apply` forms
 * g = w1 sign(f) grad_f + w2 (t + grad_off) and steps the unconverged points. */
typedef struct {
  int64_t M;
  const float* sdf; int64_t ld_sdf;      /* f = sdf[i*ld_sdf] */
  const float* y; const float* jlbs;     /* LBS output [M,3] and dLBS/dq [M,3,3] */
  const float* rays; const float* cam;
  uint8_t* converged;                    /* [M] written by prepare, read by apply */
  float* t_out; int64_t ld_t; float* s_out;
  const float* grad_f; const float* grad_off;   /* [M,3] each (apply) */
  const float* p; float* p_out;          /* (apply) */
  float dthreshold, athreshold, w1, w2;
} sr_newton2_args;
int sr_newton_prepare(const sr_newton2_args* host_args, void* stream);
int sr_newton_apply(const sr_newton2_args* host_args, void* stream);

/* ---------------------------------------------------------------- device-driven refiner (a12; the `sr_trace_newton` of SURVEY 8(b))
 * The whole of utils/FindSurfacePs.py::OptimizeSurfacePs (:114-163) for P rays as a fixed sequence of launches whose row
 * count lives in device memory: `live[k]` = unfinished rays entering phase k (live[0] = P).  The queue of unfinished rays
 * (x, v, frame, orig: two copies, phase parity selects) is compacted by wave ballots at the end of every phase, so finished
 * rays leave the layer GEMMs immediately and the host never learns a count.  After sr_refine_init the caller issues per phase
 *   sr_mlp_chain(forward, m_dev = live + k) -> sr_refine_mid
 *   [-> sr_mlp_chain(reverse) -> sr_refine_finish   for the update phases 1..times]
 * The kernels that put rays into a queue (_init: phase 0; _mid mode 0: phase 1; _finish of phase k: phase k + 1) also write those
 * rays' first-layer input rows a0 / a0d when both pointers are given; sr_refine_embed(phase) writes the same rows for the queue
 * of `phase` as a launch of its own (same arithmetic, same bits; needed only by a caller that passes a0 = a0d = NULL to the others).
 * phase 0 (mid mode 0): initial test; phases 1..times (mode 1): test of the current points + Newton update of the failing
 * ones; phase times+1 (mode 2): test of the last update.  p_out / conv_out are indexed by the rays' original position.
 * The layer chains read a0 / a0d (first-layer inputs) and leave f in sdf_out[:,0], the deformation
 * offset in def_out[:,0:3]; the reverse chains start from `unit` rows (1,0,0,0) (SDF) and `t` rows (deformer) and leave
 * the input cotangents in a0bar (+ skipbar: the skip-concat part, n_skip columns) and a0dbar. */
typedef struct {
  int32_t P, times;
  const float* p0; const float* rays; const int64_t* batch_inds;   /* [P,3], [P,3], [P] inputs (read by _init) */
  const float* cam;                                                /* [3] camera centre (device) */
  int32_t L_sdf; const float* w_sdf; int32_t L_def; const float* w_def;   /* PE bands + per-band weights (2L floats each) */
  const float* conds; int64_t ld_conds; int32_t E;                 /* per-frame deformation codes [nframes, E] */
  const float* A; const float* trans; int32_t nframes;             /* posed transforms [nframes,24,12], translations [nframes,3] */
  const float* vol; int32_t D, H, W; float bmin[3], bmax[3];       /* channel-last skinning-weight volume + its box */
  float dthreshold, athreshold, w1, w2;
  int32_t* live;                                                   /* [times + 3] */
  float* x[2]; float* v[2]; int32_t* frame[2]; int32_t* orig[2];   /* the queue: [P,3], [P,3], [P], [P] each */
  float* unit;                                                     /* [P,4] rows (1,0,0,0), written by _init */
  float* a0; int64_t ld_a0; float* a0d; int64_t ld_a0d;
  const float* sdf_out; int64_t ld_sdf; const float* def_out; int64_t ld_def;
  uint8_t* conv; float* t; float* s;                               /* [P], [P,4], [P] */
  const float* a0bar; int64_t ld_a0bar; const float* skipbar; int64_t ld_skipbar; int32_t n_skip;
  const float* a0dbar; int64_t ld_a0dbar;
  float* p_out; uint8_t* conv_out;                                 /* [P,3], [P] */
} sr_refine_args;
int sr_refine_init(const sr_refine_args* host_args, void* stream);
int sr_refine_embed(const sr_refine_args* host_args, int32_t phase, void* stream);
int sr_refine_mid(const sr_refine_args* host_args, int32_t phase, int32_t mode, void* stream);
int sr_refine_finish(const sr_refine_args* host_args, int32_t phase, void* stream);


/* ---------------------------------------------------------------- MCGpu (a17)
 * Replaces MCGpu/MCGpu.cpp:20-56 mc_gpu -> MCGpu::init/MC/scaleVertices (CudaKernels.cu:524-639) and
 * kernels K6-K9.  Two calls because the output sizes are data dependent (the reference also copies
 * its two counters to the host between K6 and K7, CudaKernels.cu:628):
 *   sr_mc_count : classify + exclusive scans into `workspace` (sr_mc_workspace_bytes);
 *                 counts_dev[0] = #vertices, counts_dev[1] = #faces (2 x uint32, device memory)
 *   sr_mc_emit  : verts [V,3] f32 = lattice position * step + min, faces [F,3] int64 (reversed winding;
 *                 -1 where the owning cell lies outside the grid, as the reference).
 * sdf: [nx,ny,nz] fp32 dense, index i*ny*nz + j*nz + k.  Output ORDER is deterministic: vertices by
 * lattice-edge key (cell*3+dir), faces by (cell, triangle) -- the reference's atomicAdd order is not
 * reproducible even by itself; compare after canonicalisation.  No growing singleton, no
 * 5%-of-cells scratch guess (CudaKernels.cu:590-592): the caller sizes the outputs exactly.  `workspace` must be 8-byte
 * aligned (it holds 64-bit classification planes); verts / faces double as scratch inside sr_mc_emit before they are written. */
int64_t sr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int sr_mc_count(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float iso, void* workspace, uint32_t* counts_dev, void* stream);
int sr_mc_emit(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float iso, const void* workspace, float xstep, float ystep,
               float zstep, float xmin, float ymin, float zmin, float* verts, int64_t* faces, void* stream);

/* ---------------------------------------------------------------- small per-element ops
 * sr_svd3x3: batched 3x3 SVD on device, A = U diag(S) V^T, S descending -- replaces
 *   `torch.svd(Jacobs.cpu())` of the deformation regulariser (model/network.py:576).  A,U,V [n,3,3], S [n,3].
 */
int sr_svd3x3(const float* A, int64_t n, float* U, float* S, float* V, void* stream);

/* Effective weights of up to SR_PACK_MAX_LAYERS linear layers in one launch (weight_norm dim 0 as model/network.py:65-66 and
 * model/RenderNet.py:46-47: W = g v/|v|; g NULL = plain layer): W [N, ldw] zero padded, WT [K, ldwt] = W^T zero padded,
 * norms [N] = |v_n|.  _unpack is the backward: dW [N, lddw] -> gv [N, K] (and gg [N] for weight-normed layers), i.e.
 * aten::_weight_norm_interface_backward; accumulate != 0 adds to gv / gg. */
/* dst [rows * group, ldd]: row r * group + g = (g == 0 ? a : b)[r, :n] zero padded to `width` columns; group 1 (a only) or 2 (the
 * (primal, tangent) row interleave of the group-2 GEMMs); a NULL source gives zero rows. */
int sr_rows_pad(const float* a, int64_t lda, int32_t na, const float* b, int64_t ldb, int32_t nb, int64_t rows, int32_t group, float* dst, int64_t ldd,
                int32_t width, void* stream);
/* out [n,E] = per-frame sums of the rows of X [P, ldx >= E]: out[f] = sum_{index[r] == f} X[r, :E]  (n <= 32) -- the backward of the
 * per-frame code gather conds[batch_inds] (model/Deformer.py:61,75), deterministic (fixed-order folds; torch's index_add uses float
 * atomics).  `partial`: sr_rows_frame_sum_workspace_floats(P, E, n) floats of scratch. */
int64_t sr_rows_frame_sum_workspace_floats(int64_t P, int32_t E, int32_t n);
int sr_rows_frame_sum(const float* X, int64_t ldx, int64_t P, int32_t E, const int64_t* index, int32_t n, float* partial, float* out, void* stream);

#define SR_PACK_MAX_LAYERS 16
typedef struct { const float* v; const float* g; float* W; float* WT; float* norms; int32_t N, K; int64_t ldw, ldwt; } sr_pack_layer;
typedef struct { int32_t nlayers; sr_pack_layer layer[SR_PACK_MAX_LAYERS]; } sr_pack_table;
typedef struct { const float* dW; int64_t lddw; const float* v; const float* g; const float* norms; float* gv; float* gg;
                 const float* db; float* gb;   /* optional: bias gradient gb[n] += db[n] (n < N) in the same launch */
                 int32_t N, K, accumulate, pad_; } sr_unpack_layer;
typedef struct { int32_t nlayers; sr_unpack_layer layer[SR_PACK_MAX_LAYERS]; } sr_unpack_table;
int sr_pack_weights(const sr_pack_table* host_table, void* stream);
int sr_unpack_grads(const sr_unpack_table* host_table, void* stream);

/* Adam step (torch.optim.Adam, weight_decay 0, amsgrad off -- the optimizer of train.py:139) of up to SR_ADAM_MAX_TENSORS contiguous
 * float32 tensors in one launch.  Per tensor: p, g (gradient), m (exp_avg), v (exp_avg_sq), numel, lr, bias1 = 1 - beta1^step,
 * inv_sqrt_bias2 = 1 / sqrt(1 - beta2^step) (host-side scalars of the tensor's step count). */
#define SR_ADAM_MAX_TENSORS 64
typedef struct { float* p; const float* g; float* m; float* v; int64_t numel; float lr, bias1, inv_sqrt_bias2, pad_; } sr_adam_tensor;
typedef struct { int32_t ntensors; float beta1, beta2, eps;
                 float one_minus_beta1, one_minus_beta2;   /* formed in double on the host: 1 - 0.999f is off by 1.3e-5 relative in float */
                 int32_t pad_[2]; sr_adam_tensor tensor[SR_ADAM_MAX_TENSORS]; } sr_adam_table;
int sr_adam_step(const sr_adam_table* host_table, void* stream);

/* Stream diagnostics (no reference counterpart: the reference runs one stream).
 * sr_stream_flag_set stores `value` to *flag when its stream reaches it; sr_stream_flag_wait holds its stream (one sleeping wave)
 * until *flag - value >= 0 in wrapping 32-bit arithmetic or until timeout_ms has passed, in which case *timed_out (optional) is
 * incremented and the stream proceeds.  An ordering of two streams that does not go through the runtime's events: used by
 * tools/stream_latency2.py to tell a property of hipStreamWaitEvent from a property of the schedule (the 10+ ms the ray selection
 * seemed to wait for the main stream turned out to be the host running a whole iteration ahead of the GPU, with either primitive). */
/* Diagnostics: writes the device's constant 100 MHz counter to *out when the stream reaches this point (timestamps that are
 * comparable across streams, which the runtime's event timestamps are not: tools/host_profile.py). */
int sr_stream_stamp(uint64_t* out, void* stream);
int sr_stream_flag_set(uint32_t* flag, uint32_t value, void* stream);
int sr_stream_flag_wait(const uint32_t* flag, uint32_t value, uint32_t* timed_out, int32_t timeout_ms, void* stream);

/* ---------------------------------------------------------------- interp2x_boundary3d (K10/K11)
 * Replaces MCAcc/cuda/interp2x_boundary3d.cpp:forward/backward -> interp2x_boundary3d_kernel.cu:11-151, 155-239
 * (compiled but never enabled in the reference: every Seg3dLossless is built with use_cuda_impl=False).
 * in [BC, d,h,w] -> out [BC, 2d-1,2h-1,2w-1] = mean of the 1/2/4/8 coarse parents; is_boundary (u8) = parents'
 * (v > balance) flags disagree.  _bwd: grad_out [BC, 2d-1,2h-1,2w-1] -> grad_in [BC, d,h,w] (adjoint stencil). */
int sr_interp2x3d_fwd_f32(const float* in, int64_t BC, int32_t d, int32_t h, int32_t w, float balance, float* out, uint8_t* is_boundary, void* stream);
int sr_interp2x3d_fwd_f64(const double* in, int64_t BC, int32_t d, int32_t h, int32_t w, float balance, double* out, uint8_t* is_boundary, void* stream);
int sr_interp2x3d_bwd_f32(const float* grad_out, int64_t BC, int32_t d, int32_t h, int32_t w, float* grad_in, void* stream);
int sr_interp2x3d_bwd_f64(const double* grad_out, int64_t BC, int32_t d, int32_t h, int32_t w, double* grad_in, void* stream);
/* Candidate voxels of one Seg3dLossless level (MCAcc/seg3d_lossless.py:296-312: smooth_conv3x3(is_boundary) > 0, minus the
 * voxels evaluated at earlier levels, nonzero) in one pass: out_index receives the flat indices z*H*W + y*W + x (capacity
 * D*H*W entries, unordered), *count_dev their number (uint64, device).  is_boundary / done: [D,H,W] bytes (0 / non-0). */
int sr_seg3d_candidates(const uint8_t* is_boundary, const uint8_t* done, int32_t D, int32_t H, int32_t W, int64_t* out_index, uint64_t* count_dev,
                        void* stream);

/* ---------------------------------------------------------------- rasterisation either side of the refiner
 * The reference calls pytorch3d 0.4.0 here (third-party CUDA, not in its repository; restated in oracle/raster_oracle.py,
 * parity unpinned).  Both entry points work in pytorch3d's NDC frame: +x left, +y up, pixel (row, col) centred at
 * (1 - (2 col + 1)/W, 1 - (2 row + 1)/H); xy_ndc [nimg, V, 2], z [nimg, V] = view-space depth.
 *
 * sr_points_silhouette_*: replaces PointsRasterizer(radius, points_per_pixel = K) + AlphaCompositor with one all-ones
 *   feature as called at model/network.py:178-190,495-497 through PointsRendererWithFrags (model/CameraMine.py:285-305):
 *   mask[img,row,col] = sum_k a_k prod_{j<k}(1 - a_j) over the K covering points nearest in z, a = 1 - dist2/radius^2
 *   (dist2 < radius^2, NDC units; z < 0 skipped).  _bwd returns d(sum gmask * mask)/d xy_ndc (what pytorch3d's
 *   rasterize_points backward propagates through `dists`).  `workspace` (256-byte aligned, _workspace_bytes) carries the
 *   per-pixel transmittance and selection thresholds from _fwd to _bwd.
 * sr_rasterize_meshes: replaces MeshRasterizer(blur_radius 0, faces_per_pixel 1, perspective_correct, no barycentric
 *   clipping, no culling) of model/network.py:877-892,492: faces [F,3] int64 shared by all images (rows containing -1 are
 *   skipped: MCGpu border faces) -> pix_to_face [nimg,H,W] int64 (packed img*F + f, -1 = background), bary [nimg,H,W,3]
 *   (-1 on background), zout [nimg,H,W] nullable.  zbuf_u64: scratch of nimg*H*W 8-byte words; pix_to_face and the
 *   (8-byte aligned) head of bary hold the large-face queue until the last pass overwrites them. */
int64_t sr_points_silhouette_workspace_bytes(int64_t nimg, int64_t pts_per_img, int32_t H, int32_t W, float radius);
int sr_points_silhouette_fwd(const float* xy_ndc, const float* z, int64_t nimg, int64_t pts_per_img, int32_t H, int32_t W, float radius,
                             int32_t K, float* mask, void* workspace, void* stream);
int sr_points_silhouette_bwd(const float* xy_ndc, const float* z, int64_t nimg, int64_t pts_per_img, int32_t H, int32_t W, float radius,
                             const void* workspace, const float* gmask, float* gxy, void* stream);
int sr_rasterize_meshes(const float* xy_ndc, const float* z, const int64_t* faces, int64_t nimg, int64_t V, int64_t F, int32_t H, int32_t W,
                        void* zbuf_u64, int64_t* pix_to_face, float* bary, float* zout, void* stream);

/* ---------------------------------------------------------------- shaded mesh previews of infer (csrc/shade.hip)
 * The reference's infer renders two previews with pytorch3d 0.4.0's HardPhongShader (model/network.py:306-337, installed by
 * infer.py:80-90): third-party code, restated from its published semantics, parity unpinned.  faces [F,3] int64 is
 * one template shared by N deformed copies verts [N,V,3].  A face with an index outside [0, V) -- the -1 border faces of marching
 * cubes -- is skipped; indices are NOT checked against V as an error (that would need a device-to-host copy).
 * sr_vertex_adjacency: once per template: the vertex -> (face, corner) lists as CSR, sorted by 3 f + corner within a vertex:
 *   offsets [V+1] int64 (offsets[V] = 3 x the number of used faces), nbr [3F,2] int32, 8-byte aligned = for corner c of face f the
 *   pair (faces[f][(c+1)%3], faces[f][(c+2)%3]).  cursor: scratch of V int32.  V <= 2^31 - 1.
 * sr_vertex_normals: Meshes.verts_normals_packed: n[v] = sum over its corners, in CSR order, of cross(p_next - p_v, p_prev - p_v),
 *   then n / max(|n|, 1e-6) (a vertex in no face: 0) -> normals [N,V,3].  Fixed summation order: two calls return identical bits.
 * sr_shade_phong: phong_shading + hard_rgb_blend with TexturesVertex of ones and one point light per image, on the fragments of
 *   sr_rasterize_meshes (pix_to_face [N,H,W] packed img*F + f, bary [N,H,W,3]); cam_pos, light_loc [N,3] world space; host_phong[13]
 *   = ambient rgb, diffuse rgb, specular rgb (each the light's colour times the material's), shininess, background rgb.  Per covered
 *   pixel, p / n = the barycentric blends of verts / normals, texel = b0 + b1 + b2, L = normalize(light - p), n = normalize(n),
 *   V = normalize(cam - p) (normalize: x / max(|x|, 1e-6)), c = n.L:
 *     rgb = (ambient + diffuse relu(c)) texel + specular (relu(V.(2 c n - L)) [c > 0])^shininess
 *   Background (pix_to_face < 0; also one outside [0, N F) or on a skipped face): the background colour.  rgba [N,H,W,4], 16-byte
 *   aligned.  Alpha is written as 1: what pytorch3d 0.4.0's hard_rgb_blend is believed to concatenate -- UNPINNED (nothing here
 *   could run pytorch3d; the reference's infer.py never reads it). */
int sr_vertex_adjacency(const int64_t* faces, int64_t V, int64_t F, int64_t* offsets, int32_t* cursor, int32_t* nbr, void* stream);
int sr_vertex_normals(const float* verts, int64_t N, int64_t V, const int64_t* offsets, const int32_t* nbr, float* normals, void* stream);
int sr_shade_phong(const float* verts, const float* normals, const int64_t* faces, int64_t N, int64_t V, int64_t F, int32_t H, int32_t W,
                   const int64_t* pix_to_face, const float* bary, const float* cam_pos, const float* light_loc, const float* host_phong,
                   float* rgba, void* stream);

/* ---------------------------------------------------------------- fused per-ray / per-vertex tails of one step (csrc/step_ops.hip)
 * Each pair replaces a block of elementwise torch ops of the reference's training step (and their autograd mirror) with one
 * launch for the value and one for the gradient.  Reductions are deterministic (fixed summation order, no float atomics).
 *
 * Camera (model/CameraMine.py:44-70,129-170,171-262).  All pointers are DEVICE pointers (the intrinsics are learnable
 * parameters, config.conf:10-15): R [3,3] row-major with p_cam = p R + T, T [3] (NULL = 0), f [2], c [2]; W, H in pixels;
 * one_minus_inv_w/h = (float)(1 - 1/W), (float)(1 - 1/H) computed on the host as the reference's Python scalars are.
 *   sr_cam_project_ndc_fwd: ps [n,3] -> xy [n,2] in pytorch3d's NDC frame (x = f0/(W/2) X/Z + 1 - 1/W - c0/(W/2)), z [n] = view depth.
 *   sr_cam_project_ndc_bwd: gxy / gz (either may be NULL) -> gps [n,3] (NULL: skipped) and, when `partial`
 *     ([sr_step_param_blocks(n), 16] scratch) is given, gparams [16] = gR[9] | gT[3] | gf[2] | gc[2].
 *   sr_cam_view_rays_fwd: pixels [n,3] = (col, row, 1) -> unit world rays normalize([(c0 h - u)/f0, (c1 h - w)/f1, h]) R^T.
 *   sr_cam_view_rays_bwd: grays -> gparams [16] in the same layout (gT slots untouched = 0). */
#define SR_STEP_MAX_FRAMES 8
typedef struct { const float* R; const float* T; const float* f; const float* c; float W, H, one_minus_inv_w, one_minus_inv_h; } sr_camera;
int sr_step_reduce_blocks(int64_t rows);      /* workgroups (= rows of `partial`, SR_STEP_LOSS_SLOTS - 1 floats each) a loss reduction over `rows` uses */
int sr_step_param_blocks(int64_t rows);       /* rows of `partial` (16 floats each) of the camera backward kernels */
int sr_cam_project_ndc_fwd(const float* ps, int64_t n, const sr_camera* cam, float* xy, float* z, void* stream);
int sr_cam_project_ndc_bwd(const float* ps, int64_t n, const sr_camera* cam, const float* gxy, const float* gz, float* gps, float* partial,
                           float* gparams, void* stream);
int sr_cam_view_rays_fwd(const float* pixels, int64_t n, const sr_camera* cam, float* rays, void* stream);
int sr_cam_view_rays_bwd(const float* pixels, int64_t n, const sr_camera* cam, const float* grays, float* partial, float* gparams, void* stream);

/* Cardinal rays and deformed normals (utils/utils.py:132-169) from the deformation Jacobian J [n,3,3] (J[i][j] = d d_i / d p_j):
 *   sr_cardinal_rays_fwd: out = normalize(J^-1 v); rows whose |det J| < 1e-4 (FastMinv's rule) keep normalize(v) and ok = 0.
 *   sr_cardinal_rays_bwd: cotangent of out -> gJ [n,9] = -(J^-T gu)(J^-1 v)^T and gv [n,3] = J^-T gu (either may be NULL; zero on ok = 0 rows,
 *     where the reference substitutes rays.detach()).
 *   sr_deformed_normals: out = normalize(J^-T n) (J n on singular rows); no gradient ('test' phase of compute_deformed_normals). */
int sr_cardinal_rays_fwd(const float* J, const float* v, int64_t n, float* out, uint8_t* ok, void* stream);
int sr_cardinal_rays_bwd(const float* J, const float* v, int64_t n, const float* gout, float* gJ, float* gv, void* stream);
int sr_deformed_normals(const float* J, const float* onx, int64_t n, float* out, void* stream);

/* Loss reductions.  out [SR_STEP_LOSS_SLOTS]: out[0] = the loss, out[1 + f] / out[1 + SR_STEP_MAX_FRAMES + f] = the per-frame
 * numerator / denominator sums the backward reads back as `saved`.  partial: [sr_step_reduce_blocks(rows), SR_STEP_LOSS_SLOTS - 1]
 * scratch, may be NULL when that is 1.  gloss: device scalar (cotangent of the loss).
 *   colour (model/network.py:611-618): rays (b, r, c) [P] into gt [N,H,W,3]; mean over frames of the per-frame mean of |gt - colour|_1.
 *     A row with b[i] < 0 is MASKED in the colour and the normal reduction: no term, no count, exact-zero gradients (the reference
 *     drops the rays its refiner rejected by a boolean gather, network.py:599-606 -- a host round trip; the mask keeps the shape static).
 *   normal (model/network.py:620-639): gt normal image [N,H,W,3] -> flip diag(-1,1,-1) -> world (R [3,3]) -> unit (valid when
 *     |.| > 1e-4) -> canonical (J^T), against normalize(nx_raw); weighted != 0 multiplies by clamp(-rays . n_def, 0, 1)^2 with
 *     n_def = sr_deformed_normals(J, nx_raw) (detached); masked scatter-mean over frames.  _bwd: gnx_raw [P,3], gJ [P,9] (NULL: skipped).
 *   eikonal (model/network.py:547-549): mean (|g| - 1)^2 over g [n,3].
 *   def_regu (model/network.py:565-582 + utils/utils.py:48-52): S [n,3] singular values -> mean GM(sum_k log(s_k)^2, c); _bwd goes
 *     straight to gJ [n,9] = U diag(gS) V^T with the U, V of sr_svd3x3.   sr_svd3x3_bwd: the plain gS -> gJ.
 *   mask IoU (model/network.py:652-654): masks, gt [N, hw]; mean over frames of 1 - sum(m g) / sum |m + g - m g|. */
#define SR_STEP_LOSS_SLOTS (1 + 2 * SR_STEP_MAX_FRAMES)
typedef struct { const int64_t* b; const int64_t* r; const int64_t* c; int64_t P; int32_t N, H, W; } sr_ray_pixels;
int sr_color_loss_fwd(const sr_ray_pixels* px, const float* colors, const float* gt, float* partial, float* out, void* stream);
int sr_color_loss_bwd(const sr_ray_pixels* px, const float* colors, const float* gt, const float* saved, const float* gloss, float* gcolors,
                      void* stream);
int sr_normal_loss_fwd(const sr_ray_pixels* px, const float* nx_raw, const float* J, const float* gt_normals, const float* R, const float* rays,
                       int weighted, float* partial, float* out, void* stream);
int sr_normal_loss_bwd(const sr_ray_pixels* px, const float* nx_raw, const float* J, const float* gt_normals, const float* R, const float* rays,
                       int weighted, const float* saved, const float* gloss, float* gnx_raw, float* gJ, void* stream);
int sr_eikonal_loss_fwd(const float* g, int64_t n, float* partial, float* out, void* stream);
int sr_eikonal_loss_bwd(const float* g, int64_t n, const float* gloss, float* gg, void* stream);
int sr_def_regu_loss_fwd(const float* S, int64_t n, float c, float* partial, float* out, void* stream);
int sr_def_regu_loss_bwd(const float* U, const float* S, const float* V, int64_t n, float c, const float* gloss, float* gJ, void* stream);
int sr_svd3x3_bwd(const float* U, const float* V, const float* gS, int64_t n, float* gJ, void* stream);
int sr_mask_iou_loss_fwd(const float* masks, const float* gt, int N, int64_t hw, float* partial, float* out, void* stream);
int sr_mask_iou_loss_bwd(const float* masks, const float* gt, int N, int64_t hw, const float* saved, const float* gloss, float* gmasks, void* stream);

/* Normal equations of the implicit differentiation (model/network.py:702-771): b = [grad_f ; [v]x J] (4x3),
 * rhs = grad_l^T (b^T b)^-1 b^T with FastMinv's singularity rule (ok = 0, zeros) -> cot_f [n] = -rhs[0], rhs_tail [n,3] = rhs[1:4],
 * temp [n,3] = rhs[1:4] (-[v]x). */
int sr_implicit_solve(const float* grad_f, const float* J, const float* v, const float* grad_l, int64_t n, float* cot_f, float* rhs_tail, float* temp,
                      uint8_t* ok, void* stream);

/* Texture baking (csrc/texture.hip): the reference's texture_mesh_extract.py on the GPU.  opendr's visibility / VideoAvatar's Isomapper
 * are third-party code outside the reference repository; their semantics are restated, parity unpinned.
 *   sr_uv_rasterize: vt [Vt,2] in [0,1]^2, ft [F,3] -> face [R,R] int32 (-1: none) and bary [R,R,3].  Texel (r, c) has centre
 *     u = (c + 0.5) / R, v = 1 - (r + 0.5) / R and belongs to the lowest-indexed non-degenerate UV triangle that contains it (edge
 *     functions >= 0 for either winding; |twice the area| <= 1e-14 or an index outside [0, Vt): owns nothing).  Integer atomics only.
 *   sr_face_visibility: visible [N,F] uint8 = the face owns a pixel of pix_to_face [N,H,W] (packed indices n F + f, as
 *     sr_rasterize_meshes writes them) and its three vertices are in the mask: rint of xy_pix [N,V,2] inside the viewport and
 *     mask [N,H,W] (uint8) set there.
 *   sr_view_alpha: alpha [N,V] = max(0, dot(normalize(verts - cam_pos[n]), -normals)).
 *   sr_texture_accumulate: for the T covered texels (tface [T], tbary [T,3]) and the N views in order: cosv = UV-barycentric blend of
 *     alpha (0 on a face that is not visible); where cosv > the minimum over the texel's agg_num slots, the first slot holding the
 *     minimum takes (cosv, bilinear sample of images [N,H,W,3] at the blend of the vertices' pixel positions, fids[n]).  Slots are
 *     slot-major: slot_cos / slot_view [agg_num,T], slot_rgb [agg_num,3,T]; count / min_cos / min_idx [T] carry the fill count and the
 *     running minimum between calls.  The caller initialises slot_cos = cosv0 (>= 0), slot_view = -1, slot_rgb = count = min_idx = 0,
 *     min_cos = cosv0.
 *   sr_texture_resolve: per covered texel (texel [T]: its index r R + c) into the [R,R] images: count = slots > cosv0, mask_final =
 *     count >= check_num, view_id = view of the first slot with the maximum (-1 outside mask_final), tex_median [R,R,3] = per-channel
 *     median of the filled slots (even count: mean of the two middle values; 0 outside mask_final).
 *   sr_texture_fill: texture [R,R,3] = tex_median on mask_final, a push-pull fill (known texels averaged down a 2x pyramid to 1 x 1,
 *     then bilinearly pulled back into unknown cells only) on the square dilation of tex_mask by `dilate` texels (cv2.dilate's window
 *     i - k/2 .. i - k/2 + k - 1) minus mask_final, 0 elsewhere.  workspace: sr_texture_fill_workspace_bytes(R) bytes, 16-byte aligned. */
int sr_uv_rasterize(const float* vt, const int64_t* ft, int64_t Vt, int64_t F, int32_t R, int32_t* face, float* bary, void* stream);
int sr_face_visibility(const int64_t* pix_to_face, const int64_t* faces, int64_t N, int64_t V, int64_t F, const float* xy_pix, const uint8_t* mask,
                       int32_t H, int32_t W, uint8_t* visible, void* stream);
int sr_view_alpha(const float* verts, const float* normals, const float* cam_pos, int64_t N, int64_t V, float* alpha, void* stream);
int sr_texture_accumulate(int64_t T, const int32_t* tface, const float* tbary, const int64_t* faces, int64_t F, int64_t V, int32_t N,
                          const uint8_t* visible, const float* alpha, const float* xy_pix, const float* images, int32_t H, int32_t W,
                          const int32_t* fids, int32_t agg_num, float cosv0, float* slot_cos, float* slot_rgb, int32_t* slot_view, int32_t* count,
                          float* min_cos, int32_t* min_idx, void* stream);
int sr_texture_resolve(int64_t T, const int32_t* texel, int32_t agg_num, float cosv0, int32_t check_num, const float* slot_cos,
                       const float* slot_rgb, const int32_t* slot_view, int32_t* count, uint8_t* mask_final, int32_t* view_id, float* tex_median,
                       void* stream);
int64_t sr_texture_fill_workspace_bytes(int32_t R);
int sr_texture_fill(const float* tex_median, const uint8_t* mask_final, const uint8_t* tex_mask, int32_t R, int32_t dilate, float* texture,
                    void* workspace, void* stream);

/* Template preparation for the texture stage (csrc/mesh_prep.hip): vertex-clustering simplification, box-projection charts and the
 * contested-texel count of an atlas.  The reference leaves this step to the user; the semantics are stated in DESIGN.md 3.15, unpinned.
 * Sorting, unique and compaction happen between the calls (mesh_prep_ops.py).  Integer and min / max atomics only.
 *   sr_meshprep_bounds: box [8] int32 <- the bit patterns of the float32 per-axis minimum [0..3) and maximum [3..6) of verts [V,3] over
 *     the finite coordinates (-0 counts as +0), and box[6] = 1 when a coordinate is not finite.
 *   sr_meshprep_cell_keys: key [V] = (k ny + j) nx + i with ijk = floor((v - lo) / cell): float32 subtraction, IEEE float32 division;
 *     lo [3] on the device.  cell > 0 and nx ny nz < 2^62, else SR_EINVAL.
 *   sr_meshprep_cell_mean: out [C,3] = mean of verts[order[offsets[c] .. offsets[c + 1])], summed in that order in double.
 *   sr_meshprep_face_keys: out_faces [F,3] = vertex_map[faces]; (key_hi, key_lo) = (lo Vn + mid, hi) of the sorted corners, (-1, -1)
 *     for a face with a repeated corner or an index outside [0, V).  Vn <= 2^31.
 *   sr_meshprep_face_first: with the faces sorted by (key_hi, key_lo), ties in original order (perm [F]: sorted position -> face),
 *     keep[face] = 1 for the first of every run of equal non-negative keys, else 0.
 *   sr_chart_classify: cls [F] = 2 axis + (negative ? 1 : 0) of the normal (b - a) x (c - a) in double from the float32 coordinates,
 *     every product and difference rounded on its own (no fused multiply-add); axis = argmax |n|, lowest axis on a tie, zero normal 0.
 *   sr_chart_edge_keys: key [3F] of half-edge 3 f + corner = (min V + max) 6 + cls[f]; -1 for an edge from a vertex to itself.
 *     V <= 2^30.
 *   sr_chart_hook: parent [F] int32 is a forest of stars.  next <- parent, then for neighbours i - 1, i of the sorted half-edge keys
 *     (perm [3F]: position -> half-edge) with equal non-negative keys, whose faces have different roots: next[larger root] =
 *     min(next[larger root], smaller root); changed [1] = 1 when there was one.  n = 3 F.
 *   sr_chart_jump: next[f] = parent[parent[f]]; changed = 1 when some next[f] != parent[f].
 *   sr_chart_bbox: per chart (chart [F] in [0, C)) the box of its faces' projected corners: for axis k and positive sign (u, v) =
 *     (x_{k+1}, x_{k+2}), swapped for a negative sign.  bbox_min [C,2], extent [C,2] = max - min in float32; box [C,4] int32 is scratch.
 *   sr_chart_uv: vt [3F,2], vt[3 f + corner] = (origin[chart] + padding + 0.5 + (p - bbox_min[chart]) scale) / R in double, rounded
 *     once; origin [C,2] int64.
 *   sr_uv_overlap_count: total [1] = the number of texel centres (sr_uv_rasterize's convention) that lie strictly inside two or more
 *     non-degenerate UV triangles (every barycentric > eps); count [R,R] int32 = triangles per texel.
 * Quadric-optimal placement of the cluster representatives (the clustering, the faces and the map are unchanged):
 *   sr_meshprep_cell_faces: slot [3F]; slot[3 f + k] = vertex_map[faces[f][k]] unless an earlier corner of face f has that cell or the
 *     row has an index outside [0, V): then C.  A stable sort of slot by value lists, per cell, every face that touches it once, in
 *     ascending face index.
 *   sr_meshprep_cell_quadric: per cell c of `cells` [C] (its grid key; ijk = key mod nx, key / nx mod ny, key / (nx ny)), from the faces
 *     face_slots[face_offsets[c] .. face_offsets[c + 1]) / 3 (positions of the sorted slots) and the members order[offsets[c] ..
 *     offsets[c + 1]) as for sr_meshprep_cell_mean, all in double from the float32 inputs: every face with area adds w n n^T to A and
 *     w d n to b (N = (p1 - p0) x (p2 - p0), L = |N|, n = N / L, w = L / 2, d = n . p0; L = 0 or not finite adds nothing); entry e of
 *     the list goes to partial sum e mod 16, each partial sum runs in list order, and the 16 meet pairwise (1, 2, 4, 8 apart).  m = the
 *     cell mean, lambda = reg trace(A) / 3, x = m + (A + lambda I)^-1 (b - A m) by Cholesky; lambda > 0 false, or x not finite: x = m
 *     and SR_QUADRIC_NO_PLANES.  x is clamped per component to [lo + i cell, lo + (i + 1) cell] (SR_QUADRIC_CLAMPED when that moved
 *     it) and rounded once: out [C,3]; flags [C] int32; shift [C] float32 = |x - m| / cell.  reg > 0 and finite, cell > 0.
 *   sr_meshprep_face_flips: for g in [0, Fn), new face new_faces[g] at new_verts [Vn,3] against old face faces[source[g]] at verts:
 *     counts [2] int64 = (faces whose unnormalised normals have a negative dot product, faces whose new normal is zero). */
#define SR_QUADRIC_CLAMPED 1
#define SR_QUADRIC_NO_PLANES 2
int sr_meshprep_cell_faces(const int64_t* faces, int64_t F, const int64_t* vertex_map, int64_t V, int64_t C, int64_t* slot, void* stream);
int sr_meshprep_cell_quadric(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* face_slots, const int64_t* face_offsets,
                             const int64_t* order, const int64_t* offsets, const int64_t* cells, int64_t C, const float* lo, float cell, int64_t nx,
                             int64_t ny, double reg, float* out, int32_t* flags, float* shift, void* stream);
int sr_meshprep_face_flips(const float* verts, int64_t V, const int64_t* faces, int64_t F, const float* new_verts, int64_t Vn,
                           const int64_t* new_faces, const int64_t* source, int64_t Fn, int64_t* counts, void* stream);
int sr_meshprep_bounds(const float* verts, int64_t V, int32_t* box, void* stream);
int sr_meshprep_cell_keys(const float* verts, int64_t V, const float* lo, float cell, int64_t nx, int64_t ny, int64_t nz, int64_t* key, void* stream);
int sr_meshprep_cell_mean(const float* verts, int64_t V, const int64_t* order, const int64_t* offsets, int64_t C, float* out, void* stream);
int sr_meshprep_face_keys(const int64_t* faces, int64_t F, const int64_t* vertex_map, int64_t V, int64_t Vn, int64_t* out_faces, int64_t* key_hi,
                          int64_t* key_lo, void* stream);
int sr_meshprep_face_first(const int64_t* key_hi, const int64_t* key_lo, const int64_t* perm, int64_t F, uint8_t* keep, void* stream);
int sr_chart_classify(const float* verts, int64_t V, const int64_t* faces, int64_t F, int32_t* cls, void* stream);
int sr_chart_edge_keys(const int64_t* faces, int64_t F, int64_t V, const int32_t* cls, int64_t* key, void* stream);
int sr_chart_hook(const int64_t* sorted_key, const int64_t* perm, int64_t n, const int32_t* parent, int32_t* next, int64_t F, int32_t* changed,
                  void* stream);
int sr_chart_jump(const int32_t* parent, int64_t F, int32_t* next, int32_t* changed, void* stream);
int sr_chart_bbox(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int32_t* cls, const int64_t* chart, int64_t C, int32_t* box,
                  float* bbox_min, float* extent, void* stream);
int sr_chart_uv(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int32_t* cls, const int64_t* chart, int64_t C,
                const float* bbox_min, const int64_t* origin, double scale, int32_t padding, int32_t R, float* vt, void* stream);
int sr_uv_overlap_count(const float* vt, const int64_t* ft, int64_t Vt, int64_t F, int32_t R, double eps, int32_t* count, int64_t* total,
                        void* stream);

/* Edge-collapse decimation of the template (csrc/mesh_collapse.hip; DESIGN.md 3.15: this package's own semantics, unpinned).  One round
 * on verts [V,3] float32, faces [F,3] (every index in [0, V), no repeated corner) and quadrics [V,10] double (xx xy xz yy yz zz of
 * sum w n n^T, then sum w d n, then sum w d^2); sorting, unique and compaction happen between the calls (mesh_prep_ops.py).  Integer
 * atomics only (or, add, 64-bit min).  V <= 2^31 and F <= 2^30 throughout, else SR_EINVAL.
 *   sr_collapse_vertex_quadrics: quadrics[v] = the plane quadrics (n, w, d as for sr_meshprep_cell_quadric) of the faces slots[offsets[v]
 *     .. offsets[v + 1]) / 3, summed in that order; slots [3F] = the corners 3 f + c sorted (stably) by the vertex they hold.
 *   sr_collapse_edge_keys: key [3F] of half-edge 3 f + c (corner c to corner c + 1) = min V + max; -1 in a row that is not a face.
 *   sr_collapse_edge_heads: unique_key [E] ascending, its run perm[offsets[e] .. offsets[e + 1]) in the sorted half-edges (perm [3F]:
 *     position -> half-edge): edges [E,2] = (key / V, key mod V), count [E] = the run's length, opposite [E,2] = the vertex opposite
 *     the run's first and second half-edge (-1: none), locked [V] int32 = 1 on both ends of every edge whose count is not 2 (zeroed
 *     here first), directed [2E] = a V + b and, E later, b V + a: sorted, they list every vertex's neighbours in ascending order.
 *   sr_collapse_candidates: per edge (a, b): Q = Q_a + Q_b, m the midpoint, x = m + (A + lambda I)^-1 (b - A m), lambda = reg trace(A)
 *     / 3, by Cholesky (x = m when lambda > 0 fails or x is not finite); positions [E,3] = x rounded to float32; cost = max(x^T A x -
 *     2 b^T x + c, 0) at the rounded x in double, rounded to float32.  key [E] = (bits of cost) << 32 | fmix32(e) (murmur3's 32-bit
 *     finaliser) when the edge is a candidate, else INT64_MAX.  A candidate has count 2, unlocked ends, two distinct opposite vertices
 *     that are the only common neighbours of a and b (neighbours [2E] = the sorted `directed`, neighbour_offsets [V + 1] into it),
 *     val(a) + val(b) - 4 >= 3 and val(opposite) - 1 >= 3, and every face at a or b that does not hold the other keeps n_old . n_new
 *     > flip_cos |n_old| |n_new| and |n_new| > 0 with that corner at x.  reg > 0 and finite, -1 <= flip_cos < 1.
 *   sr_collapse_min1: m1 [V] = the least key < INT64_MAX over the edges at v, INT64_MAX without one.
 *   sr_collapse_min2: m2 [V] = min(m1[v], m1[u] over the neighbours u of v); m2 must not be m1.
 *   sr_collapse_select: selected [E] uint8 = key < INT64_MAX and key == m2[a] == m2[b]; record [2] int64 = (selected, candidates).
 *   sr_collapse_apply_vertices: for every selected edge, in place: verts[a] = positions[e], quadrics[a] += quadrics[b], target[b] = a
 *     (target [V] int64; the selected edges must share no endpoint, as those of sr_collapse_select do).
 *   sr_collapse_apply_faces: out_faces [F,3] = target[faces]; keep [F] uint8 = the three are distinct.
 *   sr_collapse_map_jump: next[v] = parent[parent[v]]; changed [1] int32 = 1 when some next[v] != parent[v]; next must not be parent. */
int sr_collapse_vertex_quadrics(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* slots, const int64_t* offsets,
                                double* quadrics, void* stream);
int sr_collapse_edge_keys(const int64_t* faces, int64_t F, int64_t V, int64_t* key, void* stream);
int sr_collapse_edge_heads(const int64_t* unique_key, const int64_t* offsets, int64_t E, const int64_t* perm, const int64_t* faces, int64_t F, int64_t V,
                           int64_t* edges, int32_t* count, int64_t* opposite, int32_t* locked, int64_t* directed, void* stream);
int sr_collapse_candidates(const float* verts, int64_t V, const int64_t* faces, int64_t F, const double* quadrics, const int64_t* slots,
                           const int64_t* offsets, const int64_t* neighbours, const int64_t* neighbour_offsets, const int64_t* edges,
                           const int32_t* count, const int64_t* opposite, const int32_t* locked, int64_t E, double reg, double flip_cos,
                           float* positions, int64_t* key, void* stream);
int sr_collapse_min1(const int64_t* edges, const int64_t* key, int64_t E, int64_t V, int64_t* m1, void* stream);
int sr_collapse_min2(const int64_t* edges, int64_t E, int64_t V, const int64_t* m1, int64_t* m2, void* stream);
int sr_collapse_select(const int64_t* edges, const int64_t* key, int64_t E, int64_t V, const int64_t* m2, uint8_t* selected, int64_t* record,
                       void* stream);
int sr_collapse_apply_vertices(const int64_t* edges, const float* positions, const uint8_t* selected, int64_t E, float* verts, int64_t V,
                               double* quadrics, int64_t* target, void* stream);
int sr_collapse_apply_faces(const int64_t* faces, int64_t F, const int64_t* target, int64_t V, int64_t* out_faces, uint8_t* keep, void* stream);
int sr_collapse_map_jump(const int64_t* parent, int64_t V, int64_t* next, int32_t* changed, void* stream);

/* Drawing the textured template (csrc/texrender.hip): a mip-mapped UV shader on the fragments of sr_rasterize_meshes.  The semantics
 * are this package's own: stated here, restated in float64 by the tests, unpinned.
 *   Mip buffer: float4 texels, levels concatenated; level 0 has side R, level l + 1 side (R_l + 1) / 2, the last level side 1 (L
 *     levels, R <= 32768); a level starts where the one before ends, so every texel is 16-byte aligned when the buffer is.
 *   sr_texture_mips: texture [R,R,3] float32, or uint8 when is_u8 (a byte x is x / 255.f, IEEE division); valid [R,R] uint8, null = all
 *     valid.  Level 0 texel = (rgb w, w), w = 1 on a valid texel and 0 elsewhere.  Texel (r, c) of level l + 1 = the sum of the
 *     in-range texels of {2r, 2r + 1} x {2c, 2c + 1} of level l, divided by their number (1, 2 or 4).  One launch per level.
 *   sr_texture_face_lod: lod [N,F] per image and face from xy_pix [N,V,2] (pixels), faces [F,3], vt [Vt,2], ft [F,3]: with J the
 *     Jacobian of the affine map pixel -> uv through the three corners, rho = R max(|J column x|, |J column y|) (Euclidean lengths,
 *     texels per pixel) and lod = clamp(log2(rho) + bias, 0, L - 1).  A face with an index outside [0, V) / [0, Vt), or a screen
 *     triangle with |det| < 1e-12, gets L - 1.  L must be the level count of R.
 *   sr_shade_textured: pix_to_face [N,H,W] (packed n F + f), bary [N,H,W,3] (perspective-correct) -> rgba [N,H,W,4], 16-byte aligned,
 *     and coverage [N,H,W] (nullable).  Covered pixel: uv = sum_k b_k vt[ft[f][k]]; on level l the sample point is x = u R_l - 0.5,
 *     y = (1 - v) R_l - 0.5 (sr_uv_rasterize's texel centres), four clamp-to-edge taps with bilinear weights, on the levels
 *     floor(lod) and min(floor(lod) + 1, L - 1) blended by lod - floor(lod) (lod [N,F] read at the packed index) -> (P, w); rgba =
 *     (P / w, 1) where w > 0, (host_hole[3], 1) otherwise; coverage = w.  Uncovered pixel (p < 0, p >= N F, or an ft index outside
 *     [0, Vt)): rgba = (bg_image [N,H,W,3] if given, else host_background[3]; 0), coverage 0, and the texture is not read.  No
 *     atomics: two runs give identical bits. */
int sr_texture_mips(const void* texture, int32_t is_u8, const uint8_t* valid, int32_t R, float* mips, void* stream);
int sr_texture_face_lod(const float* xy_pix, const int64_t* faces, const float* vt, const int64_t* ft, int64_t N, int64_t V, int64_t F,
                        int64_t Vt, int32_t R, float bias, int32_t L, float* lod, void* stream);
int sr_shade_textured(const int64_t* pix_to_face, const float* bary, int64_t N, int64_t F, int32_t H, int32_t W, const int64_t* ft,
                      const float* vt, int64_t Vt, const float* mips, int32_t R, int32_t L, const float* lod, const float* host_background,
                      const float* host_hole, const float* bg_image, float* rgba, float* coverage, void* stream);

/* Skinning-weight field of a body mesh (csrc/lbsw.hip): compute_lbswField + smooth_weights of model/Deformer.py:235-284.
 *   sr_lbsw_knn_blend: field [nj,D,H,W] (channel-major, W fastest) over the box [bmin, bmax] (host float[3] each).  Voxel (w, h, d) has
 *     centre ((w + 1/2) / W) (bmax - bmin) + bmin per axis, or (w / (W - 1)) ... with align_corners (every size >= 2 then).  Its value
 *     is the blend of the rows of vert_ws [nv,nj] of the k nearest of verts [nv,3], weighted by 1 / clamp(distance, 1e-4, 1) and
 *     normalised over the k.  "Nearest" orders the vertices by (squared float32 distance to the float32 centre, vertex index): of
 *     equal distances the LOWER VERTEX INDEX wins (torch.topk, which the reference calls, promises no order among ties).  The
 *     selected distances are re-evaluated in double for the weights.  1 <= k <= min(SR_LBSW_MAX_K, nv), else SR_EINVAL.
 *   sr_lbsw_smooth: one Jacobi step src -> dst (distinct buffers, both [nj,D,H,W]): interior voxels become mean6 + 0.7 (w - mean6) of
 *     the OLD field, then every voxel, border included, is divided by its sum over the channels.  A grid without interior (a size
 *     < 3) is only renormalised.  No truncation of small weights (Deformer.py:243 has it commented out).
 * Neither uses atomics: two calls give identical bits. */
#define SR_LBSW_MAX_K 32
int sr_lbsw_knn_blend(const float* verts, const float* vert_ws, int64_t nv, int32_t nj, int32_t k, int32_t W, int32_t H, int32_t D,
                      const float* bmin, const float* bmax, int32_t align_corners, float* field, void* stream);
int sr_lbsw_smooth(const float* src, float* dst, int32_t nj, int32_t W, int32_t H, int32_t D, void* stream);

/* SMPL body model, forward only, float32 (csrc/smpl.hip): SMPL.forward / skeleton / avatar of smpl_pytorch/SMPL.py:93-173 with
 * batch_rodrigues / batch_global_rigid_transformation of smpl_pytorch/util.py:35-103.  24 joints; all pointers are device memory
 * unless named host_*.  No atomics: two calls give identical bits.
 *   sr_smpl_shape:   v_shaped [B,nv,3] = v_template [nv,3] + sum_k beta [B,nbeta] shapedirs [nbeta, nv*3].
 *   sr_smpl_regress: out [B,nk,3] = sum_v reg [nv,nk] x [B,nv,3], 3 nk <= 128.  Partial sums of 128 vertices in ascending order go
 *     to `partial` (sr_smpl_regress_workspace_floats floats), a second launch adds them in ascending order.
 *   sr_smpl_pose:    theta [B,24,3] axis-angle -> Rs [B,24,3,3] by the reference's route (|theta + 1e-8|, half-angle quaternion,
 *     normalise, quat2mat); theta NULL: Rs is an input.  feature [B,207] = (Rs[:,1:] - I); the chain over host_parents [24]
 *     (host_parents[i] < i for i > 0, entry 0 ignored) from the rest joints J [B,24,3] gives J_transformed [B,24,3] and
 *     A [B,24,4,4] = G - pad(G [J;0]).
 *   sr_smpl_skin:    verts [B,nv,3] = (sum_j weights [nv,24] A[b,j]) [v_posed; 1] with v_posed = rest[b,v] + posedirs [207,nv,3] .
 *     feature[b]; rest is read at rest + b * rest_batch_stride (floats; 0 shares one mesh among the batch).  posedirs and feature
 *     both NULL: v_posed = rest (SMPL.avatar).  One workgroup serves SR_SMPL_BATCH_TILE batch items of 128 vertices, so posedirs
 *     is read once per batch tile.
 * Limits (SR_EINVAL beyond them): the batch index is a grid's second dimension, so B <= 65535 for sr_smpl_shape and sr_smpl_regress
 * and B <= 65535 * SR_SMPL_BATCH_TILE for sr_smpl_skin (a longer sequence is evaluated in slices); nv <= INT32_MAX / 4; for
 * sr_smpl_regress also nv * nk and 3 * B * nk <= INT32_MAX. */
#define SR_SMPL_BATCH_TILE 8
int sr_smpl_shape(const float* v_template, const float* shapedirs, const float* beta, int32_t B, int32_t nbeta, int64_t nv, float* v_shaped,
                  void* stream);
int64_t sr_smpl_regress_workspace_floats(int32_t B, int64_t nv, int32_t nk);
int sr_smpl_regress(const float* x, const float* reg, int32_t B, int64_t nv, int32_t nk, float* partial, float* out, void* stream);
int sr_smpl_pose(const float* theta, float* Rs, const float* J, const int32_t* host_parents, int32_t B, float* feature, float* J_transformed,
                 float* A, void* stream);
int sr_smpl_skin(const float* rest, int64_t rest_batch_stride, const float* posedirs, const float* feature, const float* weights, const float* A,
                 int32_t B, int64_t nv, float* verts, void* stream);

/* SMPL body model, backward, float32 (csrc/smpl_grad.hip): the adjoints of the four stages above, shapes and limits as there.  No float
 * atomics; every sum has an order fixed by the shapes, so two calls give identical bits.  A g* argument is the cotangent of the
 * tensor it names.
 *   sr_smpl_regress_bwd: g_x [B,nv,3] = sum_k reg [nv,nk] g_out [B,nk,3] (nk <= 42); accumulate != 0 adds to g_x instead.
 *   sr_smpl_shape_bwd:   g_beta [B,nbeta] = sum_e shapedirs [nbeta, nv*3] g_vshaped [B, nv*3], nbeta <= 32; `partial` holds
 *     sr_smpl_shape_bwd_workspace_floats floats (one row per 2048 elements, added in ascending order by a second launch).
 *   sr_smpl_skin_bwd:    from gV [B,nv,3]: g_rest [B,nv,3] = (sum_j w_vj R_j)^T gV (R_j: the 3x3 of A[b,j]), gA [B,24,12] (rows 0..2 of
 *     each 4x4) = sum_v w_vj gV_v (x) [v_posed_v; 1] with v_posed recomputed as in sr_smpl_skin, and with posedirs
 *     g_feature [B,207] = sum_{v,c} posedirs[p,v,c] g_rest[b,v,c] (posedirs, feature and g_feature all NULL: v_posed = rest).
 *     `partial` holds sr_smpl_skin_bwd_workspace_floats floats: one row per batch item and 128 vertices, added in ascending order by
 *     a second launch.  posedirs is read once per SR_SMPL_BATCH_TILE batch items.
 *   sr_smpl_pose_bwd:    the reverse of sr_smpl_pose, from gA [B,24,12], gJ_transformed [B,24,3], g_feature [B,207] and gRs [B,24,3,3]
 *     (each may be NULL = zero); Rs and A are sr_smpl_pose's outputs.  -> gJ [B,24,3], and g_theta [B,24,3] through the axis-angle
 *     route as written (the +1e-8 included), or with theta NULL gRs_out [B,24,3,3]. */
int sr_smpl_regress_bwd(const float* g_out, const float* reg, int32_t B, int64_t nv, int32_t nk, int32_t accumulate, float* g_x, void* stream);
int64_t sr_smpl_shape_bwd_workspace_floats(int32_t B, int32_t nbeta, int64_t nv);
int sr_smpl_shape_bwd(const float* shapedirs, const float* g_vshaped, int32_t B, int32_t nbeta, int64_t nv, float* partial, float* g_beta,
                      void* stream);
int64_t sr_smpl_skin_bwd_workspace_floats(int32_t B, int64_t nv);
int sr_smpl_skin_bwd(const float* rest, int64_t rest_batch_stride, const float* posedirs, const float* feature, const float* weights,
                     const float* A, const float* gV, int32_t B, int64_t nv, float* partial, float* g_rest, float* gA, float* g_feature,
                     void* stream);
int sr_smpl_pose_bwd(const float* theta, const float* Rs, const float* J, const float* A, const int32_t* host_parents, int32_t B,
                     const float* gA, const float* gJ_transformed, const float* g_feature, const float* gRs, float* g_theta, float* gRs_out,
                     float* gJ, void* stream);

/* Keypoint data term of smpl_fit.py (csrc/smpl_grad.hip), value and gradient in one launch: for frame t < T and joint k < K <= 64,
 * p = joints [T,K,3] + trans [T,3] is projected as RectifiedPerspectiveCameras.project does (pc = p R + T, x = cx - fx pc_x / pc_z,
 * y = cy - fy pc_y / pc_z) and contributes (w_k c_tk)^2 sigma^2 r^2 / (sigma^2 + r^2), r the pixel distance to kp [T,K,3] = (x, y, c).
 * A joint with c = 0 or a non-finite target contributes nothing; one with pc_z <= 0 contributes nothing and is counted in behind [T].
 * host_camera: 16 HOST floats R [3,3], T [3], fx, fy, cx, cy (passed by value to the kernel).  -> energy [T], g_joints [T,K,3],
 * g_trans [T,3] (the gradients of energy[t]); the sums over k run in ascending order. */
int sr_keypoint_energy(const float* joints, const float* trans, const float* kp, const float* joint_weights, const float* host_camera,
                       float sigma, int32_t T, int32_t K, float* energy, float* g_joints, float* g_trans, int32_t* behind, void* stream);

/* Silhouette term of smpl_fit.py (csrc/silfit.hip).  No atomics; two calls give identical bits.
 *   sr_edt:           d2 [F,H,W] int32 = the exact squared pixel distance of every pixel to the nearest non-zero pixel of mask [F,H,W]
 *     uint8 in the same frame (0 on the mask); SR_EDT_EMPTY in every entry of a frame without one.  F <= 65535, H, W <= 8192.  Two launches.
 *   sr_contour_flags: flags [F,H,W] uint8 = 1 where a mask pixel has a 4-neighbour inside the image that is background.
 *   sr_silhouette_energy: for frame t < F the points [F,V,3] (world, translation included) are projected as in sr_keypoint_energy
 *     (host_camera: the same 16 HOST floats); pixel (col, row) has its centre at x = col, y = row.
 *       e_in[t]  = (1/V) sum_v rho(d(x, y)), rho(r) = sigma^2 r^2 / (sigma^2 + r^2), d the bilinear interpolation of sqrt(d2) in the cell
 *         x0 = min(floor(x), W-2), y0 = min(floor(y), H-2); a vertex with pc_z <= 0, a non-finite pixel position or one outside
 *         [0, W-1] x [0, H-1] contributes nothing and is counted in outside[t]; a frame whose d2 holds SR_EDT_EMPTY has e_in = 0.
 *       e_cov[t] = (1/n) sum_{s<n} rho(max(0, min_v |c_ts - xy_tv| - margin)), n = min(counts[t], S), c = samples [F,S,2] int32 (x, y);
 *         the minimum runs over the vertices in front of the camera with a finite pixel position, a tie goes to the lower index, a
 *         sample without any such vertex contributes nothing; the match is held fixed in the gradient.
 *     -> e_in [F], e_cov [F], outside [F] int32, g_points [2,F,V,3] (the gradients of e_in[t] and of e_cov[t]), and the work arrays
 *     xy [F,V,2], valid [F,V] uint8 (0 behind / non-finite, 1 in front, 2 inside the image), vres [F,V,3] (a vertex's inside value and
 *     its gradient in the pixel position), match [F,S] int32 (-1: none), sres [F,S,3] (a sample's residual value and its gradient at the
 *     matched pixel).  H, W >= 2, S <= 65536.  Three launches: projection and inside term, match, gradient and sums. */
#define SR_EDT_EMPTY 1073741824
int sr_edt(const uint8_t* mask, int32_t F, int32_t H, int32_t W, int32_t* d2, void* stream);
int sr_contour_flags(const uint8_t* mask, int32_t F, int32_t H, int32_t W, uint8_t* flags, void* stream);
int sr_silhouette_energy(const float* points, const int32_t* d2, const int32_t* samples, const int32_t* counts, const float* host_camera,
                         float sigma, float margin, int32_t F, int32_t V, int32_t S, int32_t H, int32_t W, float* xy, uint8_t* valid,
                         float* vres, int32_t* match, float* sres, float* e_in, float* e_cov, int32_t* outside, float* g_points, void* stream);

/* Mesh regularisers of the template step (csrc/mesh_reg.hip): mesh_laplacian_smoothing(method='uniform'), mesh_edge_loss and
 * mesh_normal_consistency of pytorch3d 0.4.0 as model/network.py:655-670 calls them, restated, on one mesh of V vertices.
 * Topology, int32, built once per remesh by mesh_losses.MeshTopology: nbr_row [V+1] / nbr [2E] the neighbour CSR (ascending per row),
 * pairs [P,4] = (v0, v1, a, b) one row per pair of faces at an edge, pair_row [V+1] / pair_ent [4P] the CSR of the entries
 * pair * 4 + slot per vertex (ascending per row).  `terms` is a set of SR_MESHREG_* bits; a term that is off is neither computed nor read.
 *   sr_meshreg_fwd: out[3] = (lap, edge, nc), 0 for a term that is off.  lap_q [V,3] (lap), edge_g [V,3] (edge) and pair_g [P,4,3]
 *     (normal; may be null when no gradient is wanted) receive what the backward gathers; workspace: sr_meshreg_workspace_bytes(V, P)
 *     bytes, 8-byte aligned, not zeroed.  At most three launches.
 *   sr_meshreg_bwd: grad [V,3] = g_lap d lap + g_edge d edge + g_nc d nc, the three cotangents read from DEVICE memory (one float each);
 *     a null cotangent or a null buffer leaves that term out.  One launch, one thread per vertex, gathers only.
 * No atomics: all sums run in a fixed order, two calls give identical bits. */
#define SR_MESHREG_LAP 1
#define SR_MESHREG_EDGE 2
#define SR_MESHREG_NORMAL 4
int64_t sr_meshreg_workspace_bytes(int64_t V, int64_t P);
int sr_meshreg_fwd(const float* verts, int64_t V, const int32_t* nbr_row, const int32_t* nbr, int64_t E, const int32_t* pairs, int64_t P,
                   int32_t terms, float target_length, float* lap_q, float* edge_g, float* pair_g, void* workspace, float* out, void* stream);
int sr_meshreg_bwd(int64_t V, const int32_t* nbr_row, const int32_t* nbr, int64_t E, const int32_t* pair_row, const int32_t* pair_ent, int64_t P,
                   const float* lap_q, const float* edge_g, const float* pair_g, const float* g_lap, const float* g_edge, const float* g_nc,
                   float* grad, void* stream);

/* Frames of a capture sequence kept on the GPU as bytes (csrc/frames.hip): what dataset/dataset.py:85-115 decodes and uploads per
 * iteration, as one launch per batch.  The store, written once: img_u8 [F, pitch3] and normal_u8 [F, pitch3] (NULL: the sequence has
 * no normals; then out_normal is NULL too) hold H*W*3 bytes per frame in the order cv2.imread gives them (B, G, R per pixel),
 * mask_u8 [F, pitch1] holds H*W bytes, each 0 or 1.  The bytes behind a frame up to its pitch are padding and are never converted.
 *   sr_frames_fetch: for slot n < N with frame f = ids[n], out_img [N,H,W,3] = (b / 255 - 0.5) * 2, out_normal [N,H,W,3] =
 *     (2 b) / 255 - 1 with the three channels of each pixel reversed, out_mask [N,H,W] = (float) m: the reference's float32
 *     expressions with IEEE division, bit for bit.  The ids come EITHER by value, ids_by_value a HOST pointer to an sr_frame_ids whose
 *     first N entries are used (copied into the launch: no transfer, no synchronisation), OR from DEVICE memory, ids_device [N]
 *     int64; exactly one of the two is non-NULL.  An id outside [0, F) reads nothing: its slot is NaN in out_img / out_normal and 0
 *     in out_mask.
 * Limits (SR_EINVAL beyond them): pitch3 and pitch1 multiples of 16 with pitch3 >= 3 H W and pitch1 >= H W; the three stores 16-byte
 * aligned; 1 <= N <= SR_FRAMES_MAX_BATCH by value, N <= 65535 from device memory (the slot is a grid's second dimension);
 * H W <= SR_FRAMES_MAX_PIXELS.  16-byte stores are used when H W % 4 == 0 and the outputs are 16-byte aligned, dword stores otherwise.
 * No atomics: two calls give identical bits. */
#define SR_FRAMES_MAX_BATCH 16
#define SR_FRAMES_MAX_PIXELS 1073741824
struct sr_frame_ids_s {
  int32_t id[SR_FRAMES_MAX_BATCH];
};
typedef struct sr_frame_ids_s sr_frame_ids;
int sr_frames_fetch(const uint8_t* img_u8, const uint8_t* normal_u8, const uint8_t* mask_u8, int64_t pitch3, int64_t pitch1, int32_t F, int32_t H,
                    int32_t W, const sr_frame_ids* ids_by_value, const int64_t* ids_device, int32_t N, float* out_img, float* out_normal,
                    float* out_mask, void* stream);

/* Device-side training log (csrc/trainlog.hip): the scalars a training loop prints per iteration, gathered into one row of a float32
 * ring in device memory by one small launch, so that the host reads rows later instead of waiting for each value.
 *   sr_log_row: one workgroup of one wave.  Lane k < n reads slot k and writes ring[(row % ring_rows) * ld + k]; the columns
 *     n <= k < ld of that row are written as NaN, so that a value of an earlier lap of the ring never reads as current.  Slot kinds:
 *     SR_LOG_EMPTY -> NaN; SR_LOG_F32: src[k] is a DEVICE float32 scalar, copied bit for bit; SR_LOG_I64: src[k] is a DEVICE int64
 *     scalar, converted with (float) (round to nearest even); SR_LOG_IMM: imm[k], a host float.
 *   `slots_by_value` is a HOST pointer; the structure is copied into the launch (no transfer, no synchronisation).  The POINTERS and
 *   the immediates are captured when the call is issued; the VALUES behind the pointers are read in stream order, i.e. the row holds
 *   what earlier work on `stream` left there -- the caller keeps the sources alive until the launch has run.  No atomics, plain loads
 *   and stores: two calls give identical bits.
 * SR_EINVAL: n outside [1, SR_LOG_MAX_SLOTS], ld < n, ring_rows < 1, row < 0, a kind that is none of the four, a NULL src of an F32 /
 * I64 slot, an F32 source that is not 4-byte aligned, an I64 source that is not 8-byte aligned, a NULL or not 4-byte aligned ring, a
 * NULL slots_by_value. */
#define SR_LOG_MAX_SLOTS 32
#define SR_LOG_EMPTY 0
#define SR_LOG_F32 1
#define SR_LOG_I64 2
#define SR_LOG_IMM 3
struct sr_log_slots_s {
  const void* src[SR_LOG_MAX_SLOTS];
  float imm[SR_LOG_MAX_SLOTS];
  uint8_t kind[SR_LOG_MAX_SLOTS];
};
typedef struct sr_log_slots_s sr_log_slots;
int sr_log_row(const sr_log_slots* slots_by_value, int32_t n, float* ring, int32_t ring_rows, int32_t ld, int64_t row, void* stream);

/* Motion-JPEG encoder (csrc/mjpeg.hip): baseline sequential JPEG (SOF0), 8 bit, YCbCr (JFIF full range) 4:2:0, of B frames
 * rgb [B,H,W,3] uint8 -- the entropy-coded bytes only; the host writes the header segments and EOI around them.  With R = ceil(H / 16)
 * MCU rows of M = ceil(W / 16) MCUs (the picture padded by repeating its last column and row), one restart interval is one MCU row.
 * All arithmetic is integer: two calls give identical bytes.
 *   sr_jpeg_transform: coef [B, R M, 6, 64] int16 = the quantised DCT coefficients of each MCU's blocks Y00 Y01 Y10 Y11 Cb Cr in zigzag
 *     order; qtab [2,64] uint16 are the luminance and chrominance divisors (1..255), in zigzag order as DQT lists them.
 *   sr_jpeg_entropy: codes every interval with huff [4,256] = (code | length << 16) of the DC luminance, DC chrominance, AC luminance
 *     and AC chrominance tables, indexed by category / (run << 4 | category); DC prediction restarts with each interval and its last
 *     byte is padded with 1s.  rowbuf receives interval i's bytes, every 0xFF followed by 0x00, at i * 12 M SR_JPEG_BLOCK_BYTES
 *     (i = b R + r) and row_len [B R] their count.  `bits` is scratch of bits_dwords dwords, 128-byte aligned, zeroed by the call:
 *     B R intervals of (6 M SR_JPEG_BLOCK_BYTES / 4 rounded up to a multiple of 32) dwords.
 *   sr_jpeg_gather: out = the frames' scan data one after the other, frame b at offsets[b] .. offsets[b + 1] (offsets [B+1] int64):
 *     its intervals in order with RSTm, m = r mod 8, behind interval r < R - 1.  row_start [B R] int64 is scratch.
 * SR_JPEG_BLOCK_BYTES bounds the code of one block before stuffing for every input (a DC code of at most 22 bits and 63 AC codes of at
 * most 26), so the buffers' sizes are functions of (B, H, W) alone: SR_ENOSPC if bits_dwords is less than the B R strides above, rowbuf_bytes < 12 B R M
 * SR_JPEG_BLOCK_BYTES or out_bytes < B (12 R M SR_JPEG_BLOCK_BYTES + 2 (R - 1)), and nothing is launched.  SR_EINVAL: a NULL
 * pointer, B, H or W outside [1, 65535], coef not 16-byte or bits not 128-byte aligned. */
#define SR_JPEG_BLOCK_BYTES 208
int sr_jpeg_transform(const uint8_t* rgb, int32_t B, int32_t H, int32_t W, const uint16_t* qtab, int16_t* coef, void* stream);
int sr_jpeg_entropy(const int16_t* coef, int32_t B, int32_t H, int32_t W, const uint32_t* huff, uint32_t* bits, int64_t bits_dwords,
                    uint8_t* rowbuf, int64_t rowbuf_bytes, uint32_t* row_len, void* stream);
int sr_jpeg_gather(const uint8_t* rowbuf, const uint32_t* row_len, int32_t B, int32_t H, int32_t W, int64_t* row_start, uint8_t* out,
                   int64_t out_bytes, int64_t* offsets, void* stream);

/* Surface-distance evaluation (csrc/surfdist.hip): exact point-to-mesh distance through a uniform grid, and a stratified surface
 * sampler.  The semantics are this package's own: stated here, restated in float64 by the tests, unpinned.
 *   tri [F,12] float32, 16-byte aligned: the corners a, b, c of every face and three floats of padding.  F < 2^31.
 *   Grid: lo [3] on the device, cell > 0, (nx, ny, nz) with at most 2^24 cells; the coordinate of x on an axis is floor((x - lo) / cell)
 *     in float32 (IEEE subtraction and division), clamped to [0, n - 1]; a cell's key is (k ny + j) nx + i.
 *   sr_surfdist_face_cells: count [F] = the number of cells the box of face f overlaps (the product of its three coordinate ranges).
 *   sr_surfdist_emit_pairs: key [pairs] / pair_face [pairs]: face f writes its cells in ascending key from offset[f] on (offset = the
 *     exclusive cumulative sum of count, pairs = its total); nothing is written at or beyond `pairs`.
 *   sr_surfdist_query: per point the float32 distance to the mesh as a set of closed triangles, the face that attains it (the lowest
 *     index among equal float32 squared distances) and the closest point on that face.  cell_start [cells + 1] int64 / cell_faces [pairs]
 *     int32: the faces of every cell.  The search visits Chebyshev rings of cells round the point's (clamped) cell and stops when the
 *     best squared distance is below (1 - 2^-14)^2 times a lower bound of everything unvisited, or nothing is left; at most
 *     max(nx, ny, nz) rings.  A point with a NaN or Inf coordinate gets dist = NaN, face = -1, closest = NaN without any search.
 *   sr_surfdist_brute: the same outputs from a loop over all faces, with the same distance function and tie rule: bit-identical.
 *   sr_mesh_sample: n samples of the surface: sample i lies at r = (i + xi) / n cum_area[F - 1] (double) of the cumulative face areas
 *     cum_area [F] float64 -- the first face with cum_area > r -- with barycentrics (1 - sqrt u, sqrt u (1 - v), sqrt u v); xi, u, v =
 *     (splitmix64(3 i + {0, 1, 2} + seed 0x9E3779B97F4A7C15) >> 11) 2^-53.  points [n,3], face [n], normals [n,3] (unit, of the face).
 * SR_EINVAL: a NULL pointer, a count <= 0, F >= 2^31 - 1, tri not 16-byte aligned, cell <= 0 or more than 2^24 cells. */
int sr_surfdist_face_cells(const float* tri, int64_t F, const float* lo, float cell, int32_t nx, int32_t ny, int32_t nz, int64_t* count, void* stream);
int sr_surfdist_emit_pairs(const float* tri, int64_t F, const float* lo, float cell, int32_t nx, int32_t ny, int32_t nz, const int64_t* offset,
                           int64_t pairs, int64_t* key, int32_t* pair_face, void* stream);
int sr_surfdist_query(const float* points, int64_t P, const float* tri, int64_t F, const float* lo, float cell, int32_t nx, int32_t ny, int32_t nz,
                      const int64_t* cell_start, const int32_t* cell_faces, int64_t pairs, float* dist, int64_t* face, float* closest, void* stream);
int sr_surfdist_brute(const float* points, int64_t P, const float* tri, int64_t F, float* dist, int64_t* face, float* closest, void* stream);
int sr_mesh_sample(const float* tri, const double* cum_area, int64_t F, int64_t n, int64_t seed, float* points, int64_t* face, float* normals,
                   void* stream);

/* Point-to-plane ICP of surface samples against a mesh (csrc/icp.hip; DESIGN.md 3.19, this package's own semantics): the two launches of
 * one iteration.  The mesh, the grid and their refusals are sr_surfdist_query's.
 *   state [SR_ICP_STATE] float64 on the device: M (3 x 3, row major), t (3), the done flag at SR_ICP_DONE (0 or 1), then the number of
 *     solves that ran live; T(p) = M p + t.  (ox, oy, oz), rho > 0: the frame the system is normalised in (centre and half diagonal of
 *     the target's box).
 *   sr_icp_accumulate: for every sample p of points [S,3]: q = fl32(((M0 px + M1 py) + M2 pz) + t) per row, in double; (d, f, c) =
 *     sr_surfdist_query's triple of q; n = the unit normal of face f in double (0 without area); the pair is kept when q is finite and
 *     d <= max_dist.  With x = (q - o) / rho, w = [x cross n, n, n.x, n.(q - c) / rho] (8 numbers), a block adds w_j w_l (j <= l, row
 *     major: 36), 1 and d^2 over its kept pairs and writes them as its row of partial [blocks, SR_ICP_COLS] (the last two columns are
 *     0).  blocks must be min(ceil(S / 256), SR_ICP_MAX_BLOCKS).  With the done flag set nothing is written, unless `measure` is not 0.
 *   sr_icp_solve (one wave): the column sums of partial over the blocks in ascending order; the first 7 x 7 of them scaled to a unit
 *     diagonal and solved for xi = (omega, tau, sigma) by Cholesky in double -- sigma is 0 unless `scale`; an unknown whose column
 *     has a mean square <= 2^-46 or whose pivot is below 2^-20 is set to 0 and leaves the system --; M <- (1 + sigma) exp(omega) M,
 *     t <- o + (1 + sigma) exp(omega) (t - o) + rho tau; done <- max |xi| < tol.  Row `it` of history [iters, SR_ICP_HISTORY]: kept
 *     pairs, the rms of their d (before this update), max |xi|, rank, sqrt(|M|_F^2 / 3), done.  With the done flag set on entry the
 *     state is left alone and the row repeats row it - 1 with done = 1.
 *   sr_icp_score (one 256-lane workgroup per candidate): row c of table [N,12] float64 is M (3 x 3, row major)
 *     then t of a candidate transform.  For every sample p of points [S,3] float32: q as in sr_icp_accumulate; a q that is not finite
 *     is skipped; d = sr_surfdist_query's distance of q; e = fminf(d, trunc[c]) (trunc [N] float32, +Inf: no truncation).  score
 *     [N,2] float64: row c = (the sum of (double)e (double)e, the number of samples that took part).  A lane adds its samples i = lane,
 *     lane + 256, ... in that order, a wave adds its lanes by the xor butterfly (distances 32 down to 1), the workgroup adds its
 *     waves as ((r0 + r1) + r2) + r3: no atomics, and two launches give identical bits.
 * SR_EINVAL: a NULL pointer, S <= 0, N <= 0, tri not 16-byte aligned, a bad grid, rho <= 0, max_dist < 0 or NaN, a wrong block count,
 * iters <= 0, `it` outside [0, iters). */
#define SR_ICP_MAX_BLOCKS 1024
#define SR_ICP_COLS 40
#define SR_ICP_HISTORY 6
#define SR_ICP_STATE 16
#define SR_ICP_DONE 12
int sr_icp_accumulate(const float* points, int64_t S, const float* tri, int64_t F, const float* lo, float cell, int32_t nx, int32_t ny, int32_t nz,
                      const int64_t* cell_start, const int32_t* cell_faces, int64_t pairs, const double* state, double ox, double oy, double oz,
                      double rho, float max_dist, int32_t measure, double* partial, int32_t blocks, void* stream);
int sr_icp_solve(const double* partial, int32_t blocks, double ox, double oy, double oz, double rho, int32_t scale, double tol, int32_t it,
                 int32_t iters, double* state, double* history, void* stream);
int sr_icp_score(const float* points, int64_t S, const double* table, int32_t N, const float* tri, int64_t F, const float* lo, float cell,
                 int32_t nx, int32_t ny, int32_t nz, const int64_t* cell_start, const int32_t* cell_faces, int64_t pairs, const float* trunc,
                 double* score, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SELFRECON_HIP_H_ */
