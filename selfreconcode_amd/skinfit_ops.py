"""Operators of the skin fit (csrc/skinfit.hip): GPU tensors only, no autograd.  `export_gltf.py` is the public
interface.  A glTF skin has one fixed weight vector per vertex; the trained skinner looks its 24 weights up at the deformed point, so
they change from frame to frame.  Per vertex and over the fit frames, with C candidate joints c_k and sum_k x_k = 1,

    sum_t | sum_k x_k A_{t,c_k} [q_t; 1] - (y_t - trans_t) |^2 = x^T H x,      H = sum_t D_t^T D_t,   d_tk = A_{t,c_k} [q_t; 1] - (y_t - trans_t)

`accumulate` adds a batch of frames into H (lower triangle, entry-major [36, V], float64); `solve` minimises x^T H x + lambda |x - xbar|^2
over the simplex with at most K non-zeros by enumerating the supports.  method "fused" is the HIP kernels, "composed" the same from
torch operators in float64: the witness, and what the kernels are timed against.  Two calls give identical bits.

The entry points are declared in csrc/skinfit_abi.h and bound here (_lib.bind_header): a library without them fails this import."""
import os

import torch

from . import _lib
from .build import CSRC

_DEFINES, _ = _lib.bind_header(os.path.join(CSRC, "skinfit_abi.h"))
MAX_CANDS = _DEFINES["SR_SKINFIT_MAX_CANDS"]
TRI = _DEFINES["SR_SKINFIT_TRI"]                           # rows of H: the lower triangle of an 8 x 8 matrix
JOINTS = _DEFINES["SR_SKINFIT_JOINTS"]
SLAB = _DEFINES["SR_SKINFIT_SLAB"]                         # frames of a batch that go through the LDS together
LAMBDA_FLOOR = 1e-24                                       # added to lambda: H = 0 (a rigid or one-frame capture) still has one optimum
METHODS = ("fused", "composed")


def tri(k, l):
    """Row of H that holds entry (k, l), l <= k."""
    return k * (k + 1) // 2 + l


def _check_method(method):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")


def _check_counts(C, K=None):
    if not 1 <= int(C) <= MAX_CANDS:
        raise ValueError(f"C in [1, {MAX_CANDS}] expected, got {C}")
    if K is not None and not 1 <= int(K) <= int(C):
        raise ValueError(f"K in [1, C = {C}] expected, got {K}")


def candidates(wbar, C=MAX_CANDS):
    """(cands [V,C] int32, xbar [C,V] float64) from the mean field weights wbar [V,24]: the C joints with the largest mean weight
    (stable sort: a tie goes to the lower joint), and wbar restricted to them and renormalised -- the prior of the solve.  A vertex
    whose candidates' weights sum to 0 gets 1 on its first candidate."""
    _check_counts(C)
    if wbar.dim() != 2 or wbar.shape[1] != JOINTS or wbar.shape[0] == 0:
        raise ValueError(f"candidates: wbar [V,{JOINTS}] expected, got {tuple(wbar.shape)}")
    wbar = wbar.double()
    order = torch.sort(wbar, dim=1, descending=True, stable=True)[1][:, :int(C)]
    picked = torch.gather(wbar, 1, order)
    total = picked.sum(1, keepdim=True)
    first = torch.zeros_like(picked)
    first[:, 0] = 1.
    xbar = torch.where(total > 0., picked / torch.where(total > 0., total, torch.ones_like(total)), first)
    return order.to(torch.int32).contiguous(), xbar.t().contiguous()


def new_normal_matrix(V, device):
    """H = 0: [36, V] float64."""
    return torch.zeros((TRI, int(V)), dtype=torch.float64, device=device)


def residual_rows(q, y, A, trans, cands):
    """D [T,V,C,3] float64 of a batch: d_tk = A_{t,c_k} [q_t; 1] - (y_t - trans_t), every float widened first."""
    T, V = q.shape[0], q.shape[1]
    A = A.double().reshape(T, JOINTS, 3, 4)
    qd = q.double()
    Aq = torch.einsum('tjxc,tvc->tvjx', A[..., :3], qd) + A[:, None, :, :, 3]                    # [T,V,24,3]
    index = cands.long().clamp(0, JOINTS - 1)[None, :, :, None].expand(T, V, cands.shape[1], 3)
    return torch.gather(Aq, 2, index) - (y.double() - trans.double()[:, None, :])[:, :, None, :]


def accumulate(H, q, y, A, trans, cands, method="fused"):
    """H += sum over the batch's frames of D^T D, in place, and returns H.  q, y [T,V,3] float32; A [T,24,4,4] or [T,24,12] (the
    posed transforms, or their top three rows); trans [T,3]; cands [V,C] int32; H [36,V] float64 (new_normal_matrix)."""
    _check_method(method)
    _lib.require_gpu(H, q, y, A, trans, cands)
    if q.dim() != 3 or q.shape[2] != 3 or q.shape[0] == 0 or q.shape[1] == 0 or tuple(y.shape) != tuple(q.shape):
        raise ValueError(f"accumulate: q, y [T,V,3] expected, got {tuple(q.shape)} and {tuple(y.shape)}")
    T, V = q.shape[0], q.shape[1]
    if A.dim() == 4:
        A = A[:, :, :3, :]
    if A.shape[0] != T or A.shape[1] != JOINTS or A[0, 0].numel() != 12 or tuple(trans.shape) != (T, 3):
        raise ValueError(f"accumulate: A [{T},24,4,4] or [{T},24,12] and trans [{T},3] expected, got {tuple(A.shape)} and {tuple(trans.shape)}")
    if cands.dim() != 2 or cands.shape[0] != V or cands.dtype != torch.int32:
        raise ValueError(f"accumulate: cands [{V},C] int32 expected, got {cands.dtype} {tuple(cands.shape)}")
    C = cands.shape[1]
    _check_counts(C)
    if tuple(H.shape) != (TRI, V) or H.dtype != torch.float64 or not H.is_contiguous():
        raise ValueError(f"accumulate: H [{TRI},{V}] float64, contiguous, expected, got {H.dtype} {tuple(H.shape)}")
    q, y, trans, cands = _lib.f32c(q), _lib.f32c(y), _lib.f32c(trans), cands.contiguous()
    A12 = _lib.f32c(A.reshape(T, JOINTS, 12))
    if method == "fused":
        _lib.launch("sr_skinfit_accumulate", q, q, y, A12, trans, T, V, cands, C, H)
        return H
    D = residual_rows(q, y, A12, trans, cands)
    G = torch.einsum('tvkx,tvlx->klv', D, D)
    for k in range(C):
        for l in range(k + 1):
            H[tri(k, l)] += G[k, l]
    return H


def full_matrix(H, C):
    """The symmetric [V,C,C] matrices of H [36,V]."""
    M = H.new_zeros((H.shape[1], C, C))
    for k in range(C):
        for l in range(k + 1):
            M[:, k, l] = M[:, l, k] = H[tri(k, l)]
    return M


def lambda_of(H, C, reg, floor=LAMBDA_FLOOR):
    """lambda [V] = reg trace(H) / C + floor."""
    trace = H[tri(0, 0)].clone()
    for k in range(1, C):
        trace = trace + H[tri(k, k)]
    return float(reg) * trace / float(C) + float(floor)


def objective_of(H, xbar, lam, x):
    """x^T H x + lam |x - xbar|^2 per vertex for weights x [C,V] on the candidates (float64)."""
    C = xbar.shape[0]
    M = full_matrix(H, C)
    xv = x.double().t()
    return torch.einsum('vk,vkl,vl->v', xv, M, xv) + lam * ((xv - xbar.t()) ** 2).sum(1)


def scatter_weights(joints, weights, cands):
    """joints / weights [V,K] as weights x [C,V] on the candidates `cands` [V,C]; a joint that is no candidate raises."""
    V, C = cands.shape
    x = torch.zeros((V, C), dtype=torch.float64, device=cands.device)
    for s in range(joints.shape[1]):
        hit = cands == joints[:, s:s + 1]
        used = weights[:, s] != 0
        if bool((used & ~hit.any(1)).any()):
            raise ValueError("scatter_weights: a weighted joint is not among the vertex's candidates")
        first = hit & (hit.cumsum(1) == 1)
        x += first.double() * torch.where(used, weights[:, s].double(), weights.new_zeros(()).double())[:, None]
    return x.t().contiguous()


def _round_weights(x):
    """float32 weights [V,C] of float64 x [V,C] whose sum is 1: the largest takes what the rounding left."""
    w32 = x.float()
    left = 1. - w32.double().sum(1)                  # (the kernel subtracts in ascending candidate order; the entries are exact in double)
    big = x.argmax(1, keepdim=True)                  # (the first of equal values)
    fixed = (torch.gather(w32, 1, big).double() + left[:, None]).float()
    return w32.scatter(1, big, fixed)


def _pack(x, mask, cands, K):
    """joints / weights [V,K] of x [V,C] float32 and the chosen masks: the chosen candidates in ascending order, then joint 0, weight 0."""
    V, C = x.shape
    chosen = ((mask[:, None] >> torch.arange(C, device=x.device)[None, :]) & 1).bool()
    order = torch.sort((~chosen).to(torch.int8), dim=1, stable=True)[1][:, :K]
    keep = torch.gather(chosen, 1, order)
    weights = torch.where(keep, torch.gather(x, 1, order), x.new_zeros(()))
    joints = torch.where(keep & (weights > 0.), torch.gather(cands, 1, order), torch.zeros_like(order, dtype=torch.int32))
    return joints.to(torch.int32).contiguous(), weights.contiguous()


def _fallback(xbar_v, K):
    """(x [V,C] float64, mask [V]) without a search: the K largest xbar (a tie to the lower candidate), renormalised."""
    V, C = xbar_v.shape
    clean = torch.where(torch.isnan(xbar_v), torch.full_like(xbar_v, -float('inf')), xbar_v)
    order = torch.sort(clean, dim=1, descending=True, stable=True)[1][:, :K]
    chosen = torch.zeros((V, C), dtype=torch.bool, device=xbar_v.device).scatter(1, order, True)
    pos = torch.where(chosen & (xbar_v > 0.), xbar_v, torch.zeros_like(xbar_v))
    total = pos.sum(1, keepdim=True)
    usable = torch.isfinite(total) & (total > 0.)
    first = chosen & (chosen.cumsum(1) == 1)
    x = torch.where(usable, pos / torch.where(usable, total, torch.ones_like(total)), first.double())
    mask = (chosen.long() << torch.arange(C, device=xbar_v.device)[None, :]).sum(1)
    return x, mask


def solve(H, xbar, cands, K=4, reg=1e-6, method="fused", floor=LAMBDA_FLOOR):
    """Per vertex the minimiser of x^T H x + lambda |x - xbar|^2 over x >= 0, sum x = 1 with at most K non-zeros among the C
    candidates -> {'joints' [V,K] int32, 'weights' [V,K] float32 (sum 1; unused slots joint 0, weight 0), 'objective' [V] float64,
    'mask' [V] int32, 'lambda' [V] float64}.  H [36,V] float64, xbar [C,V] float64, cands [V,C] int32."""
    _check_method(method)
    _lib.require_gpu(H, xbar, cands)
    if xbar.dim() != 2 or cands.dim() != 2 or xbar.shape[1] != cands.shape[0] or xbar.shape[0] != cands.shape[1] or cands.shape[0] == 0:
        raise ValueError(f"solve: xbar [C,V] and cands [V,C] expected, got {tuple(xbar.shape)} and {tuple(cands.shape)}")
    C, V = xbar.shape
    _check_counts(C, K)
    K = int(K)
    if tuple(H.shape) != (TRI, V) or H.dtype != torch.float64 or xbar.dtype != torch.float64 or cands.dtype != torch.int32:
        raise ValueError(f"solve: H [{TRI},{V}] float64, xbar float64 and cands int32 expected")
    if not (float(reg) >= 0. and float(reg) < float('inf') and 0. < float(floor) < float('inf')):
        raise ValueError(f"solve: reg >= 0 and floor > 0, both finite, expected, got {reg} and {floor}")
    H, xbar, cands = H.contiguous(), xbar.contiguous(), cands.contiguous()
    dev = H.device
    if method == "fused":
        joints = torch.empty((V, K), dtype=torch.int32, device=dev)
        weights = torch.empty((V, K), dtype=torch.float32, device=dev)
        objective = torch.empty((V,), dtype=torch.float64, device=dev)
        mask = torch.empty((V,), dtype=torch.int32, device=dev)
        lam = torch.empty((V,), dtype=torch.float64, device=dev)
        _lib.launch("sr_skinfit_solve", H, H, xbar, cands, V, C, K, float(reg), float(floor), joints, weights, objective, mask, lam)
        return {'joints': joints, 'weights': weights, 'objective': objective, 'mask': mask, 'lambda': lam}
    lam = lambda_of(H, C, reg, floor)
    M = full_matrix(H, C)
    xb = xbar.t().contiguous()
    finite = torch.isfinite(H[:tri(C - 1, C - 1) + 1].sum(0) + xbar.sum(0)) & torch.isfinite(lam)
    Ms = torch.where(finite[:, None, None], M, torch.zeros_like(M))
    ls = torch.where(finite, lam, torch.ones_like(lam))
    xs = torch.where(finite[:, None], xb, torch.zeros_like(xb))
    eye = torch.eye(C, dtype=torch.float64, device=dev)
    best_obj = torch.full((V,), float('inf'), dtype=torch.float64, device=dev)
    best_x = torch.zeros((V, C), dtype=torch.float64, device=dev)
    best_mask = torch.zeros((V,), dtype=torch.int64, device=dev)
    best_count = torch.zeros((V,), dtype=torch.int64, device=dev)
    for m in range(1, 1 << C):
        count = bin(m).count("1")
        if count > K:
            continue
        inside = torch.tensor([(m >> k) & 1 for k in range(C)], dtype=torch.float64, device=dev)
        both = inside[:, None] * inside[None, :]
        system = (Ms + ls[:, None, None] * eye) * both + eye * (1. - inside)[None, :, None]
        L, info = torch.linalg.cholesky_ex(system)
        rhs = torch.stack([ls[:, None] * xs * inside, inside.expand(V, C)], 2)
        sol = torch.cholesky_solve(rhs, L)
        u, w = sol[..., 0], sol[..., 1]
        nu = (u.sum(1) - 1.) / w.sum(1)
        x = (u - nu[:, None] * w) * inside
        obj = torch.einsum('vk,vkl,vl->v', x, Ms, x) + ls * ((x - xs) ** 2).sum(1)
        ok = (info == 0) & ~(x < 0.).any(1) & torch.isfinite(obj)
        take = ok & ((obj < best_obj) | ((obj == best_obj) & (count < best_count)))
        best_obj = torch.where(take, obj, best_obj)
        best_x = torch.where(take[:, None], x, best_x)
        best_mask = torch.where(take, torch.full_like(best_mask, m), best_mask)
        best_count = torch.where(take, torch.full_like(best_count, count), best_count)
    fx, fmask = _fallback(xb, K)
    best_x = torch.where(finite[:, None], best_x, fx)
    best_mask = torch.where(finite, best_mask, fmask)
    best_obj = torch.where(finite, best_obj, torch.full_like(best_obj, float('nan')))
    joints, weights = _pack(_round_weights(best_x), best_mask, cands, K)
    return {'joints': joints, 'weights': weights, 'objective': best_obj, 'mask': best_mask.to(torch.int32), 'lambda': lam}
