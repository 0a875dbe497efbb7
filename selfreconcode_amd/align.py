"""Rigid and similarity alignment of a mesh onto another by point-to-plane ICP on the GPU (csrc/icp.hip): GPU tensors
only, no autograd.  `icp_align` estimates T(p) = s R p + t that takes `pred` onto `gt`; `evaluate.surface_metrics(..., align=...)` and
`python -m selfreconcode_amd.evaluate --align ...` use it.

ICP is a local method: it converges from a start in which most samples already find the right part of the target (rotations of some
tens of degrees on a body-like shape).  The default start only matches centroids (and sizes, with `scale`).  For a larger rotation --
another up axis, a scan facing the other way -- `init="axes"` / `init="search"` put a deterministic coarse-to-fine rotation search in
front: every rotation of a fixed table about the matched centroids gets a symmetric truncated score in one launch per
direction (sr_icp_score), the best few are refined by short ICP runs, and the ordinary ICP starts from the best of those.  An `init`
matrix is taken as it is.  Either mesh may be a surfdist_ops.Surface, which prepares it once and keeps its grid: pred is prepared once
per call (the search's reverse direction uses the same Surface), gt's grid is the caller's to keep (icp_index).  Out of scope: partial
overlap and outlier-robust registration, reflections, non-rigid alignment, point-to-point and symmetric ICP objectives, quantile trimming."""
from dataclasses import dataclass
import itertools

import numpy as np
import torch

from . import _lib
from . import surfdist_ops as sd

MAX_BLOCKS, COLS, HISTORY, STATE, DONE = _lib.SR_ICP_MAX_BLOCKS, _lib.SR_ICP_COLS, _lib.SR_ICP_HISTORY, _lib.SR_ICP_STATE, _lib.SR_ICP_DONE
TABLE = 12                                                            # doubles per candidate transform of sr_icp_score: M (row major), t
INIT_BOUND = 1e-6                                                     # |M M^T / s^2 - I| of an `init` matrix (a float32 matrix passes)
INITS = ("centroid", "none", "axes", "search")
SUPER_FIBONACCI_PSI = 1.533751168755204288118041                      # the root of psi^4 = psi + 4 of the super-Fibonacci spiral


def blocks_of(samples):
    """The block count of sr_icp_accumulate for `samples` samples: fixed from the count alone."""
    return min((int(samples) + 255) // 256, MAX_BLOCKS)


def transform_points(M, t, points):
    """fl32(((M0 px + M1 py) + M2 pz) + t) per row, in double: points [P,3] under T(p) = M p + t (M [3,3], t [3] float64 tensors on the
    points' device), in the operation order of sr_icp_accumulate."""
    p = points.double()
    cols = [((M[i, 0] * p[:, 0] + M[i, 1] * p[:, 1]) + M[i, 2] * p[:, 2]) + t[i] for i in range(3)]
    return torch.stack(cols, 1).float()


@dataclass
class Alignment:
    """T(p) = scale rotation p + translation as `matrix` [4,4] float64 (numpy), and how the iteration went: `iterations` solves ran
    before the update fell below `tol` (`converged`) or the launches ran out, `rank` unknowns were constrained by the data at the last
    of them, `pairs` samples are within `max_dist` under the result, `rms_before` / `rms_after` is the rms distance of the kept pairs
    under the initial / final transform, `history` [iters, 6] = (kept pairs, rms, max |xi|, rank, scale, done) per launched solve.
    `search` is set when a rotation search chose the start (init "axes" / "search"): `kind`, `candidates` (N of the table), `top`
    (the indices of the refined candidates, best raw score first), `score` / `refined` (their J before and after refinement),
    `winner` (its index in the table) and `angle_deg`, the rotation angle of the winner's refined transform from the centroid start."""
    matrix: np.ndarray
    scale: float
    rotation: np.ndarray
    translation: np.ndarray
    iterations: int
    converged: bool
    rank: int
    pairs: int
    rms_before: float
    rms_after: float
    history: np.ndarray
    search: dict | None = None

    def apply(self, verts):
        """verts [V,3] (GPU tensor) under the transform, as float32: the double product, rounded once."""
        _lib.require_gpu(verts)
        if verts.dim() != 2 or verts.shape[1] != 3:
            raise ValueError(f"verts [V,3] expected, got {tuple(verts.shape)}")
        m = torch.from_numpy(np.ascontiguousarray(self.matrix)).to(verts.device)
        return transform_points(m[:3, :3], m[:3, 3], verts.detach())

    def summary(self):
        """What the metrics carry as `alignment`: plain Python values."""
        out = {"matrix": self.matrix.tolist(), "scale": self.scale, "iterations": self.iterations, "converged": self.converged,
               "rank": self.rank, "rms_before": self.rms_before, "rms_after": self.rms_after}
        if self.search is not None:
            out["search"] = dict(self.search)
        return out


def check_init(init):
    """(M [3,3], t [3]) float64 of a 4 x 4 similarity matrix.  ValueError unless it is finite, its last row is (0, 0, 0, 1), M M^T =
    s^2 I with every entry of M M^T / s^2 - I within INIT_BOUND, and det M > 0 (no reflection, no shear, no anisotropic scale)."""
    m = np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init, np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError("init: a finite 4 x 4 matrix expected")
    if not np.array_equal(m[3], [0., 0., 0., 1.]):
        raise ValueError("init: the last row must be (0, 0, 0, 1)")
    M = m[:3, :3]
    g = M @ M.T
    s2 = np.trace(g) / 3.
    if not s2 > 0 or np.abs(g / s2 - np.eye(3)).max() > INIT_BOUND or not np.linalg.det(M) > 0:
        raise ValueError(f"init: not a similarity (M M^T = s^2 I within {INIT_BOUND:g} and det > 0 expected)")
    return M.copy(), m[:3, 3].copy()


def frame_of(index):
    """((ox, oy, oz), rho) as Python floats: the centre and the half diagonal of the box of the vertices of `index` (a MeshIndex or a
    Surface: its `box`; rho = 1 for a mesh that is one point)."""
    box = index.box.astype(np.float64)
    o = 0.5 * (box[:3] + box[3:])
    rho = 0.5 * float(np.sqrt(((box[3:] - box[:3]) ** 2).sum()))
    return (float(o[0]), float(o[1]), float(o[2])), rho if rho > 0 else 1.


def accumulate(points, index, state, frame, max_dist, partial, measure=False):
    """One launch of sr_icp_accumulate: points [S,3] float32 against `index` under `state` [16] float64 -> partial [blocks, 40]."""
    S = points.shape[0]
    if partial.shape != (blocks_of(S), COLS) or partial.dtype != torch.float64 or not partial.is_contiguous():
        raise ValueError(f"partial [{blocks_of(S)}, {COLS}] float64 expected")
    o, rho = frame
    _lib.launch("sr_icp_accumulate", points, points, S, *index.args(), state, o[0], o[1], o[2], rho, float(max_dist), int(bool(measure)), partial,
                partial.shape[0])


def solve(partial, frame, scale, tol, it, iters, state, history):
    """One launch of sr_icp_solve: partial [blocks, 40] -> state [16], row `it` of history [iters, 6]."""
    if history.shape != (iters, HISTORY) or history.dtype != torch.float64 or not history.is_contiguous():
        raise ValueError(f"history [{iters}, {HISTORY}] float64 expected")
    o, rho = frame
    _lib.launch("sr_icp_solve", partial, partial, partial.shape[0], o[0], o[1], o[2], rho, int(bool(scale)), float(tol), int(it), int(iters), state,
                history)


def rotation_candidates(kind, n=None):
    """[N,3,3] float64 (numpy): the rotations a search tries, in the order that breaks ties.

    "axes": the 24 proper rotations of the cube -- the signed permutation matrices with row i = sign_i e_perm(i), in the order of
    itertools.permutations(range(3)) x itertools.product((1, -1), repeat=3), those of determinant +1; the identity is the first
    (`n` is not used).  "search": those 24, then `n` super-Fibonacci rotations: for i < n, t = i + 1/2, r = sqrt(t / n), R = sqrt(1 -
    t / n), alpha = 2 pi t / sqrt 2, beta = 2 pi t / psi (psi^4 = psi + 4), the unit quaternion (w, x, y, z) = (R cos beta, r sin
    alpha, r cos alpha, R sin beta), normalised, as a matrix."""
    if kind not in ("axes", "search"):
        raise ValueError(f"kind must be 'axes' or 'search', got {kind!r}")
    cube = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            m = np.zeros((3, 3))
            for i in range(3):
                m[i, perm[i]] = signs[i]
            if np.linalg.det(m) > 0:
                cube.append(m)
    cube = np.stack(cube)
    if kind == "axes":
        return cube
    if n is None or int(n) != n or int(n) <= 0:
        raise ValueError(f"rotation_candidates: n > 0 expected, got {n!r}")
    n = int(n)
    t = np.arange(n, dtype=np.float64) + 0.5
    r, R = np.sqrt(t / n), np.sqrt(1. - t / n)
    alpha, beta = 2. * np.pi * t / np.sqrt(2.), 2. * np.pi * t / SUPER_FIBONACCI_PSI
    q = np.stack([R * np.cos(beta), r * np.sin(alpha), r * np.cos(alpha), R * np.sin(beta)], 1)
    a, x, y, z = (q / np.sqrt((q * q).sum(1, keepdims=True))).T
    spiral = np.stack([a * a + x * x - y * y - z * z, 2 * x * y - 2 * a * z, 2 * a * y + 2 * x * z,
                       2 * a * z + 2 * x * y, a * a - x * x + y * y - z * z, 2 * y * z - 2 * a * x,
                       2 * x * z - 2 * a * y, 2 * a * x + 2 * y * z, a * a - x * x - y * y + z * z], 1).reshape(n, 3, 3)
    return np.concatenate([cube, spiral])


def score_candidates(points, index, table, trunc):
    """One launch of sr_icp_score: score [N,2] float64 = per candidate transform T_c(p) = M p + t of table [N,12] float64 (M row major,
    then t) the sum of min(d(T_c p, mesh of `index`), trunc[c])^2 over the samples points [S,3] float32 whose image is finite, and
    their number.  trunc [N] float32.  Two launches give identical bits."""
    _lib.require_gpu(points, table, trunc)
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0 or points.dtype != torch.float32 or not points.is_contiguous():
        raise ValueError(f"points [S,3] float32 with S > 0 expected, got {tuple(points.shape)} {points.dtype}")
    N = table.shape[0] if table.dim() == 2 else 0
    if N == 0 or table.shape != (N, TABLE) or table.dtype != torch.float64 or not table.is_contiguous():
        raise ValueError(f"table [N,{TABLE}] float64 with N > 0 expected, got {tuple(table.shape)} {table.dtype}")
    if trunc.shape != (N,) or trunc.dtype != torch.float32 or not trunc.is_contiguous():
        raise ValueError(f"trunc [{N}] float32 expected, got {tuple(trunc.shape)} {trunc.dtype}")
    score = torch.empty((N, 2), dtype=torch.float64, device=points.device)
    _lib.launch("sr_icp_score", points, points, points.shape[0], table, N, *index.args(), trunc, score)
    return score


def _centroids(p, g, scale):
    """(c_p, c_g, s) on the device: the centroids of the samples, and the ratio of the rms radii about them when `scale` (else 1)."""
    p, g = p.double(), g.double()
    cp, cg = p.mean(0), g.mean(0)
    s = torch.ones((), dtype=torch.float64, device=p.device)
    if scale:
        s = ((g - cg).pow(2).sum(1).mean() / (p - cp).pow(2).sum(1).mean()).sqrt()
    return cp, cg, s


def _centroid_init(p, g, scale):
    """(M, t) on the device: the sample centroid of pred onto that of gt, with the ratio of the rms radii about them when `scale`."""
    cp, cg, s = _centroids(p, g, scale)
    return s * torch.eye(3, dtype=torch.float64, device=p.device), cg - s * cp


def _iterate(p, index, frame, M, t, iters, scale, max_dist, tol):
    """`iters` iterations (two launches each) from T(p) = M p + t -> (the samples in the order they were summed in, buf = state [16]
    and history [iters, 6] in one tensor, the last partial sums).  Nothing is read back."""
    dev = p.device
    buf = torch.zeros((STATE + iters * HISTORY,), dtype=torch.float64, device=dev)         # state and history: one copy to the host
    state, history = buf[:STATE], buf[STATE:].view(iters, HISTORY)
    state[:9] = M.reshape(9)
    state[9:12] = t
    # a wave walks neighbouring cells: the samples in the order of their cell keys under the initial transform (part of the sums' definition)
    p = sd.in_key_order(p, index.keys(transform_points(M, t, p)))[0]
    partial = torch.zeros((blocks_of(p.shape[0]), COLS), dtype=torch.float64, device=dev)
    for it in range(iters):
        accumulate(p, index, state, frame, max_dist, partial)
        solve(partial, frame, scale, tol, it, iters, state, history)
    return p, buf, partial


def _in_cell_order(points, index):
    """points in the order of their cell keys in the grid of `index` (stable)."""
    return sd.in_key_order(points, index.keys(points))[0]


def symmetric_score(P, G, index, index_pred, M, t, max_dist):
    """J [K] float64 of the transforms T_c(p) = M_c p + t_c (M [K,3,3], t [K,3] float64 on the device), DESIGN.md 3.22: the mean of
    min(d(T_c P_i, gt), tau)^2 plus s_c^2 times the mean of min(d(T_c^-1 G_j, pred), tau / s_c)^2, each over the samples whose image is
    finite, +Inf when either direction keeps none.  s_c^2 = |M_c|_F^2 / 3, T_c^-1(g) = M_c^T / s_c^2 g - M_c^T / s_c^2 t_c.  P / G:
    samples of pred / gt, each in the cell order of its own mesh's grid; index / index_pred: the MeshIndex of gt / pred.  Two launches."""
    K = M.shape[0]
    s2 = (M * M).sum((1, 2)) / 3.
    inverse = M.transpose(1, 2) / s2[:, None, None]
    back = -(inverse @ t[:, :, None])[:, :, 0]
    there = score_candidates(P, index, torch.cat([M.reshape(K, 9), t], 1).contiguous(),
                             torch.full((K,), max_dist, dtype=torch.float32, device=M.device))
    here = score_candidates(G, index_pred, torch.cat([inverse.reshape(K, 9), back], 1).contiguous(), (max_dist / s2.sqrt()).float().contiguous())
    J = there[:, 0] / there[:, 1] + s2 * (here[:, 0] / here[:, 1])
    return torch.where((there[:, 1] > 0) & (here[:, 1] > 0) & ~torch.isnan(J), J, torch.full_like(J, float("inf")))


def _search(kind, pred, index, frame, seed, scale, max_dist, tol, candidates, search_samples, top, refine_iters):
    """The rotation search of DESIGN.md 3.22 for the Surface `pred` -> (M [3,3], t [3], record) on the device: the refined transform of
    the winner, and record = (top indices [K], their J [K], their refined J [K], the winner's position in top, its refined M and t
    [12]) as one float64 tensor.  The reverse direction walks pred.grid(); its pair total is the only read."""
    index_pred = pred.grid()
    P = pred.sample(search_samples, seed)[0]
    G = sd._sample(index.tri, index.cum_area, search_samples, seed + 1)[0]
    cp, cg, s = _centroids(P, G, scale)
    P, G = _in_cell_order(P, index_pred), _in_cell_order(G, index)
    M = s * torch.from_numpy(rotation_candidates(kind, candidates)).to(P.device)
    t = cg - (M @ cp)
    K = min(top, M.shape[0])
    J = symmetric_score(P, G, index, index_pred, M, t, max_dist)
    best = torch.sort(J, stable=True)[1][:K]                                              # ties: the lower index
    starts_M, starts_t = M.index_select(0, best), t.index_select(0, best)
    refined = torch.stack([_iterate(P, index, frame, starts_M[k], starts_t[k], refine_iters, scale, max_dist, tol)[1][:TABLE] for k in range(K)])
    J_refined = symmetric_score(P, G, index, index_pred, refined[:, :9].reshape(K, 3, 3), refined[:, 9:12].contiguous(), max_dist)
    winner = torch.sort(J_refined, stable=True)[1][:1]                                    # of equal values, the first
    state = refined.index_select(0, winner)[0]
    return state[:9].reshape(3, 3), state[9:12], torch.cat([best.double(), J.index_select(0, best), J_refined, winner.double(), state])


def _search_record(kind, N, K, rec):
    """Alignment.search from the host copy of _search's record."""
    top, winner, M = [int(v) for v in rec[:K]], int(rec[3 * K]), rec[3 * K + 1:3 * K + 10].reshape(3, 3)
    s = np.sqrt((M * M).sum() / 3.)
    cos = (np.trace(M) / s - 1.) / 2. if s > 0 and np.isfinite(s) else np.nan
    return {"kind": kind, "candidates": N, "top": top, "score": [float(v) for v in rec[K:2 * K]], "refined": [float(v) for v in rec[2 * K:3 * K]],
            "winner": top[winner], "angle_deg": float(np.degrees(np.arccos(np.clip(cos, -1., 1.))))}


def icp_index(pred, index, samples=100_000, seed=0, iters=30, scale=False, max_dist=None, tol=2. ** -23, init="centroid", candidates=4096,
              search_samples=4096, top=8, refine_iters=10):
    """icp_align against a MeshIndex of the target that the caller already has; pred, a Surface or a pair, is prepared once."""
    samples, iters, tol = int(samples), int(iters), float(tol)
    if samples <= 0 or iters <= 0:
        raise ValueError(f"samples > 0 and iters > 0 expected, got {samples} and {iters}")
    if not tol >= 0:
        raise ValueError(f"tol >= 0 expected, got {tol}")
    max_dist = float(np.float32(np.inf if max_dist is None else max_dist))
    if not max_dist >= 0:
        raise ValueError(f"max_dist >= 0 expected, got {max_dist}")
    candidates, search_samples, top, refine_iters = int(candidates), int(search_samples), int(top), int(refine_iters)
    if candidates <= 0 or search_samples <= 0 or top <= 0 or refine_iters <= 0:
        raise ValueError(f"candidates, search_samples, top and refine_iters > 0 expected, got {candidates}, {search_samples}, {top} and {refine_iters}")
    fixed = None if isinstance(init, str) else check_init(init)
    if fixed is None and init not in INITS:
        raise ValueError(f"init must be 'centroid', 'none', 'axes', 'search' or a 4 x 4 matrix, got {init!r}")
    pred = sd.Surface.of(pred, "icp_align")
    dev = pred.verts.device
    for name, area in (("pred", pred.area), ("gt", index.area)):
        if not (area > 0 and np.isfinite(area)):
            raise ValueError(f"icp_align: the {name} mesh has total area {area}")
    frame = frame_of(index)
    p = pred.sample(samples, seed)[0]
    record = torch.zeros((0,), dtype=torch.float64, device=dev)
    if fixed is not None:
        M, t = torch.from_numpy(fixed[0]).to(dev), torch.from_numpy(fixed[1]).to(dev)
    elif init == "centroid":
        M, t = _centroid_init(p, sd._sample(index.tri, index.cum_area, samples, seed + 1)[0], scale)
    elif init == "none":
        M, t = torch.eye(3, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
    else:
        M, t, record = _search(init, pred, index, frame, seed, scale, max_dist, tol, candidates, search_samples, top, refine_iters)
    p, buf, partial = _iterate(p, index, frame, M, t, iters, scale, max_dist, tol)
    accumulate(p, index, buf[:STATE], frame, max_dist, partial, measure=True)             # the kept pairs under the result
    host = torch.cat([buf, partial[:, 36:38].sum(0), record]).cpu().numpy()
    state_h, hist, last = host[:STATE], host[STATE:STATE + iters * HISTORY].reshape(iters, HISTORY).copy(), host[STATE + iters * HISTORY:][:2]
    matrix = np.eye(4)
    matrix[:3, :3], matrix[:3, 3] = state_h[:9].reshape(3, 3), state_h[9:12]
    if not np.isfinite(matrix).all():
        raise ValueError("icp_align: the transform is not finite")
    s = float(np.sqrt((matrix[:3, :3] ** 2).sum() / 3.))
    iterations = int(state_h[DONE + 1])
    pairs = int(last[0])
    search = None
    if record.shape[0]:
        N = 24 if init == "axes" else 24 + candidates
        search = _search_record(init, N, min(top, N), host[STATE + iters * HISTORY + 2:])
    return Alignment(matrix=matrix, scale=s, rotation=matrix[:3, :3] / s, translation=matrix[:3, 3].copy(), iterations=iterations,
                     converged=bool(state_h[DONE] != 0.), rank=int(hist[iterations - 1, 3]), pairs=pairs, rms_before=float(hist[0, 1]),
                     rms_after=float(np.sqrt(last[1] / pairs)) if pairs else 0., history=hist, search=search)


def icp_align(pred, gt, samples=100_000, seed=0, iters=30, scale=False, max_dist=None, tol=2. ** -23, init="centroid", candidates=4096,
              search_samples=4096, top=8, refine_iters=10):
    """The Alignment that takes pred = (verts [V,3], faces [F,3]) onto gt, GPU tensors (each a pair or a surfdist_ops.Surface, whose
    grid is then used and kept): point-to-plane ICP of `samples` surface samples of pred (surfdist_ops.sample_surface with `seed`)
    against the mesh gt, rigid, or a similarity with `scale`.

    Every iteration is two launches: sr_icp_accumulate transforms the samples with the float64 state, finds every sample's closest
    point on gt (the exact float32 search of closest_point), keeps the pairs within `max_dist` (float32, `<=`; default: all) and sums
    the normal equations of the linearised point-to-plane objective in double; sr_icp_solve solves them (Cholesky; a direction the
    data does not constrain -- a plane, a sphere, a cylinder -- gets no update and lowers `rank`), composes the update with an exact
    rotation and sets a flag on the device once max |xi| < `tol`, after which the remaining launches of the `iters` return at once.
    Nothing is read back inside the loop; the result comes to the host in one copy.  Two calls give identical bits.

    `init`: "centroid" (the area-weighted sample centroid of pred onto that of gt, samples with `seed` and `seed + 1`; with `scale`
    also the ratio of the rms radii), "none", a 4 x 4 similarity matrix (check_init), or a rotation search in front of the ICP
     for a pred in any orientation: "axes" tries the 24 rotations of the cube about the matched centroids, "search"
    those and `candidates` super-Fibonacci rotations (rotation_candidates).  Every candidate gets the symmetric score J (symmetric_score:
    `search_samples` samples of each mesh, truncated at `max_dist`); the `top` candidates of lowest J (at most all of them) run
    `refine_iters` ICP iterations on the search samples and are scored again; the ICP proper starts from the lowest refined J.  Ties go
    to the lower index.  `Alignment.search` records the choice.  ICP itself is local: with "centroid", a large rotation ends in a
    converged, wrong alignment.  ValueError for a mesh without area, and RuntimeError for CPU tensors."""
    gt = sd.Surface.of(gt, "MeshIndex.build")
    return icp_index(pred, gt.grid(), samples, seed, iters, scale, max_dist, tol, init, candidates, search_samples, top, refine_iters)
