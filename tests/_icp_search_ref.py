"""Numpy restatement of the rotation search in front of the ICP (selfreconcode_amd.align `init="axes" | "search"`, sr_icp_score; DESIGN.md
3.22), written from the stated semantics in float64 on top of `_icp_ref.icp(points=..., init=...)`, `_icp_ref.samples_of` and
`_surfdist_ref.closest`.  It does not mirror the kernel's order of operations or of summation; the tests compare through bounds.

The cases: the test shape of `_icp_ref` under (s0, R0, t0) with rotations far outside the basin of the centroid start."""
import itertools
import math

import numpy as np

import _icp_ref as ir
import _surfdist_ref as sr

PSI = 1.533751168755204288118041
T0 = (0.3, -0.2, 0.4)
CYCLE = np.float64([[0, 0, 1], [1, 0, 0], [0, 1, 0]])
# name -> (s0, rotation, similarity?)
CASES = {"flip170_sim": (1.08, ((1., -2., 0.5), 170.), True), "flip170_rigid": (1., ((1., -2., 0.5), 170.), False),
         "axes_cyc12": (1., ((0.2, 1., -0.3), 12.), False), "tilt100": (0.9, ((-1., 0.4, 2.), 100.), True)}


def _axis_angle(axis, deg):
    return ir.exp_rotation(np.deg2rad(deg) * np.float64(axis) / np.linalg.norm(axis))


def case(name, n=6):
    """(pred, gt, (s0, R0, t0), scale?) of a named case on shape(n), built like `_icp_ref.case`."""
    s0, (axis, deg), scale = CASES[name]
    R0 = _axis_angle(axis, deg)
    if name == "axes_cyc12":
        R0 = R0 @ CYCLE
    t0 = np.float64(T0)
    v, f = ir.shape(n)
    pred = ((v.astype(np.float64) - t0) @ R0 / s0).astype(np.float32)
    return (pred, f), (v, f), (s0, R0, t0), scale


def cube_rotations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            m = np.zeros((3, 3))
            for i in range(3):
                m[i, perm[i]] = signs[i]
            if np.linalg.det(m) > 0:
                out.append(m)
    return np.float64(out)


def super_fibonacci(n):
    out = []
    for i in range(n):
        t = i + 0.5
        r, R = math.sqrt(t / n), math.sqrt(1. - t / n)
        alpha, beta = 2. * math.pi * t / math.sqrt(2.), 2. * math.pi * t / PSI
        a, x, y, z = R * math.cos(beta), r * math.sin(alpha), r * math.cos(alpha), R * math.sin(beta)
        norm = math.sqrt(a * a + x * x + y * y + z * z)
        a, x, y, z = a / norm, x / norm, y / norm, z / norm
        out.append([[a * a + x * x - y * y - z * z, 2 * x * y - 2 * a * z, 2 * a * y + 2 * x * z],
                    [2 * a * z + 2 * x * y, a * a - x * x + y * y - z * z, 2 * y * z - 2 * a * x],
                    [2 * x * z - 2 * a * y, 2 * a * x + 2 * y * z, a * a - x * x - y * y + z * z]])
    return np.float64(out)


def rotation_candidates(kind, n=None):
    return cube_rotations() if kind == "axes" else np.concatenate([cube_rotations(), super_fibonacci(n)])


def nearest_angle_deg(rotations, probes=4000, seed=1):
    """The largest angle (degrees) from `probes` random rotations (normalised normal 4-vectors of default_rng(seed)) to the nearest of
    `rotations` [N,3,3]: cos(angle) = (trace(A^T B) - 1) / 2."""
    q = np.random.default_rng(seed).normal(size=(probes, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, x, y, z = q.T
    A = np.stack([a * a + x * x - y * y - z * z, 2 * x * y - 2 * a * z, 2 * a * y + 2 * x * z, 2 * a * z + 2 * x * y, a * a - x * x + y * y - z * z,
                  2 * y * z - 2 * a * x, 2 * x * z - 2 * a * y, 2 * a * x + 2 * y * z, a * a - x * x - y * y + z * z], 1)
    cos = (A @ rotations.reshape(-1, 9).T - 1.) / 2.
    return float(np.degrees(np.arccos(np.clip(cos.max(1), -1., 1.))).max())


def scores(P, G, pred, gt, Ms, ts, tau=np.inf):
    """J [K] of T_c(p) = Ms[c] p + ts[c]: mean min(d(T P, gt), tau)^2 + s^2 mean min(d(T^-1 G, pred), tau / s)^2, each mean over the
    finite images, +inf when a direction has none.  (One closest-point call per direction over all candidates' images.)"""
    Ms, ts = np.float64(Ms), np.float64(ts)
    s = np.sqrt((Ms * Ms).sum((1, 2)) / 3.)
    inv = Ms.transpose(0, 2, 1) / (s * s)[:, None, None]
    back = -np.einsum("kij,kj->ki", inv, ts)
    means = []
    for pts, mesh, A, b, cap in ((P, gt, Ms, ts, np.full(len(s), tau)), (G, pred, inv, back, tau / s)):
        q = (np.einsum("kij,nj->kni", A, pts.astype(np.float64)) + b[:, None]).astype(np.float32)
        ok = np.isfinite(q).all(2)
        d = np.zeros(ok.shape)
        d[ok] = sr.closest(q[ok], mesh[0], mesh[1])[0]
        e2 = np.where(ok, np.minimum(d, cap[:, None]) ** 2, 0.)
        with np.errstate(invalid="ignore", divide="ignore"):
            means.append(np.where(ok.any(1), e2.sum(1) / ok.sum(1), np.inf))
    return means[0] + s * s * means[1]


def search(pred, gt, kind, seed=0, scale=False, max_dist=np.inf, tol=ir.TOL, candidates=4096, search_samples=4096, top=8, refine_iters=10):
    """Steps 1-4: dict(start [4,4]: the winner's refined transform, top, score, refined, winner)."""
    P, G = ir.samples_of(pred, search_samples, seed), ir.samples_of(gt, search_samples, seed + 1)
    p64, g64 = P.astype(np.float64), G.astype(np.float64)
    cp, cg = p64.mean(0), g64.mean(0)
    s = np.sqrt(((g64 - cg) ** 2).sum(1).mean() / ((p64 - cp) ** 2).sum(1).mean()) if scale else 1.
    rotations = rotation_candidates(kind, candidates)
    J = scores(P, G, pred, gt, s * rotations, cg - s * (rotations @ cp), max_dist)
    best = np.argsort(J, kind="stable")[:min(top, len(rotations))]
    starts = []
    for c in best:
        init = np.eye(4)
        init[:3, :3], init[:3, 3] = s * rotations[c], cg - s * (rotations[c] @ cp)
        starts.append(ir.icp(pred, gt, search_samples, seed, refine_iters, scale, max_dist, tol, init=init, points=P)["matrix"])
    starts = np.float64(starts)
    refined = scores(P, G, pred, gt, starts[:, :3, :3], starts[:, :3, 3], max_dist)
    w = int(np.argsort(refined, kind="stable")[0])
    return {"start": starts[w], "top": [int(c) for c in best], "score": J[best].tolist(), "refined": refined.tolist(), "winner": int(best[w])}


def align(pred, gt, kind, samples, seed=0, iters=30, scale=False, max_dist=np.inf, tol=ir.TOL, dtype=np.float64, found=None, **search_opts):
    """Steps 1-5: the search (or `found`, an earlier result of it), then `_icp_ref.icp` from the winner's transform."""
    found = found or search(pred, gt, kind, seed, scale, max_dist, tol, **search_opts)
    out = ir.icp(pred, gt, samples, seed, iters, scale, max_dist, tol, init=found["start"], dtype=dtype)
    out["search"] = found
    return out
