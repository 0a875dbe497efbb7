"""Times the ICP alignment (align.icp_align, csrc/icp.hip) on the meshes of tools/surfdist_bench.py: cube_sphere(170)
(346 800 faces) onto a jittered cube_sphere(119) x 1.05 (169 932 faces), at 10^5 and 10^6 samples.

Two things are timed.  (1) `icp_align` as a whole: the target's index build, the sampling, `iters` pairs of launches and the one copy.
(2) One iteration, the fused pair of launches (sr_icp_accumulate + sr_icp_solve) against the same iteration composed from what the
package offered before them: `closest_point`, a gather of `MeshIndex.face_normals`, the rows and their Gram matrix in torch double (one
matrix product: kinder to the composition than ten separate reductions), a copy to the host, a numpy solve and the upload of the new
state.  Both run from the same state, which is put back before every iteration (at the start, a gap of about five mean edges, and at
the converged similarity, where the surfaces touch), in alternating windows of wall time around a device synchronisation, after
seconds of warm-up (a ten-launch window measures the clock ramp, see README).

The rotation search in front of the ICP is timed on a body-size pair: the bent cube_sphere(34) of the tests (13 872
faces; a body model's mesh has 13 776, and none ships here) and its copy turned by 170 degrees, scaled and moved.  (3) The scores of
the N = 24 + 4096 = 4120 candidates for S = 4096 samples in one launch of sr_icp_score against the same scores composed from
`closest_point` in a Python loop over the candidates.  (4) The whole `icp_align(init="search")` against `init="centroid"` at the
defaults, and the search's stages on their own: the two scoring launches, the index of pred, and eight refinements of ten iterations
from the first eight rows of the table (the cube's rotations: wide gaps, the expensive regime -- where the top candidates of a real
run lie decides their cost).  The same windows after the same warm-up; the Python loop runs once per window (it takes minutes).

    python tools/icp_bench.py [--out FILE.json] [--seconds 2.0] [--windows 3] [--only {icp,search}]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selfreconcode_amd import align  # noqa: E402
from selfreconcode_amd import mesh_prep_ops as mp  # noqa: E402
from selfreconcode_amd import surfdist_ops as sd  # noqa: E402
from selfreconcode_amd.synthetic import cube_sphere  # noqa: E402

ITERS = 30


def meshes(dev):
    pv, pf = cube_sphere(170)
    gv, gf = cube_sphere(119)
    gv = (gv.numpy() + np.random.default_rng(5).normal(0., 0.004, gv.shape)).astype(np.float32) * np.float32(1.05)
    return (pv.to(dev), pf.to(dev)), (torch.from_numpy(gv).to(dev), gf.to(dev))


def wall(fn, calls):
    """ms per call of `calls` back-to-back calls, wall time around a synchronisation."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def warm(fn, seconds):
    t0, n = time.time(), 0
    while time.time() - t0 < seconds or n < 2:
        fn(); torch.cuda.synchronize(); n += 1
    return n


def host_solve(G, count, scale):
    """xi [7] of the normal equations on the host: the scaled system, numpy's solver (a singular system: least squares)."""
    nu = 7 if scale else 6
    diag = np.diag(G)[:nu]
    keep = np.flatnonzero(diag > count * 2. ** -46)
    dsc = 1. / np.sqrt(diag[keep])
    A, rhs = G[np.ix_(keep, keep)] * dsc[:, None] * dsc[None], -G[keep, 7] * dsc
    xi = np.zeros(7)
    try:
        xi[keep] = np.linalg.solve(A, rhs) * dsc
    except np.linalg.LinAlgError:
        xi[keep] = np.linalg.lstsq(A, rhs, rcond=None)[0] * dsc
    return xi


def host_update(M, t, xi, o, rho):
    w = xi[:3]
    angle = np.sqrt((w * w).sum())
    R = np.eye(3)
    if angle > 0:
        k = w / angle
        K = np.float64([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(angle) * K + (1. - np.cos(angle)) * (K @ K)
    sd_ = 1. + xi[6]
    return sd_ * (R @ M), o + sd_ * (R @ (t - o)) + rho * xi[3:6]


class Iteration:
    """One ICP iteration from a fixed state, fused and composed."""

    def __init__(self, p, index, frame, state0, scale):
        self.p, self.index, self.frame, self.scale = p, index, frame, scale
        self.state0 = state0.clone()
        self.state = state0.clone()
        self.history = torch.zeros((1, align.HISTORY), dtype=torch.float64, device=p.device)
        self.partial = torch.zeros((align.blocks_of(p.shape[0]), align.COLS), dtype=torch.float64, device=p.device)
        self.normals = index.face_normals()
        self.o = torch.tensor(frame[0], dtype=torch.float64, device=p.device)
        self.state0_h = state0.cpu().numpy()

    def fused(self):
        self.state.copy_(self.state0)
        align.accumulate(self.p, self.index, self.state, self.frame, float("inf"), self.partial)
        align.solve(self.partial, self.frame, self.scale, 0., 0, 1, self.state, self.history)

    def composed(self):
        s = self.state0_h
        state = torch.from_numpy(s).to(self.p.device)                                    # the upload of the state
        M, t = state[:9].view(3, 3), state[9:12]
        q = align.transform_points(M, t, self.p)
        dist, face, closest = sd.closest_point(q, self.index)
        n = self.normals[face].double()
        qd = q.double()
        x = (qd - self.o) / self.frame[1]
        kept = (torch.isfinite(q).all(1) & (dist <= float("inf"))).double()[:, None]
        W = torch.cat([torch.linalg.cross(x, n), n, (n * x).sum(1, keepdim=True), (n * (qd - closest.double())).sum(1, keepdim=True) / self.frame[1]], 1) * kept
        d = dist.double() * kept[:, 0]
        host = torch.cat([(W.t() @ W).reshape(-1), torch.stack([kept.sum(), (d * d).sum()])]).cpu().numpy()
        xi = host_solve(host[:64].reshape(8, 8), host[64], self.scale)
        return host_update(s[:9].reshape(3, 3), s[9:12], xi, np.float64(self.frame[0]), self.frame[1])


def body_pair(dev, n=34):
    """(pred, gt, truth [4,4]): the bent cube_sphere(n) of tests/_icp_ref.py and pred = R0^T (v - t0) / s0 with R0 170 degrees about (1,
    -2, 0.5), s0 = 1.08, t0 = (0.3, -0.2, 0.4) -- the `flip170_sim` case of the tests at a body's size."""
    v, f = cube_sphere(n)
    v = v.numpy().astype(np.float64)
    v = v * (1. + 0.25 * np.sin(3. * v[:, 0] + 1.) * np.cos(2. * v[:, 1]) + 0.2 * v[:, 2] * v[:, 0])[:, None] * np.float64([1., 0.7, 0.45])
    v = v.astype(np.float32)
    w = np.deg2rad(170.) * np.float64([1., -2., 0.5]) / np.linalg.norm([1., -2., 0.5])
    K = np.float64([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / np.deg2rad(170.)
    R0 = np.eye(3) + np.sin(np.deg2rad(170.)) * K + (1. - np.cos(np.deg2rad(170.))) * (K @ K)
    s0, t0 = 1.08, np.float64([0.3, -0.2, 0.4])
    truth = np.eye(4)
    truth[:3, :3], truth[:3, 3] = s0 * R0, t0
    pred = ((v.astype(np.float64) - t0) @ R0 / s0).astype(np.float32)
    f = f.to(dev)
    return (torch.from_numpy(pred).to(dev), f), (torch.from_numpy(v).to(dev), f), truth


def composed_scores(points, index, table, trunc):
    """score [N,2] as sr_icp_score defines it, from closest_point in a loop over the candidates."""
    out = []
    for c in range(table.shape[0]):
        q = align.transform_points(table[c, :9].view(3, 3), table[c, 9:], points)
        e = torch.minimum(sd.closest_point(q, index)[0], trunc[c]).double()
        ok = torch.isfinite(q).all(1)
        out.append(torch.stack([(e * e)[ok].sum(), ok.sum().double()]))
    return torch.stack(out)


def search_bench(dev, args):
    """(3) and (4) of the module text."""
    pred, gt, truth = body_pair(dev)
    index, index_pred = sd.MeshIndex.build(gt[0], gt[1]), sd.MeshIndex.build(pred[0], pred[1])
    S, n = 4096, 4096
    P = align._in_cell_order(sd._sample(index_pred.tri, index_pred.cum_area, S, 0)[0], index_pred)
    G = sd._sample(index.tri, index.cum_area, S, 1)[0]
    cp, cg, s = align._centroids(P, G, True)
    M = s * torch.from_numpy(align.rotation_candidates("search", n)).to(dev)
    table = torch.cat([M.reshape(-1, 9), cg - (M @ cp)], 1).contiguous()
    N = table.shape[0]
    trunc = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    one = lambda: align.score_candidates(P, index, table, trunc)  # noqa: E731
    loop = lambda: composed_scores(P, index, table, trunc)  # noqa: E731
    res = {"faces": int(gt[1].shape[0]), "candidates": N, "samples": S, "device": torch.cuda.get_device_name(0)}
    n1 = warm(one, args.seconds)
    res["score"] = {"launch_ms": [wall(one, max(3, n1))], "launch_calls": max(3, n1)}
    print(json.dumps(res), flush=True)
    a, b = one(), loop()                                                                  # (the loop's warm-up: N calls of closest_point)
    res["launch_vs_composed"] = float(((a[:, 0] - b[:, 0]).abs() / b[:, 0]).max())
    res["counts_equal"] = bool(torch.equal(a[:, 1], b[:, 1]))
    launch, composed = res["score"]["launch_ms"], []
    for _ in range(args.windows):                                                         # alternating windows; one pass of the loop each
        composed.append(wall(loop, 1))
        launch.append(wall(one, max(3, n1)))
        print(json.dumps({"composed_ms": composed[-1], "launch_ms": launch[-1]}), flush=True)
    res["score"].update({"composed_ms": composed, "composed_calls": 1, "ratio": float(np.median(composed) / np.median(launch))})
    print(json.dumps(res), flush=True)
    for init in ("centroid", "search"):
        fn = lambda: align.icp_align(pred, gt, scale=True, init=init)  # noqa: E731
        calls = warm(fn, args.seconds)
        r = fn()
        res[init] = {"align_ms": [wall(fn, max(3, calls)) for _ in range(args.windows)], "calls": max(3, calls), "iterations": r.iterations,
                     "converged": r.converged, "rms_after": r.rms_after, "error": float(np.abs(r.matrix - truth).max()), "search": r.search}
        print(json.dumps({init: res[init]}), flush=True)
    # the stages of the search on their own: the two scoring launches, and K = 8 refinements of 10 iterations from the table's first rows
    frame = align.frame_of(index)
    t = cg - (M @ cp)
    score = lambda: align.symmetric_score(P, align._in_cell_order(G, index), index, index_pred, M, t, float("inf"))  # noqa: E731
    refine = lambda: [align._iterate(P, index, frame, M[k], t[k], 10, True, float("inf"), 2. ** -23) for k in range(8)]  # noqa: E731
    build = lambda: sd.MeshIndex.build(pred[0], pred[1])  # noqa: E731
    for name, fn in (("stage_score_ms", score), ("stage_refine8_ms", refine), ("stage_pred_index_ms", build)):
        calls = warm(fn, args.seconds)
        res[name] = wall(fn, max(3, calls))
        print(json.dumps({name: res[name]}), flush=True)
    res["search_over_centroid"] = float(np.median(res["search"]["align_ms"]) / np.median(res["centroid"]["align_ms"]))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0); ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--only", choices=("icp", "search"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
    if args.only == "search":
        res = {"search": search_bench(dev, args)}
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    pred, gt = meshes(dev)
    index = sd.MeshIndex.build(gt[0], gt[1])
    frame = align.frame_of(index)
    res = {"pred_faces": int(pred[1].shape[0]), "gt_faces": int(gt[1].shape[0]), "iters": ITERS, "device": torch.cuda.get_device_name(0), "sizes": []}
    for samples in (100_000, 1_000_000):
        row = {"samples": samples, "blocks": align.blocks_of(samples)}
        for mode, scale in (("rigid", False), ("similarity", True)):
            fn = lambda: align.icp_align(pred, gt, samples=samples, iters=ITERS, scale=scale)  # noqa: E731
            calls = warm(fn, args.seconds)
            row[mode + "_align_ms"] = wall(fn, max(3, calls))
            a = fn()
            row[mode] = {"iterations": a.iterations, "converged": a.converged, "rank": a.rank, "scale": a.scale, "rms_before": a.rms_before,
                         "rms_after": a.rms_after}
        # one iteration from the start (the identity: the meshes are concentric) and from the converged similarity
        p = sd.sample_surface(pred[0], pred[1], samples, 0)[0]
        warm(lambda: sd.closest_point(p, index), args.seconds)
        row["closest_point_ms"] = wall(lambda: sd.closest_point(p, index), 20)           # (surfdist_bench's default query, for reference)
        final = align.icp_align(pred, gt, samples=samples, iters=ITERS, scale=True)
        start = np.zeros(align.STATE)
        start[:9] = np.eye(3).reshape(9)
        end = np.zeros(align.STATE)
        end[:9], end[9:12] = final.matrix[:3, :3].reshape(9), final.matrix[:3, 3]
        for label, s in (("start", start), ("converged", end)):
            state = torch.from_numpy(s).to(dev)
            order = torch.sort(mp.cell_keys(align.transform_points(state[:9].view(3, 3), state[9:12], p), index.lo, index.cell, index.n), stable=True)[1]
            it = Iteration(p[order].contiguous(), index, frame, state, True)
            it.fused()
            got, want = it.state.cpu().numpy()[:12], np.concatenate([x.reshape(-1) for x in it.composed()])
            row[label + "_fused_vs_composed"] = float(np.abs(got - want).max())
            nf, nc = warm(it.fused, args.seconds), warm(it.composed, args.seconds)
            fused, composed = [], []
            for _ in range(args.windows):                                                 # alternating windows
                fused.append(wall(it.fused, max(3, nf)))
                composed.append(wall(it.composed, max(3, nc)))
            row[label] = {"fused_ms": fused, "composed_ms": composed, "fused_calls": max(3, nf), "composed_calls": max(3, nc),
                          "ratio": float(np.median(composed) / np.median(fused))}
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    if args.only is None:
        res["search"] = search_bench(dev, args)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
