"""Times the ICP alignment (align.icp_align, csrc/icp.hip) on the meshes of tools/surfdist_bench.py: cube_sphere(170)
(346 800 faces) onto a jittered cube_sphere(119) x 1.05 (169 932 faces), at 10^5 and 10^6 samples.

Two things are timed.  (1) `icp_align` as a whole: the target's index build, the sampling, `iters` pairs of launches and the one copy.
(2) One iteration, the fused pair of launches (sr_icp_accumulate + sr_icp_solve) against the same iteration composed from what the
package offered before them: `closest_point`, a gather of `MeshIndex.face_normals`, the rows and their Gram matrix in torch double (one
matrix product: kinder to the composition than ten separate reductions), a copy to the host, a numpy solve and the upload of the new
state.  Both run from the same state, which is put back before every iteration (at the start, a gap of about five mean edges, and at
the converged similarity, where the surfaces touch), in alternating windows of wall time around a device synchronisation, after
seconds of warm-up (a ten-launch window measures the clock ramp, see README).

    python tools/icp_bench.py [--out FILE.json] [--seconds 2.0] [--windows 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0); ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
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
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
