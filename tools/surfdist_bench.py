"""Times the surface-distance evaluation at the shipped size on the GPU: 10^6 samples of cube_sphere(170) (173 402 vertices, the fine
stage's template size) against a jittered cube_sphere(119) x 1.05 (84 968 vertices) and back -- the index build, the grid query with and
without pre-sorting the points by cell key, a sweep of the cell constant (cell = c sqrt(area / faces)) at a gap of five mean edges and
at one of half an edge, and the brute-force kernel on a
16 384-point subsample scaled to 10^6 points.  HIP events around many launches after seconds of warm-up (a 10-launch window measures
the clock ramp, see README).

    python tools/surfdist_bench.py [--out profiles/surface_distance.md] [--seconds 2.0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selfreconcode_amd import surfdist_ops as sd  # noqa: E402
from selfreconcode_amd.evaluate import surface_metrics  # noqa: E402
from selfreconcode_amd.synthetic import cube_sphere  # noqa: E402

SAMPLES, SUBSAMPLE = 1_000_000, 16384
FACTORS = (1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
NEAR = 1.045               # the samples scaled to this radius lie within the jitter of the other mesh: a gap of about half a mean edge


def timed(fn, seconds, min_runs=3):
    """ms per call: warm up for `seconds` of wall time, then time as many calls between two events."""
    t0, n = time.time(), 0
    while time.time() - t0 < seconds or n < 1:
        fn(); torch.cuda.synchronize(); n += 1
    runs = max(min_runs, n)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(runs):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / runs, runs


def meshes(dev):
    pv, pf = cube_sphere(170)
    gv, gf = cube_sphere(119)
    gv = (gv.numpy() + np.random.default_rng(5).normal(0., 0.004, gv.shape)).astype(np.float32) * np.float32(1.05)
    return (pv.to(dev), pf.to(dev)), (torch.from_numpy(gv).to(dev), gf.to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surfdist_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
    pred, gt = meshes(dev)
    pts = sd.sample_surface(pred[0], pred[1], SAMPLES, 0)[0]
    back = sd.sample_surface(gt[0], gt[1], SAMPLES, 1)[0]
    res = {"samples": SAMPLES, "pred_faces": int(pred[1].shape[0]), "gt_faces": int(gt[1].shape[0]), "default_factor": sd.CELL_FACTOR, "sweep": []}
    res["sample_ms"], _ = timed(lambda: sd.sample_surface(pred[0], pred[1], SAMPLES, 0), args.seconds)
    base = (sd.MeshIndex.build(gt[0], gt[1]).area / gt[1].shape[0]) ** 0.5
    sub = pts[torch.arange(SUBSAMPLE, device=dev) * (SAMPLES // SUBSAMPLE)].contiguous()
    for c in FACTORS:
        index = sd.MeshIndex.build(gt[0], gt[1], c * base)
        row = {"factor": c, "cell": index.cell, "grid": list(index.n), "pairs_per_face": index.pairs / gt[1].shape[0]}
        row["build_ms"], _ = timed(lambda: sd.MeshIndex.build(gt[0], gt[1], c * base), args.seconds)
        row["query_sorted_ms"], row["runs"] = timed(lambda: sd.closest_point(pts, index), args.seconds)
        row["query_unsorted_ms"], _ = timed(lambda: sd.closest_point(pts, index, presort=False), args.seconds)
        row["mqueries_per_s"] = SAMPLES / (min(row["query_sorted_ms"], row["query_unsorted_ms"]) * 1e-3) / 1e6
        near = (pts * NEAR).contiguous()
        row["near_sorted_ms"], _ = timed(lambda: sd.closest_point(near, index), args.seconds)
        row["near_unsorted_ms"], _ = timed(lambda: sd.closest_point(near, index, presort=False), args.seconds)
        res["sweep"].append(row)
        print(json.dumps(row), flush=True)
    index = sd.MeshIndex.build(gt[0], gt[1])
    res["default"] = {"cell": index.cell, "grid": list(index.n), "pairs_per_face": index.pairs / gt[1].shape[0]}
    res["default"]["build_ms"], _ = timed(lambda: sd.MeshIndex.build(gt[0], gt[1]), args.seconds)
    res["default"]["query_ms"], _ = timed(lambda: sd.closest_point(pts, index), args.seconds)
    rindex = sd.MeshIndex.build(pred[0], pred[1])
    res["default"]["reverse_build_ms"], _ = timed(lambda: sd.MeshIndex.build(pred[0], pred[1]), args.seconds)
    res["default"]["reverse_query_ms"], _ = timed(lambda: sd.closest_point(back, rindex), args.seconds)
    res["brute_subsample_ms"], res["brute_runs"] = timed(lambda: sd.closest_point(sub, index, method="brute"), args.seconds, 2)
    res["brute_scaled_ms"] = res["brute_subsample_ms"] * SAMPLES / SUBSAMPLE
    res["brute_gpairs_per_s"] = SUBSAMPLE * gt[1].shape[0] / (res["brute_subsample_ms"] * 1e-3) / 1e9
    res["grid_over_brute"] = res["brute_scaled_ms"] / res["default"]["query_ms"]
    sub4 = pts[torch.arange(4 * SUBSAMPLE, device=dev) * (SAMPLES // (4 * SUBSAMPLE))].contiguous()      # 256 blocks: one per CU (16 384 points fill 64)
    res["brute_4x_subsample_ms"], _ = timed(lambda: sd.closest_point(sub4, index, method="brute"), args.seconds, 2)
    res["brute_4x_scaled_ms"] = res["brute_4x_subsample_ms"] * SAMPLES / (4 * SUBSAMPLE)
    g, b = sd.closest_point(sub, index), sd.closest_point(sub, index, method="brute")
    res["grid_equals_brute_on_subsample"] = all(torch.equal(x, y) for x, y in zip(g, b))
    res["metrics_ms"], _ = timed(lambda: surface_metrics(pred, gt, SAMPLES, 0, (0.01,)), args.seconds)
    res["metrics"] = surface_metrics(pred, gt, SAMPLES, 0, (0.01,))
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(f"| cell = c sqrt(area / faces), {SAMPLES} points against {res['gt_faces']} faces | grid | pairs / face | build | query, points sorted "
                     "by cell key | query, caller's order | Mqueries/s | same, samples at radius " + str(NEAR) + " (sorted / caller's order) |\n|---|---|---|---|---|---|---|---|\n")
            for r in res["sweep"]:
                fh.write(f"| c = {r['factor']} (cell {r['cell']:.4g}) | {r['grid'][0]} x {r['grid'][1]} x {r['grid'][2]} | {r['pairs_per_face']:.2f} | "
                         f"{r['build_ms']:.2f} ms | {r['query_sorted_ms']:.2f} ms | {r['query_unsorted_ms']:.2f} ms | {r['mqueries_per_s']:.0f} | {r['near_sorted_ms']:.2f} / {r['near_unsorted_ms']:.2f} ms |\n")
            fh.write("\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
