"""Times the winding-number inside / outside test at the shipped size on the GPU, on the meshes of tools/surfdist_bench.py: 10^6 samples
of cube_sphere(170) against a jittered cube_sphere(119) x 1.05 -- the index build, the tree query at beta 2, 3 and 4 (and in the
caller's order at 3), the brute-force kernel on 16 384 and 65 536 of the points scaled to 10^6, the tree's error against the brute
kernel on those 16 384, surface_metrics with and without `signed`, and a sweep of the leaf constant (leaf = c sqrt(area / faces)).
HIP events around many launches after seconds of warm-up (a 10-launch window measures the clock ramp, see README).

    python tools/winding_bench.py [--out profiles/winding_number.md] [--seconds 2.0]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from surfdist_bench import SAMPLES, SUBSAMPLE, meshes, timed  # noqa: E402
from selfreconcode_amd import surfdist_ops as sd  # noqa: E402
from selfreconcode_amd import winding_ops as wn  # noqa: E402
from selfreconcode_amd.evaluate import surface_metrics  # noqa: E402

BETAS = (2.0, 3.0, 4.0)
FACTORS = (1.0, 1.5, 2.0, 3.0, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("winding_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
    pred, gt = meshes(dev)
    pts = sd.sample_surface(pred[0], pred[1], SAMPLES, 0)[0]
    F = int(gt[1].shape[0])
    res = {"samples": SAMPLES, "gt_faces": F, "default_factor": wn.LEAF_FACTOR, "default_beta": wn.BETA, "betas": [], "sweep": []}
    index = wn.WindingIndex.build(gt[0], gt[1])
    res["levels"], res["nodes"], res["cell"] = index.levels, int(index.nodes.shape[0]), index.cell
    res["leaves_with_area"] = int((index.nodes[wn.level_offset(index.levels):, 6] > 0).sum())
    res["build_ms"], _ = timed(lambda: wn.WindingIndex.build(gt[0], gt[1]), args.seconds)
    sub = pts[torch.arange(SUBSAMPLE, device=dev) * (SAMPLES // SUBSAMPLE)].contiguous()
    sub4 = pts[torch.arange(4 * SUBSAMPLE, device=dev) * (SAMPLES // (4 * SUBSAMPLE))].contiguous()
    res["brute_subsample_ms"], res["brute_runs"] = timed(lambda: wn.winding_number(sub, index, method="brute"), args.seconds, 2)
    res["brute_scaled_ms"] = res["brute_subsample_ms"] * SAMPLES / SUBSAMPLE
    res["brute_4x_subsample_ms"], _ = timed(lambda: wn.winding_number(sub4, index, method="brute"), args.seconds, 2)
    res["brute_4x_scaled_ms"] = res["brute_4x_subsample_ms"] * SAMPLES / (4 * SUBSAMPLE)
    res["brute_gangles_per_s"] = 4 * SUBSAMPLE * F / (res["brute_4x_subsample_ms"] * 1e-3) / 1e9
    exact = wn.winding_number(sub, index, method="brute")
    for beta in BETAS:
        row = {"beta": beta}
        row["query_ms"], row["runs"] = timed(lambda: wn.winding_number(pts, index, beta=beta), args.seconds)
        w = wn.winding_number(sub, index, beta=beta)
        row["max_error_vs_brute"] = float((w - exact).abs().max())
        row["decisions_differ"] = int(((w >= 0.5) != (exact >= 0.5)).sum())
        row["brute_over_tree"] = min(res["brute_scaled_ms"], res["brute_4x_scaled_ms"]) / row["query_ms"]
        res["betas"].append(row)
        print(json.dumps(row), flush=True)
    res["query_unsorted_ms"], _ = timed(lambda: wn.winding_number(pts, index, presort=False), args.seconds)
    res["one_point_query_ms"], _ = timed(lambda: wn.winding_number(pts[:1], index), 0.2)              # (the floor: launches and host work)
    res["min_abs_w_minus_half_on_subsample"] = float((exact - 0.5).abs().min())
    for c in FACTORS:
        idx = wn.WindingIndex.build(gt[0], gt[1], leaf_factor=c)
        row = {"factor": c, "levels": idx.levels, "cell": idx.cell}
        row["build_ms"], _ = timed(lambda: wn.WindingIndex.build(gt[0], gt[1], leaf_factor=c), args.seconds)
        row["query_ms"], _ = timed(lambda: wn.winding_number(pts, idx), args.seconds)
        row["max_error_vs_brute"] = float((wn.winding_number(sub, idx) - exact).abs().max())
        res["sweep"].append(row)
        print(json.dumps(row), flush=True)
    for levels in range(max(index.levels - 3, 0), wn.MAX_LEVELS + 1):                                  # what the factor chooses between
        idx = wn.WindingIndex.build(gt[0], gt[1], levels=levels)
        row = {"levels": levels, "cell": idx.cell}
        row["build_ms"], _ = timed(lambda: wn.WindingIndex.build(gt[0], gt[1], levels=levels), args.seconds / 2)
        row["query_ms"], _ = timed(lambda: wn.winding_number(pts, idx), args.seconds / 2)
        row["max_error_vs_brute"] = float((wn.winding_number(sub, idx) - exact).abs().max())
        res["sweep"].append(row)
        print(json.dumps(row), flush=True)
    res["metrics_ms"], _ = timed(lambda: surface_metrics(pred, gt, SAMPLES, 0, (0.01,)), args.seconds)
    res["metrics_signed_ms"], _ = timed(lambda: surface_metrics(pred, gt, SAMPLES, 0, (0.01,), signed=True), args.seconds)
    res["metrics_signed"] = surface_metrics(pred, gt, SAMPLES, 0, (0.01,), signed=True)["signed"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(f"| {SAMPLES} points against {F} faces, {res['levels']} levels | tree query | max error vs brute on {SUBSAMPLE} points | decisions that differ | brute / tree |\n|---|---|---|---|---|\n")
            for r in res["betas"]:
                fh.write(f"| beta = {r['beta']} | {r['query_ms']:.2f} ms | {r['max_error_vs_brute']:.3g} | {r['decisions_differ']} | {r['brute_over_tree']:.0f} x |\n")
            fh.write("\n| leaf = c sqrt(area / faces), or levels forced | levels | build | tree query, beta 3 | max error vs brute |\n|---|---|---|---|---|\n")
            for r in res["sweep"]:
                fh.write(f"| {'c = %g' % r['factor'] if 'factor' in r else 'forced'} | {r['levels']} | {r['build_ms']:.2f} ms | {r['query_ms']:.2f} ms | {r['max_error_vs_brute']:.3g} |\n")
            fh.write("\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
