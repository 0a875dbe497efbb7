"""Times the skinning-field build at the shipped size -- (W, H, D) = (129, 225, 65), 6890 vertices, 30 neighbours, 30 smoothing steps --
on the GPU: the KNN blend, the smoothing and the whole compute_lbswField, next to the reference's formulation restated with torch ops
on the same device (chunked difference tensor + topk, sliced smoothing: what a user of the reference runs today).  HIP events around
many launches after seconds of warm-up (a 10-launch window measures the clock ramp, see README).

    python tools/lbsw_bench.py [--out profiles/lbsw_field.md] [--seconds 2.0]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selfreconcode_amd import ops  # noqa: E402
from selfreconcode_amd.model.Deformer import compute_lbswField  # noqa: E402
from selfreconcode_amd.synthetic import LBS_BMAX, LBS_BMIN, synthetic_body  # noqa: E402

RES, K, STEPS = (129, 225, 65), 30, 30


def torch_knn_blend(bmin, bmax, res, verts, vws, k):
    W, H, D = res
    dev = verts.device
    z, y, x = torch.meshgrid(torch.arange(D, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    r = torch.tensor(res, device=dev).float()
    c = (torch.stack([x, y, z]).view(3, -1).t().float() / r + 0.5 / r) * (torch.tensor(bmax, device=dev) - torch.tensor(bmin, device=dev)) \
        + torch.tensor(bmin, device=dev)
    out = []
    for part in torch.split(c, 50000):
        d, i = (part[:, None, :] - verts[None]).norm(dim=-1).topk(k, dim=-1, largest=False)
        w = 1. / d.clamp(0.0001, 1.)
        w = w / w.sum(-1, keepdim=True)
        out.append((vws[i.view(-1)] * w.view(-1, 1)).view(w.shape[0], k, -1).sum(1))
    return torch.cat(out).t().reshape(1, -1, D, H, W)


def torch_smooth(f, times):
    for _ in range(times):
        mean = (f[:, :, 2:, 1:-1, 1:-1] + f[:, :, :-2, 1:-1, 1:-1] + f[:, :, 1:-1, 2:, 1:-1] + f[:, :, 1:-1, :-2, 1:-1] + f[:, :, 1:-1, 1:-1, 2:]
                + f[:, :, 1:-1, 1:-1, :-2]) / 6.0
        f[:, :, 1:-1, 1:-1, 1:-1] = (f[:, :, 1:-1, 1:-1, 1:-1] - mean) * 0.7 + mean
        f = f / f.sum(1, keepdim=True)
    return f


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lbsw_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
    v, w = (t.to(dev) for t in synthetic_body())
    pre = ops.lbsw_knn_blend(v, w, LBS_BMIN, LBS_BMAX, RES, K)
    res = {}
    res["knn_ms"], res["knn_runs"] = timed(lambda: ops.lbsw_knn_blend(v, w, LBS_BMIN, LBS_BMAX, RES, K), args.seconds)
    res["smooth30_ms"], res["smooth_runs"] = timed(lambda: ops.lbsw_smooth(pre, STEPS), args.seconds)
    res["build_ms"], _ = timed(lambda: compute_lbswField(LBS_BMIN, LBS_BMAX, RES, v, w, mean_neighbor=K, smooth_times=STEPS), args.seconds)
    res["torch_knn_ms"], res["torch_knn_runs"] = timed(lambda: torch_knn_blend(LBS_BMIN, LBS_BMAX, RES, v, w, K), args.seconds, 2)
    res["torch_smooth30_ms"], _ = timed(lambda: torch_smooth(pre[None].clone(), STEPS), args.seconds)
    nbytes = pre.numel() * 4
    res["smooth_gbs"] = 2 * nbytes * STEPS / (res["smooth30_ms"] * 1e-3) / 1e9          # one read and one write of the volume per step
    res["smooth_share_of_8tbs"] = res["smooth_gbs"] / 8000.
    res["knn_gdist_per_s"] = (pre.numel() // 24) * v.shape[0] / (res["knn_ms"] * 1e-3) / 1e9
    ours = compute_lbswField(LBS_BMIN, LBS_BMAX, RES, v, w, mean_neighbor=K, smooth_times=STEPS)
    theirs = torch_smooth(torch_knn_blend(LBS_BMIN, LBS_BMAX, RES, v, w, K), STEPS)
    res["max_abs_diff_vs_torch"] = float((ours - theirs).abs().max())
    res["share_of_voxels_off_by_1e-5"] = float(((ours - theirs).abs().amax(1) > 1e-5).float().mean())
    res["device"] = torch.cuda.get_device_name(0)
    try:
        res["sclk_mhz_after"] = torch.cuda.clock_rate()
    except Exception as e:                                                 # (needs the amdsmi bindings)
        res["sclk_mhz_after"] = f"not read ({type(e).__name__})"
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(f"| stage ({RES[0]}x{RES[1]}x{RES[2]}, 6890 vertices, k = {K}, {STEPS} steps) | HIP kernels | torch formulation, same GPU |\n|---|---|---|\n")
            fh.write(f"| KNN blend | {res['knn_ms']:.2f} ms | {res['torch_knn_ms']:.1f} ms |\n")
            fh.write(f"| {STEPS} smoothing steps | {res['smooth30_ms']:.2f} ms ({res['smooth_gbs']:.0f} GB/s, {100 * res['smooth_share_of_8tbs']:.0f} % of 8 TB/s) | "
                     f"{res['torch_smooth30_ms']:.1f} ms |\n")
            fh.write(f"| compute_lbswField | {res['build_ms']:.2f} ms | {res['torch_knn_ms'] + res['torch_smooth30_ms']:.1f} ms |\n\n")
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
