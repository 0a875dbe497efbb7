"""Times the SMPL body model (smpl_pytorch.SMPL on csrc/smpl.hip) on the synthetic model at the real body's size: the whole forward
and the skin kernel alone, for one frame and for a sequence, after seconds of warm-up (profiles/lbsw_field.md: the first launches
load code objects and the clocks ramp).  Prints one JSON line per batch size; needs a GPU.

    python tools/smpl_bench.py [--nv 6890] [--batches 1 300] [--warmup-seconds 3] [--seconds 2]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from selfreconcode_amd import ops  # noqa: E402
from selfreconcode_amd.smpl_pytorch import SMPL  # noqa: E402
from selfreconcode_amd.synthetic import det_tensor, synthetic_smpl_model  # noqa: E402


def timed(fn, warmup_seconds, seconds):
    """Mean device time per call in microseconds (events around a batch of calls), after `warmup_seconds` of the same calls."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warmup_seconds:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    calls = max(10, min(20000, int(seconds / max(time.perf_counter() - t0, 1e-6))))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record(); torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nv", type=int, default=6890)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 300])
    ap.add_argument("--warmup-seconds", type=float, default=3.0)
    ap.add_argument("--seconds", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smpl_bench: no GPU (a CPU run measures nothing about it)")
    dev = "cuda:0"
    smpl = SMPL(synthetic_smpl_model(args.nv, 0)).to(dev)
    posedirs_bytes = smpl.posedirs.numel() * 4
    for B in args.batches:
        beta = det_tensor((B, 10), 1, 1.5).to(dev)
        theta = det_tensor((B, 24, 3), 2, 0.6).to(dev)
        fwd_us, calls = timed(lambda: smpl(beta, theta, get_skin=True), args.warmup_seconds, args.seconds)
        J, v_shaped = smpl.skeleton(beta, True)
        _, feature, _, A = ops.smpl_pose(J, smpl.parents, theta=theta)
        skin_us, _ = timed(lambda: ops.smpl_skin(v_shaped, smpl.weight[0], A, smpl.posedirs, feature), 1.0, args.seconds)
        tiles = -(-B // ops.SMPL_BATCH_TILE)
        # what the skin kernel has to move: posedirs once per batch tile, v_shaped in, verts out, the weights once per tile
        streamed = tiles * (posedirs_bytes + smpl.weight.numel() * 4) + 2 * B * args.nv * 12
        print(json.dumps({"nv": args.nv, "B": B, "forward_us": round(fwd_us, 2), "forward_us_per_frame": round(fwd_us / B, 3),
                          "skin_kernel_us": round(skin_us, 2), "batch_tiles": tiles, "posedirs_MB": round(posedirs_bytes / 1e6, 2),
                          "skin_bytes_streamed_MB": round(streamed / 1e6, 2), "posedirs_share_of_bytes": round(tiles * posedirs_bytes / streamed, 4),
                          "skin_GB_per_s": round(streamed / skin_us / 1e3, 1), "skin_GFMA_per_s": round(B * args.nv * (3 * 207 + 288 + 9) / skin_us / 1e3, 1),
                          "timed_calls": calls}), flush=True)


if __name__ == "__main__":
    main()
