"""Times one batch of frames out of the GPU-resident store (ops.frames_fetch, csrc/frames.hip) at the sizes the training stages use:
3, 2 and 1 frames of 540 x 540 and 1 frame of 1080 x 1080, with and without normals, by-value ids and ids in device memory.  HIP events
around many back-to-back launches after seconds of warm-up (a 10-launch window measures the clock ramp, see README), the output buffers
reused so that the allocator is not timed.  Bytes moved per batch: N H W (7 read + 28 written) with normals, (4 + 16) without.

    python tools/dataset_bench.py [--out profiles/scene_dataset.md] [--seconds 2.0]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selfreconcode_amd import ops  # noqa: E402

FRAMES = 64
CASES = [(3, 540), (2, 540), (1, 540), (1, 1080)]
HBM_MEASURED_GBS, HBM_SPEC_GBS = 6290., 8000.        # float4 copy on this part / the data sheet


def timed(fn, seconds, min_runs=50):
    """us per call: warm up for `seconds` of wall time, then time as many calls between two events."""
    t0, n = time.time(), 0
    while time.time() - t0 < seconds or n < 1:
        fn(); n += 1
        if n % 256 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    runs = max(min_runs, n)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(runs):
        fn()
    b.record(); torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / runs, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dataset_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
    rows = []
    for N, S in CASES:
        g = torch.Generator(device=dev); g.manual_seed(S)
        img = torch.randint(0, 256, (FRAMES, ops.frames_pitch(3 * S * S)), dtype=torch.uint8, device=dev, generator=g)
        normal = torch.randint(0, 256, (FRAMES, ops.frames_pitch(3 * S * S)), dtype=torch.uint8, device=dev, generator=g)
        mask = torch.randint(0, 2, (FRAMES, ops.frames_pitch(S * S)), dtype=torch.uint8, device=dev, generator=g)
        ids = [(17 * i + 5) % FRAMES for i in range(N)]
        ids_dev = torch.tensor(ids, device=dev)
        for with_normals in (True, False):
            out = [torch.empty((N, S, S, 3), device=dev), torch.empty((N, S, S, 3), device=dev) if with_normals else None, torch.empty((N, S, S), device=dev)]
            nrm = normal if with_normals else None
            us_value, runs = timed(lambda: ops.frames_fetch(img, nrm, mask, S, S, ids, out=out), args.seconds)
            us_device, _ = timed(lambda: ops.frames_fetch(img, nrm, mask, S, S, ids_dev, out=out), args.seconds)
            nbytes = N * S * S * (35 if with_normals else 20)
            rows.append({"frames": N, "size": S, "normals": with_normals, "us_by_value": us_value, "us_device_ids": us_device, "runs": runs,
                         "bytes": nbytes, "gbs_by_value": nbytes / us_value / 1e3, "float_mb_uploaded_by_the_reference": N * S * S * (28 if with_normals else 16) / 1e6})
    res = {"rows": rows, "device": torch.cuda.get_device_name(0), "warmup_seconds": args.seconds}
    try:
        res["sclk_mhz_after"] = torch.cuda.clock_rate()
    except Exception as e:                                                 # (needs the amdsmi bindings)
        res["sclk_mhz_after"] = f"not read ({type(e).__name__})"
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("| batch | normals | by-value ids | ids in device memory | bytes moved | GB/s (by value) | of 6.29 TB/s measured copy | of 8 TB/s |\n|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write(f"| {r['frames']} x {r['size']}^2 | {'yes' if r['normals'] else 'no'} | {r['us_by_value']:.1f} us | {r['us_device_ids']:.1f} us | "
                         f"{r['bytes'] / 1e6:.1f} MB | {r['gbs_by_value']:.0f} | {100 * r['gbs_by_value'] / HBM_MEASURED_GBS:.0f} % | "
                         f"{100 * r['gbs_by_value'] / HBM_SPEC_GBS:.0f} % |\n")
            fh.write("\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
