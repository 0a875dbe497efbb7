"""What logging costs the training loop: the driver's own iteration (train.step + train.LoopLog) on build_synthetic_scene at 540 x 540,
coarse stage, three frames per step, with log = 'off', 'device' (one sr_log_row launch per iteration, rows read when they arrive) and
'item' (the reference's ~15 blocking reads per iteration).  The variants are interleaved, three repeats each, after seconds of warm-up
(a short window reads the clock ramp, see README); per variant ms per iteration and how far the host is ahead when it has issued the
last step (host-ahead: what a blocking read per iteration throws away).  The same network, optimiser and data serve every window.

    python tools/train_log_bench.py [--out profiles/train_loop.md] [--steps 60] [--warmup-seconds 8] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selfreconcode_amd import mlp_engine  # noqa: E402
from selfreconcode_amd import train as driver  # noqa: E402
from selfreconcode_amd.optim import FusedAdam  # noqa: E402
from selfreconcode_amd.synthetic import build_synthetic_scene  # noqa: E402

FRAMES, RAYS, MODES = 3, 2048, ('off', 'device', 'item')


def sensors():
    """Shader clock and socket power of this process's GPU, read from sysfs as bench.py reads them (None where the files do not exist)."""
    from bench import gpu_sensors
    return gpu_sensors(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--steps", type=int, default=60); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup-seconds", type=float, default=8.0); ap.add_argument("--bench-headline-ms", type=float, default=None,
                                                                                 help="bench.py's ms per step on the same box, for the record")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_log_bench: needs the GPU (a CPU run says nothing about it)")
    dev = torch.device("cuda:0")
    net, ds, conf = build_synthetic_scene(device=dev, frame_num=64, stage="coarse", consistent_masks=False)
    ds.attach_rendered_observations(net, {'sdfRatio': 1., 'deformerRatio': 0.5, 'renderRatio': 1.})
    mlp_engine.set_deferred_param_grads(True)
    opt = FusedAdam([{'params': ds.learnable_weights()}, {'params': [p for p in net.parameters() if p.requires_grad]}], lr=conf.get_float('train.learning_rate'))
    net._side_stream(dev)
    logs = {m: driver.LoopLog(m, dev, out=lambda *a, **k: None) for m in MODES}
    state = {"it": 0}

    def iteration(mode):
        it = state["it"]
        base = (it * FRAMES) % (ds.frame_num - FRAMES + 1)
        f = torch.arange(base, base + FRAMES, device=dev)
        ratio = {'sdfRatio': 1., 'deformerRatio': driver.deformer_ratio(float(it)), 'renderRatio': 1.}
        loss = driver.step(net, opt, ds.batch(f), RAYS, ratio, f)
        logs[mode].record(0, it, loss, net.info, ratio, opt.param_groups[0]['lr'])
        state["it"] = it + 1

    def window(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            iteration(mode)
            if i == n // 2:
                loaded = sensors()                                   # (GPU loaded: two small file reads)
        t_issued = time.perf_counter()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        logs[mode].flush()
        return {"sensors_mid_window": loaded, "ms_per_iteration": (t1 - t0) / n * 1e3, "host_issue_ms_per_iteration": (t_issued - t0) / n * 1e3, "host_ahead_ms_at_the_end": (t1 - t_issued) * 1e3}

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.warmup_seconds:           # every variant takes part in the warm-up
        for m in MODES:
            for _ in range(5):
                iteration(m)
        torch.cuda.synchronize()
    for m in MODES:
        logs[m].flush()
    before = sensors()
    runs = {m: [] for m in MODES}
    for _ in range(args.repeats):
        for m in MODES:                                              # interleaved: a drift of the box hits every variant alike
            runs[m].append(window(m, args.steps))
    after = sensors()
    res = {"device": torch.cuda.get_device_name(0), "steps_per_window": args.steps, "repeats": args.repeats, "warmup_seconds": args.warmup_seconds,
           "workload": f"{FRAMES} frames x {RAYS} rays, 540 x 540, coarse stage, lr {conf.get_float('train.learning_rate')}, iterations {state['it']} in all",
           "sensors_before": before, "sensors_after": after, "runs": runs, "device_log_stalls": logs['device'].stalls,
           "rows_logged": {m: len(logs[m].rows) for m in MODES}, "bench_headline_ms_same_box": args.bench_headline_ms}
    summary = {}
    for m in MODES:
        ms = [r["ms_per_iteration"] for r in runs[m]]
        summary[m] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
                      "host_ahead_ms": [round(r["host_ahead_ms_at_the_end"], 2) for r in runs[m]],
                      "host_issue_ms": [round(r["host_issue_ms_per_iteration"], 2) for r in runs[m]]}
    res["summary"] = summary
    off = summary['off']
    res["device_within_the_spread_of_off"] = bool(off["min_ms"] <= summary['device']["median_ms"] <= off["max_ms"])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# The training loop with its log off, on the device, and read value by value\n\n")
            fh.write(f"`tools/train_log_bench.py`: {res['workload']}; {args.repeats} interleaved windows of {args.steps} iterations per variant after "
                     f"{args.warmup_seconds:.0f} s of warm-up, on {res['device']}.  Clock / power before: {before}; after: {after}.\n\n")
            fh.write("| log | ms per iteration (median) | min – max of the repeats | host issue ms per iteration | host-ahead at the end of a window, ms |\n|---|---|---|---|---|\n")
            for m in MODES:
                s_ = summary[m]
                fh.write(f"| `{m}` | {s_['median_ms']:.2f} | {s_['min_ms']:.2f} – {s_['max_ms']:.2f} | {s_['host_issue_ms']} | {s_['host_ahead_ms']} |\n")
            fh.write(f"\n`device` inside the spread of the `off` repeats: **{res['device_within_the_spread_of_off']}**.  Stalls of the device log: "
                     f"{res['device_log_stalls']}.\n")
            if args.bench_headline_ms is not None:
                fh.write(f"\n`bench.py --gpus 1` on the same box in the same session: {args.bench_headline_ms:.2f} ms per step "
                         f"(`off` here: {off['median_ms']:.2f}).\n")
            fh.write("\n```json\n" + json.dumps(res) + "\n```\n")


if __name__ == "__main__":
    main()
