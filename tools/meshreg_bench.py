"""Times the mesh regularisers of the template step (mesh_losses.py, csrc/mesh_reg.hip) on the GPU at the template sizes of the coarse and
the fine stage (marching-cubes templates of the synthetic scene, V about 87k and 196k):

  * the fused op, forward + backward, all three terms with the reference's weights (10, 10, 0.001);
  * the same terms restated with torch ops on the same GPU (index_add / gathers / autograd) -- the only other implementation there is:
    the parent commit cannot run these terms at all;
  * MeshTopology.from_faces (once per remesh);
  * the coarse-stage training step with the terms off and on, A/B alternated in blocks in one process.

Seconds of warm-up before every timing (a window of ten launches measures the clock ramp, see profiles/lbsw_field.md).

    python tools/meshreg_bench.py [--out profiles/mesh_regularisers.md] [--seconds 2.0] [--no-step]
    python tools/meshreg_bench.py --op-only 200      # just 200 forward + backward calls of the op at the coarse size: run this under
                                                     # `rocprofv3 --kernel-trace --stats -- python ...` and divide the meshreg_* calls by 200
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selfreconcode_amd.mesh_losses import MeshTopology, mesh_regularisers  # noqa: E402
from selfreconcode_amd.synthetic import build_synthetic_scene  # noqa: E402

WEIGHTS = (10., 10., 0.001)
RATIO = {'sdfRatio': 1., 'deformerRatio': 0.5, 'renderRatio': 1.}


def template(stage, dev):
    net, _, _ = build_synthetic_scene(device=dev, frame_num=64, stage=stage, consistent_masks=False)
    with torch.no_grad():
        v, f = net.discretizeSDF(RATIO, None, 0.0)
    return v.detach().float().contiguous(), f[(f >= 0).all(1)].long().contiguous()


def torch_terms(v, topo):
    """The three terms with torch ops (differences first, as the kernels)."""
    e, deg, p = topo.edges.long(), topo.deg.long(), topo.pairs.long()
    diff = v[e[:, 1]] - v[e[:, 0]]
    s = torch.zeros_like(v).index_add(0, e[:, 0], diff).index_add(0, e[:, 1], -diff)
    d = torch.where((deg > 0)[:, None], s / deg.clamp(min=1)[:, None], -v)
    lap = d.norm(dim=1).mean()
    edge = (diff.norm(dim=1) ** 2).mean()
    v0, v1, a, b = (v[p[:, k]] for k in range(4))
    n0, n1 = torch.cross(v1 - v0, a - v0, dim=-1), -torch.cross(v1 - v0, b - v0, dim=-1)
    nc = (1. - (n0 * n1).sum(-1) / (n0.norm(dim=1) * n1.norm(dim=1)).clamp(min=1e-8)).mean()
    return lap, edge, nc


def fused_iter(v, topo):
    v.grad = None
    lap, edge, nc = mesh_regularisers(v, topo, *WEIGHTS)
    (WEIGHTS[0] * lap + WEIGHTS[1] * edge + WEIGHTS[2] * nc).backward()


def torch_iter(v, topo):
    v.grad = None
    lap, edge, nc = torch_terms(v, topo)
    (WEIGHTS[0] * lap + WEIGHTS[1] * edge + WEIGHTS[2] * nc).backward()


def timed(fn, seconds, min_runs=5):
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


def step_ab(dev, seconds, blocks=6, per_block=10):
    """ms per coarse-stage iteration (3 frames, 2048 rays, 540 x 540) with the terms off / on, blocks alternated; the remesh stays outside."""
    from selfreconcode_amd import mlp_engine
    from selfreconcode_amd.optim import FusedAdam
    net, ds, conf = build_synthetic_scene(device=dev, frame_num=64, stage="coarse", consistent_masks=False)
    mlp_engine.set_deferred_param_grads(True)
    opt = FusedAdam([{'params': ds.learnable_weights()}, {'params': [p for p in net.parameters() if p.requires_grad]}], lr=conf.get_float('train.learning_rate'))
    state = {"it": 0}

    def step():
        f = torch.arange(3, device=dev) + (state["it"] * 3) % 60
        opt.zero_grad(set_to_none=True)
        loss = net(ds.batch(f), 2048, RATIO, f)
        loss.backward()
        net.propagateTmpPsGrad(f, RATIO)
        opt.step()
        state["it"] += 1
        if net.forward_time % net.remesh_intersect == 0:       # keep the remesh (and the topology build) out of the timed blocks
            net.forward_time = 1

    def set_terms(on):
        for k, w in zip(('laplacian_weight', 'edge_weight', 'norm_weight'), WEIGHTS):
            net.conf['pc_weight'][k] = w if on else -w

    for on in (False, True):                                   # warm both variants (the first `on` step builds the topology)
        set_terms(on)
        t0 = time.time()
        while time.time() - t0 < seconds:
            step(); torch.cuda.synchronize()
    ms = {False: [], True: []}
    for b in range(2 * blocks):
        on = b % 2 == 1
        set_terms(on)
        step(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(per_block):
            step()
        torch.cuda.synchronize()
        ms[on].append((time.perf_counter() - t0) * 1e3 / per_block)
    med = lambda x: sorted(x)[len(x) // 2]                       # noqa: E731
    return dict(step_off_ms=med(ms[False]), step_on_ms=med(ms[True]), step_off_blocks=ms[False], step_on_blocks=ms[True], template_V=int(net.TmpVs.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--no-step", action="store_true"); ap.add_argument("--op-only", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshreg_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
    if args.op_only:
        v, f = template("coarse", dev)
        topo = MeshTopology.from_faces(f, v.shape[0])
        v.requires_grad_(True)
        for _ in range(args.op_only):
            fused_iter(v, topo)
        torch.cuda.synchronize()
        print(json.dumps(dict(op_only_iterations=args.op_only, V=v.shape[0], E=topo.num_edges, P=topo.num_pairs)))
        return
    res = {"device": torch.cuda.get_device_name(0), "weights": WEIGHTS, "sizes": []}
    for stage in ("coarse", "fine"):
        v, f = template(stage, dev)
        topo = MeshTopology.from_faces(f, v.shape[0])
        r = dict(stage=stage, V=int(v.shape[0]), F=int(f.shape[0]), E=int(topo.num_edges), P=int(topo.num_pairs))
        r["topology_ms"], _ = timed(lambda: MeshTopology.from_faces(f, v.shape[0]), args.seconds)
        v.requires_grad_(True)
        r["fused_ms"], r["fused_runs"] = timed(lambda: fused_iter(v, topo), args.seconds)
        g = v.grad.clone()
        r["torch_ms"], r["torch_runs"] = timed(lambda: torch_iter(v, topo), args.seconds)
        r["max_grad_diff_vs_torch"] = float((v.grad - g).abs().max() / g.abs().max())
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)
    if not args.no_step:
        res.update(step_ab(dev, args.seconds))
    try:
        res["sclk_mhz_after"] = torch.cuda.clock_rate()
    except Exception as e:                                                 # (needs the amdsmi bindings)
        res["sclk_mhz_after"] = f"not read ({type(e).__name__})"
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("| template | V | E | P | fused op, fwd + bwd | torch restatement, same GPU | MeshTopology.from_faces |\n|---|---|---|---|---|---|---|\n")
            for r in res["sizes"]:
                fh.write(f"| {r['stage']} | {r['V']} | {r['E']} | {r['P']} | {r['fused_ms']:.3f} ms | {r['torch_ms']:.3f} ms | {r['topology_ms']:.2f} ms |\n")
            if "step_on_ms" in res:
                fh.write(f"\ncoarse-stage step (3 frames, 2048 rays, 540 x 540, template of {res['template_V']} vertices), median of alternated blocks: "
                         f"terms off {res['step_off_ms']:.2f} ms, terms on {res['step_on_ms']:.2f} ms\n")
            fh.write("\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
