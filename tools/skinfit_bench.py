"""Times the skin fit at the shipped size on the GPU: the synthetic avatar (selfreconcode_amd.synthetic) with a capture of 300 frames and
its template simplified to 20 000 faces.  The fused path (sr_skinfit_accumulate over the batches + sr_skinfit_solve) against the composed
one (the same from torch operators in float64), each on the deformer's outputs already in memory, so that the two time the fit and not
the MLP.  Checks on the way that both choose the same supports.  Then the whole export with --self-check semantics: the (a) / (b) / (c)
mean distances of export/selfcheck.txt.  HIP events around many calls after seconds of warm-up (a 10-launch window measures the clock
ramp, see README).

    python tools/skinfit_bench.py [--out profiles/gltf_export.json] [--seconds 2.0] [--frames 300] [--faces 20000]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from surfdist_bench import timed  # noqa: E402
from selfreconcode_amd import skinfit_ops as so  # noqa: E402

K, C, BATCH = 4, 8, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--frames", type=int, default=300); ap.add_argument("--faces", type=int, default=20000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skinfit_bench: needs the GPU (a CPU run says nothing about it)")
    from selfreconcode_amd.animate import training_tables
    from selfreconcode_amd.export_gltf import evaluate_deformer, export_avatar, field_weights
    from selfreconcode_amd.mesh_prep import simplify_to
    from selfreconcode_amd.posed import FULL_RATIO
    from selfreconcode_amd.synthetic import build_synthetic_scene
    dev = "cuda:0"
    net, ds, _ = build_synthetic_scene(device=dev, frame_num=args.frames, H=64, W=64, consistent_masks=False)
    mesh = simplify_to(*net.discretizeSDF(FULL_RATIO, None, 0.), args.faces)
    verts, faces = mesh.verts, mesh.faces
    V, T = verts.shape[0], args.frames
    res = {"V": int(V), "F": int(faces.shape[0]), "T": T, "K": K, "C": C, "batch": BATCH}
    poses, trans, codes = training_tables(net)
    batches, w_sum = [], torch.zeros((V, 24), dtype=torch.float64, device=dev)
    for k0 in range(0, T, BATCH):
        sl = slice(k0, k0 + BATCH)
        q, y, A = evaluate_deformer(net, verts, poses[sl], trans[sl], codes[sl])
        w_sum += field_weights(net.deformer.defs[1], q).view(q.shape[0], V, 24).double().sum(0)
        batches.append((q, y, A[:, :, :3, :].reshape(-1, 24, 12).contiguous(), trans[sl].contiguous()))
    cands, xbar = so.candidates(w_sum / T, C)

    def accumulate(method):
        H = so.new_normal_matrix(V, dev)
        for q, y, A, tr in batches:
            so.accumulate(H, q, y, A, tr, cands, method)
        return H

    def fit(method):
        return so.solve(accumulate(method), xbar, cands, K, method=method)
    fused, composed = fit("fused"), fit("composed")
    res["same_supports"] = float((fused['mask'] == composed['mask']).float().mean())
    res["objective_rel_diff"] = float(((fused['objective'] - composed['objective']).abs() / composed['objective'].abs().clamp_min(1e-300)).max())
    H = accumulate("fused")
    res["fused_accumulate_ms"], _ = timed(lambda: accumulate("fused"), args.seconds)
    res["fused_solve_ms"], _ = timed(lambda: so.solve(H, xbar, cands, K), args.seconds)
    res["fused_solve_k8_ms"], _ = timed(lambda: so.solve(H, xbar, cands, 8), args.seconds)
    res["fused_ms"], res["fused_runs"] = timed(lambda: fit("fused"), args.seconds)
    res["composed_accumulate_ms"], _ = timed(lambda: accumulate("composed"), args.seconds)
    res["composed_solve_ms"], _ = timed(lambda: so.solve(H, xbar, cands, K, method="composed"), args.seconds)
    res["composed_ms"], res["composed_runs"] = timed(lambda: fit("composed"), args.seconds)
    res["composed_over_fused"] = res["composed_ms"] / res["fused_ms"]
    with tempfile.TemporaryDirectory() as root:
        torch.cuda.synchronize()
        t0 = time.time()
        record = export_avatar(net, root, verts, faces, K=K, B=8, C=C, self_check=True, batch_size=BATCH)
        res["export_seconds"] = time.time() - t0
        res["glb_bytes"] = os.path.getsize(os.path.join(root, "export", "avatar.glb"))
    res["self_check"] = record["self_check"]
    res["kept_variance"] = record["kept_variance"]
    res["residual_fit"], res["residual_naive"] = record["residual_fit"], record["residual_naive"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
