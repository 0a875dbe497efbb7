"""Times the template preparation of the texture stage at the fine stage's template size -- cube_sphere(170): 173 402 vertices, 346 800
faces -> simplify_to(20000) -> unwrap_charts(1680) -- on the GPU, stage by stage, the simplification with both vertex placements (and
their report counts and simplify_quality against the source), and with the edge-collapse decimation simplify_collapse(20000) and the
unwrap of its result.  Wall time around synchronised calls after seconds of
warm-up (these functions read flags and boxes back, so they are host-paced: HIP events around them would say the same).

    python tools/template_prep_bench.py [--out profiles/template_prepare.md] [--seconds 2.0]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selfreconcode_amd import mesh_prep  # noqa: E402
from selfreconcode_amd.synthetic import cube_sphere  # noqa: E402

N, TARGET, R = 170, 20000, 1680


def timed(fn, seconds, min_runs=3):
    """ms per call: warm up for `seconds` of wall time, then time as many synchronised calls."""
    t0, n = time.time(), 0
    while time.time() - t0 < seconds or n < 1:
        fn(); torch.cuda.synchronize(); n += 1
    runs = max(min_runs, n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / runs, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("template_prep_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
    v, f = (t.to(dev) for t in cube_sphere(N))
    probes = []
    mesh = mesh_prep.simplify_to(v, f, TARGET, probes=probes)
    atlas = mesh_prep.unwrap_charts(mesh.verts, mesh.faces, R)
    res = {"vertices": v.shape[0], "faces": f.shape[0], "target_faces": TARGET, "resolution": R, "cell": mesh.cell, "probes": len(probes),
           "out_vertices": mesh.verts.shape[0], "out_faces": mesh.faces.shape[0], "charts": atlas.labels.shape[0], "scale": atlas.scale,
           "rounds": atlas.rounds, "overlap_texels": atlas.overlap_texels}
    res["simplify_mesh_ms"], res["simplify_mesh_runs"] = timed(lambda: mesh_prep.simplify_mesh(v, f, mesh.cell), args.seconds)
    res["simplify_to_ms"], res["simplify_to_runs"] = timed(lambda: mesh_prep.simplify_to(v, f, TARGET), args.seconds)
    # the quadric placement: the same clustering, two more launches and one more sort; its counts and both placements' distance to the source
    res["simplify_mesh_quadric_ms"], res["simplify_mesh_quadric_runs"] = timed(lambda: mesh_prep.simplify_mesh(v, f, mesh.cell, placement="quadric"), args.seconds)
    res["simplify_to_quadric_ms"], res["simplify_to_quadric_runs"] = timed(lambda: mesh_prep.simplify_to(v, f, TARGET, placement="quadric"), args.seconds)
    res["simplify_mesh_again_ms"], _ = timed(lambda: mesh_prep.simplify_mesh(v, f, mesh.cell), args.seconds)      # (the spread of the first line)
    for placement in mesh_prep.PLACEMENTS:
        report = {}
        m = mesh_prep.simplify_to(v, f, TARGET, placement=placement, report=report)
        res["report_" + placement] = report
        res["quality_" + placement] = mesh_prep.simplify_quality(m, v, f)
        res["sphere_error_" + placement] = float((m.verts.double().norm(dim=1) - 1.).abs().max())            # (the template is the unit sphere)
    # the edge-collapse decimation to the same budget: its rounds, its distance to the source, and what box projection makes of its result
    report = {}
    cm = mesh_prep.simplify_collapse(v, f, TARGET, report=report)
    res["report_collapse"] = report
    res["quality_collapse"] = mesh_prep.simplify_quality(cm, v, f)
    res["sphere_error_collapse"] = float((cm.verts.double().norm(dim=1) - 1.).abs().max())
    res["simplify_collapse_ms"], res["simplify_collapse_runs"] = timed(lambda: mesh_prep.simplify_collapse(v, f, TARGET), args.seconds)
    catlas = mesh_prep.unwrap_charts(cm.verts, cm.faces, R)
    res.update(collapse_charts=catlas.labels.shape[0], collapse_overlap_texels=catlas.overlap_texels, collapse_scale=catlas.scale, collapse_unwrap_rounds=catlas.rounds)
    res["collapse_unwrap_ms"], _ = timed(lambda: mesh_prep.unwrap_charts(cm.verts, cm.faces, R), args.seconds)
    res["simplify_to_again_ms"], _ = timed(lambda: mesh_prep.simplify_to(v, f, TARGET), args.seconds)           # (the clustering once more, after the collapse lines)
    res["unwrap_ms"], res["unwrap_runs"] = timed(lambda: mesh_prep.unwrap_charts(mesh.verts, mesh.faces, R), args.seconds)
    res["unwrap_full_size_ms"], _ = timed(lambda: mesh_prep.unwrap_charts(v, f, R), args.seconds)       # the unsimplified template: the kernels at size
    ext = atlas.extent.cpu().numpy()
    res["pack_host_ms"], _ = timed(lambda: mesh_prep.pack_charts(ext, R, 2), min(args.seconds, 0.5))
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(f"| stage (cube_sphere({N}): {res['vertices']} vertices, {res['faces']} faces) | time |\n|---|---|\n")
            fh.write(f"| simplify_mesh at the chosen cell {res['cell']:.5f} -> {res['out_vertices']} vertices, {res['out_faces']} faces | {res['simplify_mesh_ms']:.2f} ms |\n")
            fh.write(f"| simplify_to({TARGET}): {res['probes']} probes + the mesh | {res['simplify_to_ms']:.2f} ms |\n")
            fh.write(f"| simplify_mesh at that cell, placement=\"quadric\" | {res['simplify_mesh_quadric_ms']:.2f} ms |\n")
            fh.write(f"| simplify_to({TARGET}), placement=\"quadric\" | {res['simplify_to_quadric_ms']:.2f} ms |\n")
            fh.write(f"| simplify_mesh at that cell, placement=\"mean\", timed again | {res['simplify_mesh_again_ms']:.2f} ms |\n")
            rc = res["report_collapse"]
            fh.write(f"| simplify_collapse({TARGET}) -> {rc['vertices']} vertices, {rc['faces']} faces in {rc['rounds']} rounds ({rc['collapses']} collapses"
                     f"{', stalled' if rc['stalled'] else ''}) | {res['simplify_collapse_ms']:.2f} ms |\n")
            fh.write(f"| simplify_to({TARGET}), timed again after it | {res['simplify_to_again_ms']:.2f} ms |\n")
            fh.write(f"| unwrap_charts({R}) of the collapse's result: {res['collapse_charts']} charts, overlap_texels {res['collapse_overlap_texels']}, "
                     f"{res['collapse_unwrap_rounds']} passes | {res['collapse_unwrap_ms']:.2f} ms |\n")
            fh.write(f"| unwrap_charts({R}) of the clustering's result: {res['charts']} charts, overlap_texels {res['overlap_texels']}, {res['rounds']} passes of the component search | {res['unwrap_ms']:.2f} ms |\n")
            fh.write(f"| of which pack_charts on the host | {res['pack_host_ms']:.2f} ms |\n")
            fh.write(f"| unwrap_charts({R}) of the unsimplified template | {res['unwrap_full_size_ms']:.2f} ms |\n\n")
            fh.write("| placement | clamped | no_planes | flipped | zero_area | max_shift | source -> simplified mean / max | simplified -> source mean / max "
                     "| volume ratio | largest \\| \\|x\\| - 1 \\| of a vertex |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for placement in mesh_prep.PLACEMENTS:
                r, q = res["report_" + placement], res["quality_" + placement]
                fh.write(f"| {placement} | {r['clamped']} | {r['no_planes']} | {r['flipped']} | {r['zero_area']} | {r['max_shift']:.4f} | "
                         f"{q['source_to_simplified']['mean']:.3g} / {q['source_to_simplified']['max']:.3g} | "
                         f"{q['simplified_to_source']['mean']:.3g} / {q['simplified_to_source']['max']:.3g} | {q['volume_ratio']:.6f} | "
                         f"{res['sphere_error_' + placement]:.3g} |\n")
            q = res["quality_collapse"]
            fh.write(f"| (collapse) | - | - | {rc['flipped']} | {rc['zero_area']} | - | {q['source_to_simplified']['mean']:.3g} / {q['source_to_simplified']['max']:.3g} | "
                     f"{q['simplified_to_source']['mean']:.3g} / {q['simplified_to_source']['max']:.3g} | {q['volume_ratio']:.6f} | {res['sphere_error_collapse']:.3g} |\n")
            fh.write("\n")
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
