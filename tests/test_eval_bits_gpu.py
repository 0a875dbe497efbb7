"""The host layer of the geometry evaluation (surfdist_ops.py, winding_ops.py, align.py, evaluate.py),
pinned bit for bit and launch for launch.  Its kernels are held to float64 restatements by tests/test_surfdist_gpu.py, test_icp_gpu.py,
test_icp_search_gpu.py and test_winding_gpu.py; this file holds what the layer above them hands out to the recorded SHA-256 digests of
tests/golden/eval_bits.npz, and counts the index builds of one evaluated frame.

Shapes: the pairs of _icp_ref.case on the n = 16 shape (3072 faces, what the ICP tests use), the UV sphere of test_mesh_bits_gpu with
-1 rows among its faces, its torus wound inward, its open height field, and cube_sphere(16) plus one triangle that spans the box at
cell 0.02 (the cell-doubling loop).  3000 points and samples: no multiple of 256, twelve ICP blocks."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import _icp_ref as ir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3000
ICP = dict(samples=N, iters=12)
SEARCH = dict(candidates=200, search_samples=777, top=3, refine_iters=6)
MESH_INDEX = ("verts", "faces", "tri", "cum_area", "area", "lo", "cell", "n", "nx", "ny", "nz", "cell_start", "cell_faces", "pairs")
WINDING_INDEX = ("verts", "faces", "tri", "corner", "cell", "levels", "nodes", "leaf_start", "leaf_faces", "volume", "flipped")


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def single_meshes():
    """name -> (verts float32, faces int64, cell of the MeshIndex)"""
    from selfreconcode_amd.synthetic import cube_sphere
    import test_mesh_bits_gpu as mb
    m = mb.meshes()
    v, f = [x.numpy() for x in cube_sphere(16)]
    nv = len(v)
    huge = (np.concatenate([v, np.float32([[-1.2, -1.2, -1.2], [1.2, 1.2, -1.2], [1.2, -1.2, 1.2]])]), np.concatenate([f, np.int64([[nv, nv + 1, nv + 2]])]))
    return {"gt": ir.case("rigid", 16)[1] + (None,), "padded": m["padded"][:2] + (None,), "flipped": (m["torus"][0], m["torus"][1][:, ::-1].copy(), None),
            "open": m["boundary"][:2] + (None,), "huge": huge + (0.02,)}


def _query_points(v, seed):
    """[N,3] float32 round the box of v: inside, near and far from the surface, and one NaN row."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    p = 0.5 * (lo + hi) + (hi - lo).max() * rng.uniform(-0.8, 0.8, (N, 3))
    p[N // 2:] = v[rng.integers(0, len(v), N - N // 2)] + 0.01 * rng.normal(size=(N - N // 2, 3))
    p[1234] = np.nan
    return p.astype(np.float32)


def _alignment_dict(a):
    return {"matrix": a.matrix.tolist(), "scale": a.scale, "rotation": a.rotation.tolist(), "translation": a.translation.tolist(),
            "iterations": a.iterations, "converged": a.converged, "rank": a.rank, "pairs": a.pairs, "rms_before": a.rms_before,
            "rms_after": a.rms_after, "history": a.history.tolist(), "search": a.search}


def _write_folder(root, pred, gt):
    """An infer result folder of two frames (the second grown by 1 %) and their ground truth under `root`."""
    from selfreconcode_amd.mesh_io import write_ply
    rec, gtd = os.path.join(root, "result"), os.path.join(root, "gt")
    os.makedirs(os.path.join(rec, "meshs"))
    os.makedirs(gtd)
    write_ply(os.path.join(rec, "tmp.ply"), pred[0], pred[1])
    for fid, grow in ((0, 1.), (12, 1.01)):
        np.save(os.path.join(rec, "meshs", "%d.npy" % fid), (pred[0] * np.float32(grow)).astype(np.float32))
        write_ply(os.path.join(gtd, "%d.ply" % fid), gt[0], gt[1])
    return rec, gtd


def eval_digests(tmp):
    """name -> SHA-256 (as 32 uint8), in a fixed order, of what the evaluation stack hands out: every public field of both indices,
    closest_point, sample_surface, winding_number, the Alignment of icp_align from every kind of start, surface_metrics,
    vertex_to_surface, an error-mesh PLY, and the files and printed lines of the command in both modes.  `tmp` is an empty folder for
    the files (its name is taken out of the printed lines).  oracle/gen_eval_bits_golden.py records what this returns."""
    from selfreconcode_amd import evaluate, surfdist_ops as sd, winding_ops as wn
    from selfreconcode_amd.align import icp_align
    from selfreconcode_amd.mesh_io import write_ply
    out = {}

    def put(name, t):
        if isinstance(t, (dict, list, tuple, float, int, bool)):
            t = json.dumps(t, sort_keys=True).encode()
        raw = t if isinstance(t, bytes) else t.detach().cpu().contiguous().numpy().tobytes()
        assert name not in out
        out[name] = torch.from_numpy(np.frombuffer(hashlib.sha256(raw).digest(), np.uint8).copy())

    def put_all(name, tensors):
        for k, t in enumerate(tensors if isinstance(tensors, (tuple, list)) else (tensors,)):
            put(f"{name}_{k}", t)

    def put_lines(name, lines):
        put(name, [ln.replace(str(tmp), "TMP") for ln in lines])

    for name, (v, f, cell) in single_meshes().items():
        tv, tf = _t(v), _t(f)
        index, pyramid = sd.MeshIndex.build(tv, tf, cell), wn.WindingIndex.build(tv, tf)
        if name == "huge":
            assert index.cell > 0.02                                                      # the cell was doubled
        assert pyramid.flipped or name != "flipped"
        for k in MESH_INDEX:
            put(f"{name}_grid_{k}", getattr(index, k))
        put(f"{name}_grid_face_normals", index.face_normals())
        for k in WINDING_INDEX:
            put(f"{name}_pyramid_{k}", getattr(pyramid, k))
        p = _t(_query_points(v, 7))
        put_all(f"{name}_closest_grid", sd.closest_point(p, index))
        put_all(f"{name}_closest_unsorted", sd.closest_point(p, index, presort=False))
        put_all(f"{name}_closest_brute", sd.closest_point(p, index, method="brute"))
        put_all(f"{name}_sample", sd.sample_surface(tv, tf, N, 3))
        put_all(f"{name}_sample_cum", sd.sample_surface(tv, tf, N, 4, cum_area=index.cum_area))
        put(f"{name}_winding_tree", wn.winding_number(p, pyramid))
        put(f"{name}_winding_unsorted", wn.winding_number(p, pyramid, presort=False))
        put(f"{name}_winding_brute", wn.winding_number(p, pyramid, method="brute"))
        put(f"{name}_winding_inf", wn.winding_number(p, pyramid, beta=float("inf")))
        put_all(f"{name}_signed_distance", evaluate.signed_distance(p, index, pyramid))
    tv, tf = [_t(x) for x in single_meshes()["gt"][:2]]
    put_all("gt_pyramid_levels2", [getattr(wn.WindingIndex.build(tv, tf, levels=2), k) for k in ("nodes", "leaf_start", "leaf_faces", "cell")])
    put_all("gt_pyramid_leaf1", [getattr(wn.WindingIndex.build(tv, tf, leaf_factor=1.), k) for k in ("nodes", "leaf_start", "leaf_faces", "levels")])

    pairs = {}
    for name in ("rigid", "similarity"):
        pred, gt, answer = ir.case(name, 16)
        dp, dg = (_t(pred[0]), _t(pred[1])), (_t(gt[0]), _t(gt[1]))
        pairs[name] = (dp, dg)
        start = ir.truth_matrix(answer)
        start[:3, 3] += 0.01
        for label, init in (("centroid", "centroid"), ("none", "none"), ("axes", "axes"), ("search", "search"), ("matrix", start)):
            put(f"{name}_icp_{label}", _alignment_dict(icp_align(dp, dg, scale=name == "similarity", init=init, **ICP, **SEARCH)))
    put("rigid_icp_max_dist", _alignment_dict(icp_align(*pairs["rigid"], max_dist=0.1, seed=5, **ICP)))

    dp, dg = pairs["rigid"]
    common = dict(samples=N, seed=3, taus=(0.02, 0.1))
    put("metrics_plain", evaluate.surface_metrics(dp, dg, **common))
    put("metrics_rigid", evaluate.surface_metrics(dp, dg, align="rigid", align_opts=ICP, **common))
    put("metrics_search", evaluate.surface_metrics(dp, dg, align="rigid", align_opts=dict(ICP, init="search", **SEARCH), **common))
    put("metrics_signed", evaluate.surface_metrics(dp, dg, signed=True, **common))
    put("metrics_rigid_signed", evaluate.surface_metrics(dp, dg, align="rigid", align_opts=ICP, signed=True, beta=2.5, **common))
    found = icp_align(*pairs["similarity"], scale=True, **ICP)
    put("metrics_given_alignment", evaluate.surface_metrics(*pairs["similarity"], align=found, **common))
    m = single_meshes()
    padded, flipped = (_t(m["padded"][0]), _t(m["padded"][1])), (_t(m["flipped"][0]), _t(m["flipped"][1]))
    put("metrics_padded_flipped_signed", evaluate.surface_metrics(padded, flipped, signed=True, **common))
    put("vertex_plain", evaluate.vertex_to_surface(dp[0], dg))
    put("vertex_signed", evaluate.vertex_to_surface(dp[0], dg, signed=True))
    put("vertex_rigid_signed", evaluate.vertex_to_surface(dp[0], dg, align="rigid", align_opts=ICP, faces=dp[1], signed=True))
    put("vertex_given_alignment", evaluate.vertex_to_surface(pairs["similarity"][0][0], pairs["similarity"][1], align=found))
    put("vertex_flipped_signed", evaluate.vertex_to_surface(padded[0], flipped, signed=True))
    lines, ply = [], os.path.join(tmp, "error.ply")
    put("error_mesh_limit", evaluate.write_error_mesh(ply, pairs["similarity"][0], pairs["similarity"][1], found, True, 3.0, None, lines.append))
    put("error_mesh_ply", open(ply, "rb").read())
    put_lines("error_mesh_lines", lines)

    pred, gt, _ = ir.case("similarity", 8)                                                 # mesh-pair mode
    a, b, e, js = [os.path.join(tmp, x) for x in ("a.ply", "b.ply", "e.ply", "m.json")]
    write_ply(a, pred[0], pred[1])
    write_ply(b, gt[0], gt[1])
    lines = []
    put("pair_result", evaluate.main(["--pred", a, "--gt", b, "--samples", str(N), "--tau", "0.05", "--align", "similarity", "--align-samples", "2003",
                                      "--align-iters", "12", "--signed", "--error-mesh", e, "--out", js], out=lines.append))
    put_lines("pair_lines", lines)
    put("pair_error_mesh", open(e, "rb").read())
    put("pair_json", open(js, "rb").read())

    pred, gt, _ = ir.case("rigid", 8)                                                      # folder mode
    rec, gtd = _write_folder(tmp, pred, gt)
    lines = []
    put("folder_result", evaluate.main(["--rec-root", rec, "--gt-root", gtd, "--samples", str(N), "--align", "rigid", "--align-samples", "2003",
                                        "--align-iters", "12", "--align-shared", "--signed", "--error-meshes"], out=lines.append))
    put_lines("folder_lines", lines)
    for k in ("geometry_errors.txt", "geometry_errors.json", "geometry_signed.txt", "geometry_errors/0.ply", "geometry_errors/12.ply"):
        put("folder_" + k, open(os.path.join(rec, k), "rb").read())
    return out


def test_the_evaluation_stack_gives_the_recorded_bits(golden, tmp_path):
    """tests/golden/eval_bits.npz holds the digests that oracle/gen_eval_bits_golden.py recorded with surfdist_ops.py, winding_ops.py,
    align.py and evaluate.py as they were before a mesh was prepared once and shared (surfdist_ops.Surface); a change that means to
    keep the bits does not record it again."""
    g, out = golden("eval_bits")["digests"], eval_digests(tmp_path)
    assert g.shape == (len(out), 32) and len(out) == 5 * (14 + 1 + 11 + 3 * 3 + 2 * 3 + 4 + 2) + 2 * 4 + 2 * 5 + 1 + 7 + 5 + 3 + 4 + 2 + 5
    for want, (k, v) in zip(g, out.items()):
        assert torch.equal(v, want), k


def _counted(monkeypatch, args):
    """The events of one run of the command: ("launch", entry point) per _lib.launch and ("line", text) per printed line, in order."""
    from selfreconcode_amd import _lib, evaluate
    events, launch = [], _lib.launch

    def counting(name, on, *rest):
        events.append(("launch", name))
        launch(name, on, *rest)

    monkeypatch.setattr(_lib, "launch", counting)
    evaluate.main(args, out=lambda text: events.append(("line", text)))
    monkeypatch.setattr(_lib, "launch", launch)
    return events


def test_a_frame_builds_each_index_once(monkeypatch, tmp_path):
    """Folder mode with --align rigid --signed --error-meshes builds per frame two grids (sr_surfdist_emit_pairs: ground truth,
    aligned prediction) and two pyramids (sr_winding_leaves); --align-init search needs one more grid, of the unaligned prediction;
    with --align-shared the second frame runs no ICP launch.  Before the ground truth was prepared once per file (surfdist_ops.Surface)
    the counts were four grids and three pyramids per frame."""
    pred, gt, _ = ir.case("rigid", 8)
    rec, gtd = _write_folder(str(tmp_path), pred, gt)
    base = ["--rec-root", rec, "--gt-root", gtd, "--samples", str(N), "--align", "rigid", "--align-samples", "2003", "--align-iters", "12",
            "--signed", "--error-meshes"]

    def count(events, name):
        return sum(e == ("launch", name) for e in events)

    one = _counted(monkeypatch, base + ["--frames", "1"])
    assert count(one, "sr_surfdist_emit_pairs") == 2 and count(one, "sr_winding_leaves") == 2 and count(one, "sr_icp_solve") == 12
    search = _counted(monkeypatch, base + ["--frames", "1", "--align-init", "search", "--align-candidates", "200", "--align-top", "3"])
    assert count(search, "sr_surfdist_emit_pairs") == 3 and count(search, "sr_winding_leaves") == 2
    shared = _counted(monkeypatch, base + ["--align-shared"])
    assert count(shared, "sr_surfdist_emit_pairs") == 4 and count(shared, "sr_winding_leaves") == 4
    first = next(k for k, e in enumerate(shared) if e[0] == "line" and e[1].startswith("   0: chamfer"))
    assert any(e[1].startswith("  12: chamfer") for e in shared[first:] if e[0] == "line")
    assert count(shared[:first], "sr_icp_solve") == 12 and not [e for e in shared[first:] if e[0] == "launch" and e[1].startswith("sr_icp_")]
