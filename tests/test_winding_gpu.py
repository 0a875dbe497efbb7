"""Winding-number inside / outside test on the GPU (csrc/winding.hip, winding_ops, evaluate) against the numpy restatement
of tests/_winding_ref.py in float64.

Bound of the float64 comparisons of w: max(4 E32, 8 2^-23), E32 the largest error of the float32 twin of the exact sum against the
float64 one on the same input (the noise floor of the number format, independent of the kernels; w is of order 1); the factor 4 covers
another atan2f and another order of the same sum.  The tree is compared with the restatement of the same tree: same keys, same runs,
node arrays to the float32 rounding of double sums, and w of the restated walk over the kernel's own node array, so that both take the
float32 acceptance test on the same numbers.  Every comparison prints measured / bound."""
import json
import os

import numpy as np
import pytest
import torch

import _meshprep_ref as mr
import _winding_ref as wr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2. ** -23
_CACHE = {}


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _sphere(n, jittered=True):
    from selfreconcode_amd.synthetic import cube_sphere
    key = ("sphere", n, jittered)
    if key not in _CACHE:
        v, f = [x.numpy() for x in cube_sphere(n)]
        _CACHE[key] = (mr.jitter(v, 5, 0.004) if jittered else v, f)
    return _CACHE[key]


def _mesh(name):
    """The meshes of the cases, (verts float32, faces int64) each."""
    if name in _CACHE:
        return _CACHE[name]
    v8, f8 = _sphere(8)
    v16, f16 = _sphere(16)
    if name == "sphere8":
        m = (v8, f8)
    elif name == "one":
        m = (v8, f8[:1])
    elif name == "f257":
        m = (v8, f8[:257])
    elif name == "sphere16":
        m = (v16, f16)
    elif name == "open":
        m = (v16, wr.open_sphere(v16, f16))
    elif name == "two":                                      # two spheres far apart: almost every node is empty
        m = (np.concatenate([v8, 0.05 * v8 + 5.]).astype(np.float32), np.concatenate([f8, f8 + len(v8)]))
    elif name == "spanning":                                 # one triangle through the whole box: its nodes' radius is the box's
        nv = len(v16)
        m = (np.concatenate([v16, np.float32([[-1.2, -1.2, -1.2], [1.2, 1.2, -1.2], [1.2, -1.2, 1.2]])]),
             np.concatenate([f16, np.int64([[nv, nv + 1, nv + 2]])]))
    elif name == "degenerate":                               # -1 rows and faces without area among real ones
        nv = len(v16)
        m = (np.concatenate([v16, np.float32([[0.3, 0.3, 0.3], [0.5, 0.5, 0.5], [0.7, 0.7, 0.7]])]),
             np.concatenate([f16[:50], np.int64([[3, 3, 9], [-1, -1, -1], [nv, nv + 1, nv + 2], [5, 5, 5], [-1, -1, -1]]), f16[50:], np.int64([[-1, -1, -1]])]))
    _CACHE[name] = m
    return m


def _points(name):
    """300 points (two workgroups, the second partial): 297 on the eight shells, a NaN point, a vertex, and a point of the first
    face's plane outside the face; for the two spheres, some of the shell points go round the small one."""
    key = ("points", name)
    if key not in _CACHE:
        v, f = _mesh(name)
        f = wr.clean(f)
        p = wr.shell_points(297, 11)
        if name == "two":
            p[200:] = p[200:] * np.float32(0.05) + np.float32(5.)
        a, b, c = v[f[0]]
        _CACHE[key] = np.concatenate([p, np.float32([[np.nan, 0., 0.]]), v[f[0, 1]][None], (a + 3 * (b - a) + 2 * (c - a))[None]]).astype(np.float32)
    return _CACHE[key]


def _reference(name):
    """(w64 [300], bound) of the exact sum of the case, computed once."""
    key = ("ref", name)
    if key not in _CACHE:
        v, f = _mesh(name)
        w64, e32 = wr.e32(_points(name), v, wr.clean(f))
        _CACHE[key] = (w64, max(4. * e32, 8. * EPS), e32)
    return _CACHE[key]


def _index(name, levels=None):
    from selfreconcode_amd import winding_ops as wn
    key = ("index", name, levels)
    if key not in _CACHE:
        v, f = _mesh(name)
        _CACHE[key] = wn.WindingIndex.build(_t(v), _t(f), levels=levels)
    return _CACHE[key]


def _bits(x):
    return x.view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("name", ["sphere8", "one", "f257"])
def test_brute_vs_float64(name):
    from selfreconcode_amd import winding_ops as wn
    v, f = _mesh(name)
    assert len(f) == {"sphere8": 768, "one": 1, "f257": 257}[name]
    p = _points(name)
    assert p.shape == (300, 3)
    w64, bound, e32 = _reference(name)
    w = wn.winding_number(_t(p), _index(name, 0), method="brute")
    assert w.dtype == torch.float32 and w.shape == (300,)
    w = w.cpu().numpy().astype(np.float64)
    assert np.isnan(w[297]) and np.isnan(w64[297]) and np.isfinite(np.delete(w, 297)).all()
    err = float(np.nanmax(np.abs(w - w64)))
    print(f"brute {name}: max |w - w64| {err:.3g} (bound {bound:.3g}, E32 {e32:.3g})")
    assert err <= bound
    if name == "sphere8":
        r = np.linalg.norm(p[:297], axis=1)
        assert np.array_equal(w[:297] >= 0.5, r < 1.) and abs(w[:297][r < 0.95] - 1.).max() < 1e-5 and abs(w[:297][r > 1.05]).max() < 1e-5


CASES = [("sphere16", 0), ("sphere16", 1), ("sphere16", None), ("sphere16", 5), ("two", None), ("spanning", None), ("degenerate", None), ("open", None)]


@pytest.mark.parametrize("name, levels", CASES)
def test_tree_vs_restated_tree(name, levels):
    from selfreconcode_amd import winding_ops as wn
    v, f = _mesh(name)
    index, tree = _index(name, levels), wr.build_tree(v, f, levels)
    assert index.levels == tree["levels"] == (levels if levels is not None else index.levels) and index.cell == tree["cell"]
    if name == "sphere16":
        assert index.levels == (4 if levels is None else levels)
    assert np.array_equal(index.corner.cpu().numpy(), tree["corner"])
    assert np.array_equal(index.leaf_start.cpu().numpy(), tree["leaf_start"]) and np.array_equal(index.leaf_faces.cpu().numpy(), tree["leaf_faces"])
    assert index.faces.shape[0] == len(tree["faces"]) == int(tree["leaf_start"][-1])
    nodes = index.nodes.cpu().numpy()
    assert nodes.shape == tree["nodes"].shape == (wr.level_offset(index.levels + 1), 8)
    worst = 0.
    for cols in (slice(0, 3), slice(3, 6), slice(6, 7), slice(7, 8)):                     # N, c, A, r: each against its own magnitude
        scale = float(np.abs(tree["nodes"][:, cols]).max())
        worst = max(worst, float(np.abs(nodes[:, cols].astype(np.float64) - tree["nodes"][:, cols]).max()) / scale)
    occupied = float((nodes[wr.level_offset(index.levels):, 6] > 0).mean())
    print(f"tree {name} levels {index.levels}: nodes differ by {worst / EPS:.2f} 2^-23 of their column's largest (bound 4); {occupied:.3f} of the leaves hold area")
    assert worst <= 4. * EPS
    if name == "two":
        assert occupied < 0.05
    if name == "spanning":
        assert float(nodes[:, 7].max()) > 1.5
    p = _points(name)
    _, bound, e32 = _reference(name)
    for beta in (wn.BETA, 1.0):
        counts = {}
        want = wr.tree_query(p, tree, beta, nodes=nodes, counts=counts)
        w = wn.winding_number(_t(p), index, beta=beta).cpu().numpy().astype(np.float64)
        assert np.isnan(w[297]) and np.isnan(want[297])
        err = float(np.nanmax(np.abs(w - want)))
        print(f"tree {name} levels {index.levels} beta {beta}: max |w - restated walk| {err:.3g} (bound {bound:.3g}, E32 {e32:.3g}); accepted nodes per point "
              f"up to {counts['accepted'].max()}, exact faces up to {counts['faces'].max()}")
        assert err <= bound
    if levels == 0:
        assert index.nodes.shape[0] == 1 and counts["accepted"].max() == 1


def test_beta_inf_opens_every_leaf():
    from selfreconcode_amd import winding_ops as wn
    p = _t(_points("sphere8"))
    for levels in (None, 1):
        index = _index("sphere8", levels)
        a, b = wn.winding_number(p, index, beta=float("inf")), wn.winding_number(p, index, method="brute")
        err = float((a - b)[torch.isfinite(b)].abs().max())
        print(f"beta inf vs brute, cube_sphere(8), {index.levels} levels: max |dw| {err:.3g} (bound {2 * EPS:.3g}: the same float32 terms, summed in double in another order)")
        assert err <= 2. * EPS and bool(torch.isnan(a[297]))


@pytest.mark.parametrize("name", ["sphere8", "sphere16", "two"])
def test_tree_decisions_equal_brute_on_closed_meshes(name):
    from selfreconcode_amd import winding_ops as wn
    p = _t(_points(name)[:297])
    index = _index(name)
    tree, brute = wn.winding_number(p, index), wn.winding_number(p, index, method="brute")
    err = float((tree - brute).abs().max())
    print(f"tree vs brute {name}, {index.levels} levels, beta {wn.BETA}: max |dw| {err:.3g} (the condition on the approximation is 0.05)")
    assert err <= 0.05 and torch.equal(tree >= 0.5, brute >= 0.5)


def test_flipped_faces_give_the_same_signs():
    from selfreconcode_amd import surfdist_ops as sd, winding_ops as wn
    from selfreconcode_amd.evaluate import signed_distance
    v, f = _mesh("sphere16")
    p = _t(_points("sphere16"))
    out, back = _index("sphere16"), wn.WindingIndex.build(_t(v), _t(np.ascontiguousarray(f[:, ::-1])))
    assert not out.flipped and back.flipped and out.volume > 4. and back.volume < -4. and abs(out.volume + back.volume) < 1e-9
    mesh = sd.MeshIndex.build(_t(v), _t(f))
    (s0, w0), (s1, w1) = signed_distance(p, mesh, out), signed_distance(p, mesh, back)
    assert torch.equal(_bits(s0[:298]), _bits(s1[:298]))                          # (the last two points lie on the surface, where w is 1/2)
    assert float((w0 - w1)[:297].abs().max()) <= 2. * _reference("sphere16")[1]   # (the flipped corners enter the denominator in another order)
    r = torch.linalg.norm(p[:297], dim=1)
    assert torch.equal(s0[:297] < 0, r < 1.) and bool(torch.isnan(s0[297])) and bool(torch.isnan(w0[297]))
    assert torch.equal(s0.abs()[:297], sd.closest_point(p, mesh)[0][:297])
    from selfreconcode_amd.evaluate import _signed
    z = _signed(torch.tensor([0., 0., 1., 1.], device=DEV), torch.tensor([1., 0., 1., 0.], device=DEV)).cpu().numpy()
    assert z.tolist() == [0., 0., -1., 1.] and not np.signbit(z[:2]).any()        # a distance of 0 stays +0


def test_two_calls_and_presort_give_identical_bits():
    from selfreconcode_amd import winding_ops as wn
    v, f = _mesh("sphere16")
    p = _t(_points("sphere16"))
    a, b = _index("sphere16"), wn.WindingIndex.build(_t(v), _t(f))
    assert torch.equal(_bits(a.nodes), _bits(b.nodes)) and torch.equal(a.leaf_start, b.leaf_start) and torch.equal(a.leaf_faces, b.leaf_faces)
    w = wn.winding_number(p, a)
    for other in (wn.winding_number(p, b), wn.winding_number(p, a, presort=False), wn.winding_number(p.flip(0), a).flip(0)):
        assert torch.equal(_bits(w), _bits(other))
    u = wn.winding_number(p, a, method="brute")
    assert torch.equal(_bits(u), _bits(wn.winding_number(p.flip(0), a, method="brute").flip(0)))


def test_conventions_and_refusals():
    from selfreconcode_amd import _lib, winding_ops as wn
    v, f = _mesh("sphere8")
    index = _index("sphere8")
    for method in ("tree", "brute"):
        w = wn.winding_number(torch.zeros((0, 3), device=DEV), index, method=method)
        assert w.shape == (0,) and w.dtype == torch.float32
    p = _t(_points("sphere8"))
    for bad in (0.5, -1., float("nan")):
        with pytest.raises(ValueError):
            wn.winding_number(p, index, beta=bad)
    with pytest.raises(ValueError):
        wn.winding_number(p, index, method="bvh")
    with pytest.raises(ValueError):
        wn.winding_number(p[:, :2], index)
    with pytest.raises(RuntimeError):
        wn.winding_number(p.cpu(), index)
    for levels in (-1, 8):
        with pytest.raises(ValueError):
            wn.WindingIndex.build(_t(v), _t(f), levels=levels)
    with pytest.raises(ValueError):
        wn.WindingIndex.build(_t(v), _t(np.int64([[-1, -1, -1]])))
    with pytest.raises(ValueError):
        wn.WindingIndex.build(_t(v), _t(np.int64([[0, 1, len(v)]])))
    # the entry points refuse before any launch: a misaligned tri, bad sizes, a level outside the range
    w = torch.empty((300,), dtype=torch.float32, device=DEV)
    off = torch.zeros((index.tri.numel() + 1,), dtype=torch.float32, device=DEV)[1:]
    assert off.data_ptr() % 16 == 4
    F = index.faces.shape[0]
    for name, args in (("sr_winding_brute", (p, 300, off, F, w)), ("sr_winding_brute", (p, 0, index.tri, F, w)), ("sr_winding_brute", (p, 300, index.tri, 0, w)),
                       ("sr_winding_query", (p, 300, off, F, index.nodes, index.levels, index.leaf_start, index.leaf_faces, 3., 0, w)),
                       ("sr_winding_query", (p, 300, index.tri, F, index.nodes, 8, index.leaf_start, index.leaf_faces, 3., 0, w)),
                       ("sr_winding_query", (p, 300, index.tri, F, index.nodes, index.levels, index.leaf_start, index.leaf_faces, 0.5, 0, w)),
                       ("sr_winding_leaves", (off, F, index.leaf_start, index.leaf_faces, index.levels, index.nodes)),
                       ("sr_winding_fold", (index.nodes, index.levels, index.levels)),
                       ("sr_winding_keys", (off, F, 1, index.corner, index.cell, index.levels, index.leaf_start))):
        with pytest.raises(_lib.SrError, match="SR_EINVAL"):
            _lib.launch(name, p, *args)


# ------------------------------------------------------------------------------------------------------------ metrics, command
def _pair():
    """pred: cube_sphere(16) x 0.95; gt: cube_sphere(12), whose faces' planes pass the origin at 0.99 or more (a face sags by 0.007
    at the most below the unit sphere): every pred sample, at radius 0.95 or less, is strictly inside."""
    (pv, pf), (gv, gf) = _sphere(16, jittered=False), _sphere(12, jittered=False)
    t = gv.astype(np.float64)[gf]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    sag = 1. - float(((n * t[:, 0]).sum(1) / np.linalg.norm(n, axis=1)).min())
    print(f"cube_sphere(12): the faces sag by at most {sag:.4f}")
    assert 0. < sag < 0.01
    return ((pv * np.float32(0.95)).astype(np.float32), pf), (gv, gf)


def test_surface_metrics_signed():
    from selfreconcode_amd.evaluate import surface_metrics
    pred, gt = _pair()
    dp, dg = (_t(pred[0]), _t(pred[1])), (_t(gt[0]), _t(gt[1]))
    n, taus = 20011, (0.06,)
    plain = surface_metrics(dp, dg, samples=n, seed=3, taus=taus)
    assert "signed" not in plain and surface_metrics(dp, dg, samples=n, seed=3, taus=taus, signed=False) == plain
    got = surface_metrics(dp, dg, samples=n, seed=3, taus=taus, signed=True)
    assert got == surface_metrics(dp, dg, samples=n, seed=3, taus=taus, signed=True, beta=3.0)
    block = got.pop("signed")
    assert got == plain                                                            # everything else is bit for bit what it was
    print("signed block:", json.dumps(block))
    assert block["pred_to_gt"]["inside_share"] == 1. and block["pred_to_gt"]["mean"] == -plain["pred_to_gt"]["mean"] < -0.04
    assert block["gt_to_pred"]["inside_share"] == 0. and block["gt_to_pred"]["mean"] == plain["gt_to_pred"]["mean"] > 0.04
    sphere = 4. / 3. * np.pi
    assert 0.97 * sphere * 0.95 ** 3 < block["volume_pred"] < sphere * 0.95 ** 3 and 0.97 * sphere < block["volume_gt"] < sphere
    swapped = surface_metrics(dg, dp, samples=n, seed=3, signed=True)["signed"]
    assert swapped["pred_to_gt"]["inside_share"] == 0. and swapped["pred_to_gt"]["mean"] > 0.04
    assert swapped["gt_to_pred"]["inside_share"] == 1. and swapped["gt_to_pred"]["mean"] < -0.04
    assert swapped["volume_pred"] == block["volume_gt"] and swapped["volume_gt"] == block["volume_pred"]


def _ply_colors(path, V):
    lines = open(path).read().splitlines()
    head = lines.index("end_header")
    assert lines[:head].count("property uchar red") == 1 and "element vertex %d" % V in lines[:head]
    return np.array([ln.split()[3:6] for ln in lines[head + 1:head + 1 + V]], dtype=np.int64)


def test_command_signed_error_mesh(tmp_path):
    from selfreconcode_amd import evaluate
    from selfreconcode_amd.mesh_io import read_ply, write_ply
    from selfreconcode_amd.synthetic import icosphere
    v, f = [x.numpy() for x in icosphere(2)]
    pv = (v * np.float32([1.1, 0.9, 1.0])).astype(np.float32)                      # outside along x, inside along y
    a, b, e = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "e.ply")
    write_ply(a, pv, f)
    write_ply(b, v, f)
    lines = []
    base = ["--gpu-ids", "0", "--pred", a, "--gt", b, "--samples", "5003", "--seed", "2"]
    got = evaluate.main(base + ["--signed", "--error-mesh", e, "--error-range", "0.08"], out=lines.append)
    assert len(lines) == 1 and json.loads(lines[0]) == got and 0. < got["signed"]["pred_to_gt"]["inside_share"] < 1.
    plain = evaluate.main(base, out=lines.append)
    assert "signed" not in plain and {k: x for k, x in got.items() if k != "signed"} == plain
    d = evaluate.vertex_to_surface(_t(pv), (_t(v), _t(f)), signed=True)
    assert float(d.min()) < -0.05 and float(d.max()) > 0.05
    want = evaluate.error_colors(d, 0.08, True).cpu().numpy()
    colors = _ply_colors(e, len(v))
    assert np.array_equal(colors, want) and (colors[:, 2] < 100).any() and (colors[:, 0] < 100).any()          # red and blue vertices
    rv, rf = read_ply(e)
    assert np.array_equal(rv, pv) and np.array_equal(rf, f)
    lines = []
    evaluate.main(base + ["--error-mesh", e], out=lines.append)                   # unsigned, default range: printed
    d = evaluate.vertex_to_surface(_t(pv), (_t(v), _t(f)))
    limit = evaluate.error_range(d)
    assert len(lines) == 2 and lines[1].strip().startswith("error range %.6g" % limit)
    colors = _ply_colors(e, len(v))
    assert np.array_equal(colors, evaluate.error_colors(d, limit, False).cpu().numpy()) and (colors[:, 0] == 255).all()


def test_command_folder_mode_signed_error_meshes(tmp_path):
    from selfreconcode_amd import evaluate
    from selfreconcode_amd.mesh_io import write_ply
    from selfreconcode_amd.synthetic import icosphere
    v, f = [x.numpy() for x in icosphere(2)]
    rec, gt = tmp_path / "result", tmp_path / "gt"
    os.makedirs(rec / "meshs")
    os.makedirs(gt)
    write_ply(str(rec / "tmp.ply"), v, f)
    for fid, scale in ((0, 0.9), (7, 1.02), (12, 1.1)):
        np.save(str(rec / "meshs" / ("%d.npy" % fid)), (v * scale).astype(np.float32))
    write_ply(str(gt / "0.ply"), v, f)
    write_ply(str(gt / "12.ply"), v, f)
    lines = []
    got = evaluate.main(["--rec-root", str(rec), "--gt-root", str(gt), "--samples", "3001", "--signed", "--error-meshes"], out=lines.append)
    assert list(got["frames"]) == ["0", "12"] and json.load(open(rec / "geometry_errors.json")) == got
    s0, s12 = got["frames"]["0"]["signed"], got["frames"]["12"]["signed"]
    assert s0["pred_to_gt"]["inside_share"] == 1. and s0["pred_to_gt"]["mean"] < -0.05 and s12["pred_to_gt"]["inside_share"] == 0. and s12["pred_to_gt"]["mean"] > 0.05
    assert sum(x.startswith("      signed pred_to_gt ") for x in lines) == 2 and sum("error range" in x for x in lines) == 2
    txt = open(rec / "geometry_signed.txt").read().splitlines()
    assert len(txt) == 5 and txt[0] == "      pred_to_gt gt_to_pred" and txt[1].startswith("   0: -") and txt[2].startswith("  12: ")
    assert "%.6f" % s12["pred_to_gt"]["mean"] in txt[2] and txt[3].startswith("pred_to_gt mean: ") and txt[3].rstrip().endswith("maxinds:1 0")
    assert len(open(rec / "geometry_errors.txt").read().splitlines()) == 5
    assert sorted(os.listdir(rec / "geometry_errors")) == ["0.ply", "12.ply"]
    c0, c12 = _ply_colors(str(rec / "geometry_errors" / "0.ply"), len(v)), _ply_colors(str(rec / "geometry_errors" / "12.ply"), len(v))
    assert (c0[:, 2] == 255).all() and (c0[:, 0] < 255).all() and (c12[:, 0] == 255).all() and (c12[:, 2] < 255).all()
    lines = []
    plain = evaluate.main(["--rec-root", str(rec), "--gt-root", str(gt), "--samples", "3001"], out=lines.append)
    assert not os.path.exists(rec / "geometry_plain") and all("signed" not in m for m in plain["frames"].values()) and len(lines) == 3
