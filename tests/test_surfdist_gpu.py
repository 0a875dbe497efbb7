"""Surface-distance evaluation on the GPU (csrc/surfdist.hip, surfdist_ops, evaluate) against the numpy restatement of
tests/_surfdist_ref.py in float64, and the grid query against the brute-force kernel bit for bit at sizes the CPU cannot afford.

Bound of the float64 comparisons: max(4 E32, 8 2^-23 scale), E32 the largest error of the float32 restatement against the float64 one on
the same input (the noise floor of the number format, independent of the kernels), scale the largest absolute coordinate; the factor 4
covers contraction and another evaluation order of the same formula.  Every comparison prints measured / bound."""
import json
import os

import numpy as np
import pytest
import torch

import _meshprep_ref as mr
import _surfdist_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELLS = (0.05, 0.11, 0.7, 3.0)
EPS = 2. ** -23
_CACHE = {}


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _sphere(n, jittered=True):
    from selfreconcode_amd.synthetic import cube_sphere
    key = ("sphere", n, jittered)
    if key not in _CACHE:
        v, f = [x.numpy() for x in cube_sphere(n)]
        _CACHE[key] = (mr.jitter(v, 5, 0.004) if jittered else v, f)
    return _CACHE[key]


def _index(name, v, f, cell):
    from selfreconcode_amd import surfdist_ops as sd
    key = ("index", name, cell)
    if key not in _CACHE:
        _CACHE[key] = sd.MeshIndex.build(_t(v), _t(f), cell)
    return _CACHE[key]


def _point_sets():
    """Five sets against the jittered cube_sphere(16): 1031 points each (not a multiple of 64), 64 for the centre."""
    if "sets" not in _CACHE:
        v, _ = _sphere(16)
        rng = np.random.default_rng(7)
        dirs = np.float64([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)])
        lo, parts = v.min(0), []
        for cell, m in zip(CELLS, (258, 258, 258, 257)):                 # points exactly on cell boundaries lo + k cell, every cell size
            k = rng.integers(0, int(2.1 / cell) + 2, (m, 3)).astype(np.float32)
            parts.append(lo + np.float32(cell) * k)
        _CACHE["sets"] = {
            "shell": (_unit(rng.normal(size=(1031, 3))) * rng.uniform(0.9, 1.1, (1031, 1))).astype(np.float32),
            "vertices": v[:1031].copy(),
            "far": (20. * _unit(np.concatenate([dirs, rng.normal(size=(1031 - 26, 3))]))).astype(np.float32),
            "centre": (1e-3 * rng.uniform(-0.5, 0.5, (64, 3))).astype(np.float32),
            "boundary": np.concatenate(parts).astype(np.float32)}
    return _CACHE["sets"]


def _reference(name):
    """(d64, bound) of a point set against the jittered cube_sphere(16), computed once."""
    key = ("ref", name)
    if key not in _CACHE:
        v, f = _sphere(16)
        p = _point_sets()[name]
        d64 = sr.closest(p, v, f)[0]
        e32 = float(np.abs(sr.closest(p, v, f, np.float32)[0].astype(np.float64) - d64).max())
        scale = max(float(np.abs(p).max()), float(np.abs(v).max()))
        _CACHE[key] = (d64, max(4. * e32, 8. * EPS * scale), e32, scale)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("cell", CELLS + (None,))
@pytest.mark.parametrize("name", ["shell", "vertices", "far", "centre", "boundary"])
def test_closest_point_vs_float64(name, cell):
    from selfreconcode_amd import surfdist_ops as sd
    v, f = _sphere(16)
    assert len(v) == 1538 and len(f) == 3072
    p = _point_sets()[name]
    assert len(p) == (64 if name == "centre" else 1031)
    d64, bound, e32, scale = _reference(name)
    index = _index("sphere16", v, f, cell)
    if cell is not None:
        assert index.cell == float(np.float32(cell))
        assert (index.nx * index.ny * index.nz == 1) == (cell == 3.0)
    dist, face, closest = [x.cpu().numpy() for x in sd.closest_point(_t(p), index)]
    assert dist.dtype == np.float32 and face.dtype == np.int64 and closest.dtype == np.float32
    assert dist.shape == (len(p),) and face.shape == (len(p),) and closest.shape == (len(p), 3)
    assert face.min() >= 0 and face.max() < len(f)
    err_d = float(np.abs(dist.astype(np.float64) - d64).max())
    err_face = float((sr.face_distance(p, v, f, face) - d64).max())
    err_on = float(sr.face_distance(closest, v, f, face).max())
    err_pq = float(np.abs(np.linalg.norm(p.astype(np.float64) - closest.astype(np.float64), axis=1) - dist).max())
    print(f"closest_point {name} cell {cell} (grid {index.n}, {index.pairs} pairs): |dist - d64| {err_d:.3g}, reported face {err_face:.3g}, "
          f"closest on face {err_on:.3g}, |p - closest| - dist {err_pq:.3g}; bound {bound:.3g} (E32 {e32 / EPS / scale:.2f} 2^-23 scale)")
    assert err_d <= bound and err_face <= bound and err_on <= bound and err_pq <= bound
    if name == "vertices":
        assert float(dist.max()) <= 8. * EPS * scale                       # on the surface: eps scale, not sqrt(eps)


def test_brute_vs_float64():
    from selfreconcode_amd import surfdist_ops as sd
    v, f = _sphere(16)
    p = _point_sets()["shell"]
    d64, bound, _, _ = _reference("shell")
    dist, face, closest = [x.cpu().numpy() for x in sd.closest_point(_t(p), _index("sphere16", v, f, None), method="brute")]
    err = float(np.abs(dist.astype(np.float64) - d64).max())
    print(f"brute shell: |dist - d64| {err:.3g} (bound {bound:.3g})")
    assert err <= bound and float((sr.face_distance(p, v, f, face) - d64).max()) <= bound


# ------------------------------------------------------------------------------------------------------------ grid == brute
def _same_as_brute(points, index):
    from selfreconcode_amd import surfdist_ops as sd
    g = sd.closest_point(points, index)
    b = sd.closest_point(points, index, method="brute")
    u = sd.closest_point(points, index, presort=False)
    for x, y, z in zip(g, b, u):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, z.view(torch.int32) if z.dtype == torch.float32 else z)
    assert bool(torch.isfinite(g[0]).all()) and int(g[1].min()) >= 0
    return g


def test_grid_equals_brute_large():
    """65 537 shell points against the 49 152 faces of the jittered cube_sphere(64), at the default cell and at a quarter of it."""
    from selfreconcode_amd import surfdist_ops as sd
    v, f = _sphere(64)
    rng = np.random.default_rng(3)
    p = _t((_unit(rng.normal(size=(65537, 3))) * rng.uniform(0.9, 1.1, (65537, 1))).astype(np.float32))
    coarse = sd.MeshIndex.build(_t(v), _t(f))
    fine = sd.MeshIndex.build(_t(v), _t(f), coarse.cell / 4.)
    assert fine.cell == float(np.float32(coarse.cell / 4.)) and fine.nx > 3 * coarse.nx
    b = sd.closest_point(p, coarse, method="brute")
    for index in (coarse, fine):
        g = sd.closest_point(p, index)
        assert torch.equal(g[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(g[1], b[1])
        assert torch.equal(g[2].view(torch.int32), b[2].view(torch.int32))
        print(f"grid == brute on 65 537 points: grid {index.n}, cell {index.cell:.4g}, {index.pairs} pairs ({index.pairs / len(f):.2f} F)")


def test_grid_equals_brute_two_components():
    """icosphere(2) at the origin and a copy of radius 0.05 at (5, 5, 5): almost every cell is empty."""
    from selfreconcode_amd import surfdist_ops as sd
    from selfreconcode_amd.synthetic import icosphere
    v, f = [x.numpy() for x in icosphere(2)]
    v2, f2 = np.concatenate([v, 0.05 * v + 5.]).astype(np.float32), np.concatenate([f, f + len(v)])
    rng = np.random.default_rng(4)
    p = np.concatenate([rng.uniform(-1., 6., (4000, 3)), rng.uniform(-40., 40., (1000, 3)), np.float32([[5, 5, 5], [0, 0, 0], [2.5, 2.5, 2.5]])])
    for cell in (None, 0.1):
        index = sd.MeshIndex.build(_t(v2), _t(f2), cell)
        occupied = int((index.cell_start[1:] > index.cell_start[:-1]).sum())
        assert occupied < 0.2 * index.nx * index.ny * index.nz
        g = _same_as_brute(_t(p.astype(np.float32)), index)
        assert abs(float(g[0][-3]) - 0.05) < 2e-3 and int(g[1][-3]) >= len(f)


def test_pair_cap_coarsens():
    """cube_sphere(16) plus one triangle that spans the whole box: at cell 0.02 that triangle alone overlaps 10^6 cells, so the build
    doubles the cell until the pairs fit PAIR_FACTOR F instead of allocating them."""
    from selfreconcode_amd import surfdist_ops as sd
    v, f = _sphere(16)
    nv = len(v)
    vb = np.concatenate([v, np.float32([[-1.2, -1.2, -1.2], [1.2, 1.2, -1.2], [1.2, -1.2, 1.2]])])
    fb = np.concatenate([f, np.int64([[nv, nv + 1, nv + 2]])])
    index = sd.MeshIndex.build(_t(vb), _t(fb), 0.02)
    assert index.pairs <= sd.PAIR_FACTOR * len(fb) and index.cell > 0.02 and index.cell == float(np.float32(0.02)) * 2 ** round(np.log2(index.cell / 0.02))
    assert index.nx * index.ny * index.nz <= sd.MAX_CELLS
    print(f"pair cap: cell 0.02 -> {index.cell:.4g}, grid {index.n}, {index.pairs} pairs <= {sd.PAIR_FACTOR} x {len(fb)}")
    p = np.concatenate([_point_sets()["shell"], _point_sets()["centre"], _point_sets()["far"][:200]])
    _same_as_brute(_t(p), index)
    _same_as_brute(_t(p), sd.MeshIndex.build(_t(vb), _t(fb)))
    tiny = sd.MeshIndex.build(_t(v), _t(f), 1e-6)                                         # 2.4e6 cells per axis: the cell cap, before any launch
    assert tiny.nx * tiny.ny * tiny.nz <= sd.MAX_CELLS and tiny.cell == float(np.float32(1e-6)) * 2 ** round(np.log2(tiny.cell / 1e-6))
    assert tiny.pairs <= sd.PAIR_FACTOR * len(f)
    _same_as_brute(_t(_point_sets()["shell"]), tiny)


def test_grid_equals_brute_flat_single_and_degenerate():
    from selfreconcode_amd import surfdist_ops as sd
    rng = np.random.default_rng(5)
    fv, ff = mr.flat_strip(40)                                                      # all z = 0: nz = 1
    index = sd.MeshIndex.build(_t(fv), _t(ff))
    assert index.nz == 1
    g = _same_as_brute(_t((rng.uniform(-2., 42., (3001, 3)) * np.float64([1., 0.1, 0.1])).astype(np.float32)), index)
    inside = _t(np.float32([[10.25, 0.5, 0.75], [39.5, 0.25, -2.]]))
    assert torch.allclose(sd.closest_point(inside, index)[0], torch.tensor([0.75, 2.], device=DEV), rtol=0., atol=1e-6)
    one = sd.MeshIndex.build(_t(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])), _t(np.int64([[0, 1, 2]])))
    g = _same_as_brute(_t(rng.normal(size=(1000, 3)).astype(np.float32)), one)
    assert int(g[1].max()) == 0
    for cell in (0.01, 100.):
        _same_as_brute(_t(rng.normal(size=(300, 3)).astype(np.float32)), sd.MeshIndex.build(one.verts, one.faces, cell))
    # -1 rows and faces without area (a repeated vertex, three collinear points, a point) among real ones
    v, f = _sphere(16)
    nv = len(v)
    vd = np.concatenate([v, np.float32([[0.3, 0.3, 0.3], [0.5, 0.5, 0.5], [0.7, 0.7, 0.7]])])
    fd = np.concatenate([f[:50], np.int64([[3, 3, 9], [-1, -1, -1], [nv, nv + 1, nv + 2], [5, 5, 5], [-1, -1, -1]]), f[50:], np.int64([[-1, -1, -1]])])
    index = sd.MeshIndex.build(_t(vd), _t(fd))
    assert index.faces.shape[0] == len(fd) - 3 and index.tri.shape == (len(fd) - 3, 12)
    p = np.concatenate([_point_sets()["shell"], vd[-3:], 0.5 * (vd[-3:-2] + vd[-2:-1]), _point_sets()["centre"]])
    g = _same_as_brute(_t(p), index)
    clean = fd[(fd >= 0).all(1)]
    d64 = sr.closest(p, vd, clean)[0]
    assert float(np.abs(g[0].cpu().numpy() - d64).max()) <= 8. * EPS * 1.1
    assert float(g[0][1031:1035].max()) <= 8. * EPS and int(g[1][1034]) == 51       # on the collinear face, which is the segment it spans


# ------------------------------------------------------------------------------------------------------------ conventions, refusals
def test_non_finite_points_and_empty_input():
    from selfreconcode_amd import surfdist_ops as sd
    v, f = _sphere(16)
    index = _index("sphere16", v, f, None)
    p = _point_sets()["shell"][:300].copy()
    want = [x.clone() for x in sd.closest_point(_t(p), index)]
    bad = {0: (np.nan, 0, 0), 63: (0, np.inf, 0), 64: (0, 0, -np.inf), 130: (np.nan, np.nan, np.nan), 299: (np.inf, -np.inf, np.nan)}
    for i, row in bad.items():
        p[i] = row
    for method in ("grid", "brute"):
        dist, face, closest = sd.closest_point(_t(p), index, method=method)
        rows = torch.zeros(300, dtype=torch.bool, device=DEV)
        rows[list(bad)] = True
        assert bool(torch.isnan(dist[rows]).all()) and bool((face[rows] == -1).all()) and bool(torch.isnan(closest[rows]).all())
        assert torch.equal(dist[~rows], want[0][~rows]) and torch.equal(face[~rows], want[1][~rows]) and torch.equal(closest[~rows], want[2][~rows])
        dist, face, closest = sd.closest_point(torch.zeros((0, 3), device=DEV), index, method=method)
        assert dist.shape == (0,) and face.shape == (0,) and closest.shape == (0, 3) and face.dtype == torch.int64
    with pytest.raises(ValueError):
        sd.closest_point(torch.zeros((4, 2), device=DEV), index)
    with pytest.raises(ValueError):
        sd.closest_point(torch.zeros((4, 3), device=DEV), index, method="bvh")


def test_build_refusals():
    from selfreconcode_amd import surfdist_ops as sd
    v, f = _sphere(16)
    with pytest.raises(ValueError):
        sd.MeshIndex.build(_t(v), torch.zeros((0, 3), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        sd.MeshIndex.build(_t(v), _t(np.int64([[-1, -1, -1], [0, -1, 2]])))               # nothing left after cleaning
    with pytest.raises(ValueError):
        sd.MeshIndex.build(_t(v), _t(np.int64([[0, 1, len(v)]])))
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[77, 1] = bad
        with pytest.raises(ValueError):
            sd.MeshIndex.build(_t(w), _t(f))
    for cell in (0., -1., np.nan):
        with pytest.raises(ValueError):
            sd.MeshIndex.build(_t(v), _t(f), cell)
    with pytest.raises(ValueError):
        sd.sample_surface(_t(v), _t(np.int64([[5, 5, 5]])), 10, 0)                        # no area


def test_two_builds_and_two_queries_give_identical_bits():
    from selfreconcode_amd import surfdist_ops as sd
    v, f = _sphere(16)
    p = _t(_point_sets()["shell"])
    a, b = sd.MeshIndex.build(_t(v), _t(f), 0.11), sd.MeshIndex.build(_t(v), _t(f), 0.11)
    assert a.n == b.n and a.cell == b.cell and a.pairs == b.pairs
    assert torch.equal(a.cell_start, b.cell_start) and torch.equal(a.cell_faces, b.cell_faces) and torch.equal(a.lo, b.lo)
    assert int(a.cell_start[-1]) == a.pairs and a.cell_faces.dtype == torch.int32
    s = a.cell_start.cpu().numpy()
    cf = a.cell_faces.cpu().numpy()
    assert all((np.diff(cf[s[c]:s[c + 1]]) > 0).all() for c in range(len(s) - 1))         # every cell's faces ascend
    for x, y in zip(sd.closest_point(p, a), sd.closest_point(p, b)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("n", [4099, 100003])
def test_sampler_vs_restatement(n):
    from selfreconcode_amd import surfdist_ops as sd
    v, f = _sphere(16)
    f = np.concatenate([f[:100], np.int64([[7, 7, 9]]), f[100:], np.int64([[4, 4, 4]])])  # faces without area, one of them last
    cum = sd.face_areas_cum(_t(v), _t(f))
    assert cum.dtype == torch.float64 and cum.shape == (len(f),)
    cum_h = cum.cpu().numpy()
    assert np.abs(cum_h - sr.face_areas_cum(v, f)).max() < 1e-12
    pts, face, nrm = [x.cpu().numpy() for x in sd.sample_surface(_t(v), _t(f), n, 11, cum_area=cum)]
    rp, rf, rn = sr.sample(cum_h, v, f, n, 11)
    assert pts.dtype == np.float32 and face.dtype == np.int64 and nrm.dtype == np.float32
    assert np.array_equal(face, rf)
    scale = float(np.abs(v).max())
    err = float(np.abs(pts - rp).max())
    print(f"sampler n {n}: max point error {err:.3g} (bound {4 * EPS * scale:.3g})")
    assert err <= 4. * EPS * scale
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.).max() < 1e-6
    assert np.abs(nrm - sr.face_normals(v, f)[face]).max() < 1e-6 and np.abs(nrm - rn).max() < 1e-6
    area = np.diff(cum_h, prepend=0.)
    dev = float(np.abs(np.bincount(face, minlength=len(f)) - n * area / cum_h[-1]).max())
    print(f"sampler n {n}: max |count - n a / A| {dev:.3f}")
    assert dev < 2. and not np.isin(face, [100, len(f) - 1]).any()
    again = sd.sample_surface(_t(v), _t(f), n, 11)
    assert np.array_equal(again[0].cpu().numpy(), pts) and np.array_equal(again[1].cpu().numpy(), face)
    assert not np.array_equal(sd.sample_surface(_t(v), _t(f), n, 12)[0].cpu().numpy(), pts)


# ------------------------------------------------------------------------------------------------------------ metrics, command
def _pair32():
    v, f = _sphere(32, jittered=False)
    return (v, f), ((v * np.float32(1.05)).astype(np.float32), f)


def test_surface_metrics_vs_restatement_and_closed_form():
    from selfreconcode_amd import surfdist_ops as sd
    from selfreconcode_amd.evaluate import surface_metrics, vertex_to_surface
    pred, gt = _pair32()
    n, seed, taus = 20011, 3, (0.04, 0.0505, 0.06)
    dp, dg = (_t(pred[0]), _t(pred[1])), (_t(gt[0]), _t(gt[1]))
    got = surface_metrics(dp, dg, samples=n, seed=seed, taus=taus)
    assert got == surface_metrics(dp, dg, samples=n, seed=seed, taus=taus)                # identical numbers
    assert all(isinstance(x, float) for x in (got["chamfer"], got["p2s"], got["normal_consistency"], got["pred_to_gt"]["rms"]))
    sp = [x.cpu().numpy() for x in sd.sample_surface(*dp, n, seed)]
    sg = [x.cpu().numpy() for x in sd.sample_surface(*dg, n, seed + 1)]
    ref = sr.metrics(pred, gt, (sp[0], sp[2]), (sg[0], sg[2]), taus)
    bound = 8. * EPS * 1.05
    for d in ("pred_to_gt", "gt_to_pred"):
        for k in ("mean", "rms", "max"):
            print(f"surface_metrics {d} {k}: {got[d][k]:.9g} vs {ref[d][k]:.9g} (bound {bound:.3g})")
            assert abs(got[d][k] - ref[d][k]) <= bound
    assert abs(got["chamfer"] - ref["chamfer"]) <= bound and abs(got["p2s"] - ref["p2s"]) <= bound and got["p2s"] == got["gt_to_pred"]["mean"]
    assert got["chamfer"] == 0.5 * (got["pred_to_gt"]["mean"] + got["gt_to_pred"]["mean"])
    print(f"normal consistency {got['normal_consistency']:.9g} vs {ref['normal_consistency']:.9g}")
    assert abs(got["normal_consistency"] - ref["normal_consistency"]) <= 1e-5 and got["normal_consistency"] > 0.99
    assert got["fscore@0.04"] == 0. and got["fscore@0.06"] == 1. and 0. <= got["fscore@0.0505"] <= 1.
    # closed form: both meshes are inscribed in their spheres, a face lies no deeper than R - sqrt(R^2 - L^2 / 3) below (|sum w_i v_i|^2
    # = R^2 - sum_{i<j} w_i w_j |v_i - v_j|^2 >= R^2 - L^2 / 3), L the longest edge
    edge = max(float(np.linalg.norm(m[0][m[1]] - m[0][np.roll(m[1], 1, 1)], axis=2).max()) for m in (pred, gt))
    s = 2. * (1.05 - (1.05 ** 2 - edge ** 2 / 3.) ** 0.5) + 1e-6
    print(f"directed means {got['pred_to_gt']['mean']:.6f} / {got['gt_to_pred']['mean']:.6f} in 0.05 +- {s:.3g}")
    for d in ("pred_to_gt", "gt_to_pred"):
        assert 0.05 - s <= got[d]["mean"] <= 0.05 + s and got[d]["max"] <= 0.05 + s + 0.5 * edge
    d = vertex_to_surface(dg[0], dp).cpu().numpy()
    assert d.shape == (len(gt[0]),) and np.abs(d - 0.05).max() <= s + 0.5 * edge


def test_command_mesh_pair_mode(tmp_path):
    from selfreconcode_amd import evaluate
    from selfreconcode_amd.mesh_io import write_ply
    from selfreconcode_amd.synthetic import icosphere
    v, f = [x.numpy() for x in icosphere(2)]
    a, b, out = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "m.json")
    write_ply(a, v, f)
    write_ply(b, v * 1.1 + 0.01, f)
    lines = []
    got = evaluate.main(["--gpu-ids", "0", "--pred", a, "--gt", b, "--samples", "5003", "--seed", "2", "--tau", "0.05", "0.2", "--out", out],
                        out=lines.append)
    assert len(lines) == 1 and json.loads(lines[0]) == got == json.load(open(out))
    direct = evaluate.surface_metrics((_t(v), _t(f)), (_t((v * 1.1 + 0.01).astype(np.float32)), _t(f)), 5003, 2, (0.05, 0.2))
    assert direct == got and 0.05 < got["chamfer"] < 0.15 and got["fscore@0.2"] == 1. and "fscore@0.05" in got


def test_command_folder_mode(tmp_path):
    from selfreconcode_amd import evaluate
    from selfreconcode_amd.mesh_io import write_ply
    from selfreconcode_amd.synthetic import icosphere
    v, f = [x.numpy() for x in icosphere(2)]
    rec, gt = tmp_path / "result", tmp_path / "gt"
    os.makedirs(rec / "meshs")
    os.makedirs(gt)
    write_ply(str(rec / "tmp.ply"), v, f)
    for fid, scale in ((0, 1.), (7, 1.02), (12, 1.04)):
        np.save(str(rec / "meshs" / ("%d.npy" % fid)), (v * scale).astype(np.float32))
    write_ply(str(gt / "0.ply"), v * 1.05, f)
    with open(gt / "12.obj", "w") as fh:
        fh.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in (v * 1.05).tolist())
        fh.writelines("f %d/1/1 %d/1/1 %d/1/1\n" % tuple(t) for t in (f + 1).tolist())
    lines = []
    got = evaluate.main(["--rec-root", str(rec), "--gt-root", str(gt), "--samples", "3001"], out=lines.append)
    assert list(got["frames"]) == ["0", "12"] and got["skipped"] == ["7"]
    assert any("2 frames compared, 1 skipped" in x for x in lines)
    assert got["frames"]["0"]["chamfer"] > got["frames"]["12"]["chamfer"] > 0.
    assert abs(got["frames"]["0"]["p2s"] - 0.05) < 0.01 and abs(got["frames"]["12"]["p2s"] - 0.01) < 0.005
    assert json.load(open(rec / "geometry_errors.json")) == got
    txt = open(rec / "geometry_errors.txt").read().splitlines()
    assert len(txt) == 5 and txt[1].startswith("   0: ") and txt[2].startswith("  12: ")
    assert txt[3].startswith("chamfer mean: ") and txt[3].rstrip().endswith("maxinds:0 1") and txt[4].startswith("p2s mean: ")
    assert "%.6f" % got["frames"]["12"]["chamfer"] in txt[2]
    lines = []
    one = evaluate.main(["--rec-root", str(rec), "--gt-root", str(gt), "--samples", "3001", "--frames", "2"], out=lines.append)
    assert list(one["frames"]) == ["0"] and one["skipped"] == ["7"]
