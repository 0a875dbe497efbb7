"""Quadric-optimal vertex placement of the template simplification on the GPU (csrc/mesh_prep.hip: sr_meshprep_cell_faces,
sr_meshprep_cell_quadric, sr_meshprep_face_flips; mesh_prep_ops; mesh_prep placement="quadric") against the float64 restatement of
tests/_meshquadric_ref.py.  Shapes: the UV sphere 64 x 32 and the cube of 12 x 12 quads per side, plain and jittered by 0.002, at cells
0.61, 0.43 and 0.31, plus flat grids whose answer is known in closed form (one of 800 x 800, the smallest that takes the face and the
cell kernels beyond one pass of the launch grid).

Position tolerance: the product rounds its double result to float32 once, so it may differ from the restatement by 2^-24 of the
coordinate; the bound is twice that, 2^-23 max |restated coordinate|.  The solve's own error, about (3 / reg) 2^-53, and the order of the
sums (the kernel adds 16 interleaved partial sums, the restatement adds in face order) are far below it."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import _meshprep_ref as mr
import _meshquadric_ref as mq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(name, cell) for name in mq.SHAPES for cell in mq.CELLS]
_CACHE = {}


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _bound(ref):
    return 2. ** -23 * float(np.abs(ref["verts"]).max())


def _case(name, cell):
    """One shape at one cell: the restatement, and the product's mesh and report for both placements (computed once, never changed)."""
    from selfreconcode_amd.mesh_prep import simplify_mesh
    if (name, cell) not in _CACHE:
        v, f = mq.shape(name)
        tv, tf = _t(v), _t(f)
        rq, rm = {}, {}
        quad = simplify_mesh(tv, tf, cell, placement="quadric", report=rq)
        mean = simplify_mesh(tv, tf, cell, placement="mean", report=rm)
        _CACHE[(name, cell)] = dict(v=v, f=f, tv=tv, tf=tf, ref=mq.simplify_quadric(v, f, cell), quad=quad, mean=mean, rq=rq, rm=rm)
    return _CACHE[(name, cell)]


def _optima(tv, tf, cell, reg=1e-3):
    """mesh_prep_ops.cell_quadric_optima on the grid simplify_mesh would make -> (positions, flags, shift, vertex_map)."""
    from selfreconcode_amd import mesh_prep_ops as mp
    lo, hi = mp.mesh_bounds(tv)
    n = mp.grid_shape(lo.cpu().numpy(), hi.cpu().numpy(), cell)
    cells, vmap = mp.cluster(mp.cell_keys(tv, lo, cell, n))
    return mp.cell_quadric_optima(tv, tf, vmap, cells, lo, cell, n, reg) + (vmap,)


@pytest.mark.parametrize("name, cell", CASES)
def test_quadric_vs_restatement(name, cell):
    """Per-cell flags are compared outside the cells whose restated optimum lies within 1e-9 cell of a wall of its box, and at most 1 %
    of the cells may be left out -- except on the plain cube, where nothing is left out: its low faces lie on the grid's low walls, so
    the optimum of a cell inside such a face is exactly on the wall, and it is so on both sides (every normal there is an exact axis, b -
    A m is exactly zero and the vertex stays at its mean, whose coordinate is the wall's)."""
    from selfreconcode_amd import mesh_prep_ops as mp
    c = _case(name, cell)
    ref, quad, mean, rq = c["ref"], c["quad"], c["mean"], c["rq"]
    assert quad.verts.dtype == torch.float32 and quad.cell == mean.cell == float(np.float32(cell))
    assert torch.equal(quad.faces, mean.faces) and torch.equal(quad.vertex_map, mean.vertex_map)
    assert np.array_equal(quad.faces.cpu().numpy(), ref["faces"]) and np.array_equal(quad.vertex_map.cpu().numpy(), ref["vertex_map"])
    C = len(ref["verts"])
    got = quad.verts.cpu().numpy().astype(np.float64)
    err, bound = float(np.abs(got - ref["verts"]).max()), _bound(ref)
    print(f"{name} cell {cell}: {C} cells, {len(ref['faces'])} faces, clamped {rq['clamped']} (restated {int(ref['clamped'].sum())}), no_planes {rq['no_planes']} "
          f"({int(ref['no_planes'].sum())}), near a wall {int(ref['near_wall'].sum())}, max_shift {rq['max_shift']:.4f} ({ref['max_shift']:.4f}), flipped {rq['flipped']}, "
          f"max position error {err:.3g} (bound {bound:.3g})")
    assert rq["placement"] == "quadric" and rq["cells"] == C == quad.verts.shape[0]
    assert rq["clamped"] == int(ref["clamped"].sum()) and rq["no_planes"] == int(ref["no_planes"].sum())
    assert err <= bound
    assert rq["max_shift"] == pytest.approx(ref["max_shift"], rel=1e-5)
    assert (rq["flipped"], rq["zero_area"]) == mq.face_flips(c["v"], c["f"], quad.verts.cpu().numpy(), ref["faces"], ref["source"])
    # the operator on its own: the same positions, and the flags cell by cell
    pos, flags, shift, vmap = _optima(c["tv"], c["tf"], cell)
    assert torch.equal(pos, quad.verts) and torch.equal(vmap, quad.vertex_map) and flags.dtype == torch.int32 and shift.dtype == torch.float32
    flags = flags.cpu().numpy()
    left_out = np.zeros(C, bool) if name == "cube" else ref["near_wall"]
    assert left_out.sum() <= 0.01 * C
    assert np.array_equal((flags & mp.QUADRIC_CLAMPED != 0)[~left_out], ref["clamped"][~left_out])
    assert np.array_equal((flags & mp.QUADRIC_NO_PLANES != 0)[~left_out], ref["no_planes"][~left_out])
    assert not (flags & ~3).any()
    assert float(shift.max()) == rq["max_shift"]


@pytest.mark.parametrize("cell", [0.61, 0.43])
def test_the_clamp_is_live(cell):
    """The restatement clamps 3 of 48 and 5 of 87 cells of the sphere there (6.2 % and 5.7 %)."""
    c = _case("sphere", cell)
    assert int(c["ref"]["clamped"].sum()) > 0 and c["rq"]["clamped"] > 0 and c["rm"]["clamped"] == 0


@pytest.mark.parametrize("name, cell", CASES)
def test_quality_against_the_mean_placement(name, cell):
    """Each figure of placement="quadric" against placement="mean" on the same clustering; the errors are measured on 20 000
    surfdist_ops.sample_surface samples of each simplified mesh.  What the restatement alone gives (numpy samples, cells 0.61 / 0.43 /
    0.31; tests/test_meshquadric_cpu.py asserts these conditions on it):

        sphere, mean | |s| - 1 |, quadric / mean           0.347 / 0.310 / 0.280   (jittered 0.345 / 0.311 / 0.290)     condition <= 0.5
        sphere, |1 - volume / (4 pi / 3)|, quadric / mean  0.331 / 0.274 / 0.235   (jittered 0.293 / 0.275 / 0.238)     condition <= 0.5
           (volume deficits: mean 23 % / 12 % / 6.1 %, quadric 7.6 % / 3.3 % / 1.4 %)
        plain cube, largest vertex distance, quadric / mean  0.0010 / 0.0010 / 0.0010  (1.9e-4 against 0.19 at 0.61)    condition <= 0.01
        jittered cube, mean sample distance, quadric / mean  0.013 / 0.020 / 0.102                                      condition <= 0.2
        flipped surviving faces: equal under both placements (0; 1 on the jittered sphere at 0.61); zero-area faces: 0."""
    from selfreconcode_amd.surfdist_ops import sample_surface
    c = _case(name, cell)
    fig = {}
    for placement in ("quad", "mean"):
        m = c[placement]
        pts = sample_surface(m.verts, m.faces, 20000, 1)[0].cpu().numpy()
        fig[placement] = mq.quality(name, m.verts.cpu().numpy(), m.faces.cpu().numpy(), pts)
    q, m = fig["quad"], fig["mean"]
    print(f"{name} cell {cell}: surface {q['surface']:.4g} / {m['surface']:.4g} = {q['surface'] / m['surface']:.4f}, volume {q['volume']:.4g} / {m['volume']:.4g} = "
          f"{q['volume'] / m['volume']:.4f}, vertex {q['vertex']:.4g} / {m['vertex']:.4g}, flipped {c['rq']['flipped']} / {c['rm']['flipped']}, "
          f"zero_area {c['rq']['zero_area']} / {c['rm']['zero_area']}")
    if name.startswith("sphere"):
        assert q["surface"] <= 0.5 * m["surface"]
        assert q["volume"] <= 0.5 * m["volume"]
    elif name == "cube":
        assert q["vertex"] <= 0.01 * m["vertex"]
    else:
        assert q["surface"] <= 0.2 * m["surface"]
    assert c["rq"]["flipped"] <= c["rm"]["flipped"]
    assert c["rq"]["zero_area"] == 0 and c["rm"]["zero_area"] == 0
    assert c["rm"]["placement"] == "mean" and c["rm"]["no_planes"] == 0 and c["rm"]["max_shift"] == 0.


@pytest.mark.parametrize("z", [0., 0.25])
@pytest.mark.parametrize("cell", [2.5, 3.0, 7.3])
def test_flat_grid_stays_at_the_cell_means(cell, z):
    """The planes fix only the normal component, which the mean has already: the regulariser keeps the tangential ones."""
    from selfreconcode_amd.mesh_prep import simplify_mesh
    v, f = mq.flat_grid(40, z)
    rep = {}
    got = simplify_mesh(_t(v), _t(f), cell, placement="quadric", report=rep)
    ref = mr.simplify(v, f, cell)
    assert np.array_equal(got.faces.cpu().numpy(), ref["faces"])
    err = float(np.abs(got.verts.cpu().numpy().astype(np.float64) - ref["verts"]).max())
    assert err <= 2. ** -23 * float(np.abs(ref["verts"]).max())
    assert (got.verts[:, 2] == z).all()
    assert rep["clamped"] == rep["no_planes"] == rep["flipped"] == rep["zero_area"] == 0 and rep["max_shift"] <= 1e-12


def test_one_vertex_per_cell_returns_the_input_bits():
    from selfreconcode_amd.mesh_prep import simplify_mesh
    v, f = mq.flat_grid(40)
    rep = {}
    got = simplify_mesh(_t(v), _t(f), 0.75, placement="quadric", report=rep)               # floor(i / 0.75) is a different cell for every i
    assert got.vertex_map.tolist() == list(range(1600))
    assert np.array_equal(got.verts.cpu().numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(got.faces.cpu().numpy(), f)
    assert rep == dict(placement="quadric", cells=1600, clamped=0, no_planes=0, flipped=0, zero_area=0, max_shift=0.)


def test_beyond_one_launch_pass():
    """800 x 800 vertices, each its own cell: 640 000 cells x 16 lanes and 1 276 802 faces both exceed the 2048 x 256 threads of one
    pass of the launch grid.  On z = 0 every b - A m is exactly zero, so the output is the input, bit for bit."""
    from selfreconcode_amd.mesh_prep import simplify_mesh
    v, f = mq.flat_grid(800)
    assert len(v) == 640000 and len(f) == 1276802 and min(len(v), len(f)) > 2048 * 256
    tv, tf = _t(v), _t(f)
    rep = {}
    got = simplify_mesh(tv, tf, 1.0, placement="quadric", report=rep)
    assert torch.equal(got.vertex_map, torch.arange(640000, device=DEV))
    assert torch.equal(got.verts.view(torch.int32), tv.view(torch.int32)) and torch.equal(got.faces, tf)
    assert rep == dict(placement="quadric", cells=640000, clamped=0, no_planes=0, flipped=0, zero_area=0, max_shift=0.)


def _vs_ref(v, f, cell, reg=1e-3):
    """simplify_mesh(quadric) against the restatement on a small mesh made so that no optimum the planes place lies within 1e-9 cell of
    a wall: positions to the bound, flags and counts equal -> (mesh, report, ref)."""
    from selfreconcode_amd import mesh_prep_ops as mp
    from selfreconcode_amd.mesh_prep import simplify_mesh
    rep = {}
    got = simplify_mesh(_t(v), _t(f), cell, placement="quadric", reg=reg, report=rep)
    ref = mq.simplify_quadric(v, f, cell, reg)
    assert not (ref["near_wall"] & ~ref["no_planes"]).any()                                  # (a cell without planes sits at its mean exactly, on both sides)
    assert np.array_equal(got.faces.cpu().numpy(), ref["faces"]) and np.array_equal(got.vertex_map.cpu().numpy(), ref["vertex_map"])
    assert float(np.abs(got.verts.cpu().numpy().astype(np.float64) - ref["verts"]).max()) <= _bound(ref)
    flags = _optima(_t(v), _t(mq.clean(f)), cell, reg)[1].cpu().numpy()
    assert np.array_equal(flags & mp.QUADRIC_CLAMPED != 0, ref["clamped"]) and np.array_equal(flags & mp.QUADRIC_NO_PLANES != 0, ref["no_planes"])
    assert rep["clamped"] == int(ref["clamped"].sum()) and rep["no_planes"] == int(ref["no_planes"].sum())
    return got, rep, ref


def test_edge_cases():
    from selfreconcode_amd.mesh_prep import simplify_mesh
    # one cell takes the whole mesh: no face survives, and the one vertex is placed by every face that has area
    v, f = mq.cube(3)
    f = f[v[f][:, :, 0].min(1) < 1.]                                                        # (without the side x = 1: the side x = -1 pulls the vertex over)
    v = mr.jitter(v, 2, 0.01)
    got, rep, ref = _vs_ref(v, f, 50.)
    assert got.verts.shape == (1, 3) and got.faces.shape == (0, 3) and rep["no_planes"] == 0 and rep["flipped"] == rep["zero_area"] == 0
    assert ref["mean"][0, 0] - ref["verts"][0, 0] > 0.5 and rep["max_shift"] == pytest.approx(ref["max_shift"], rel=1e-5)
    # a cell whose faces have no area (5), vertices no face references (cells 0 and 3), next to a proper triangle: they stay at the mean.
    # (Vertex 7 makes the low corner of the box, so that the triangle's one-vertex cells, whose optimum is their vertex, hold it inside.)
    v = np.float32([[0.2, 0.3, 0.1], [1.2, 0.3, 0.2], [0.2, 1.3, 0.3], [5, 5, 5], [5.1, 5.1, 5.1], [5.2, 5.2, 5.2], [9, 0.3, 0.1], [-1, -1, -1]])
    f = np.int64([[0, 1, 2], [3, 4, 5], [-1, -1, -1], [3, 3, 4]])
    got, rep, ref = _vs_ref(v, f, 0.5)
    assert ref["vertex_map"].tolist() == [1, 2, 4, 5, 5, 5, 3, 0] and ref["no_planes"].tolist() == [True, False, False, True, False, True]
    assert rep["no_planes"] == 3 and rep["clamped"] == 0 and np.array_equal(got.verts[5].cpu().numpy(), np.float32(ref["mean"][5]))
    assert got.verts[3].tolist() == v[6].tolist() and got.verts[0].tolist() == [-1., -1., -1.]
    # six faces by hand; 0.5-cells: vertices 0, 1 share one, 2, 3, 6 another, 4 and 5 are alone.  Face 0 has two corners in one cell,
    # face 3 all three; each feeds a cell once, and the faces that die in the clustering (0, 3, 4, 5) still feed
    v = np.float32([[0.1, 0.1, 0.], [0.3, 0.2, 0.1], [1.1, 0.1, 0.3], [1.3, 0.3, 0.], [0.2, 1.2, 0.4], [1.2, 1.3, 0.9], [1.2, 0.2, 0.2]])
    f = np.int64([[0, 1, 2], [0, 2, 4], [2, 5, 4], [2, 3, 6], [1, 3, 4], [0, 3, 1]])
    got, rep, ref = _vs_ref(v, f, 0.5)
    assert ref["vertex_map"].tolist() == [0, 0, 1, 1, 2, 3, 1] and ref["faces"].tolist() == [[0, 1, 2], [1, 3, 2]] and rep["no_planes"] == 0
    for extra in (0, 3):                                                                    # feeding face 0 or 3 a second time would change the answer
        twice = mq.simplify_quadric(v, np.concatenate([f, f[extra:extra + 1]]), 0.5)
        assert float(np.abs(twice["verts"] - ref["verts"]).max()) > 100 * _bound(ref)
    # rows with a negative index are ignored, by the operator itself too
    g = np.concatenate([f[:2], [[-1, -1, -1]], f[2:], [[4, -1, 2]]])
    a = _optima(_t(v), _t(f), 0.5)
    b = _optima(_t(v), _t(g), 0.5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(simplify_mesh(_t(v), _t(g), 0.5, placement="quadric").verts, a[0])
    # a NaN vertex is refused as with the mean placement
    w = v.copy(); w[2, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        simplify_mesh(_t(w), _t(f), 0.5, placement="quadric")
    with pytest.raises(RuntimeError):
        simplify_mesh(torch.from_numpy(v), torch.from_numpy(f), 0.5, placement="quadric")   # no CPU fallback


def test_two_calls_give_identical_bits():
    from selfreconcode_amd.mesh_prep import simplify_mesh
    c = _case("sphere_jitter", 0.31)
    rep = {}
    again = simplify_mesh(c["tv"], c["tf"], 0.31, placement="quadric", report=rep)
    assert torch.equal(again.verts.view(torch.int32), c["quad"].verts.view(torch.int32)) and torch.equal(again.faces, c["quad"].faces)
    assert rep == c["rq"]
    a, b = _optima(c["tv"], c["tf"], 0.31), _optima(c["tv"], c["tf"], 0.31)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_simplify_to_and_the_default():
    from selfreconcode_amd.mesh_prep import simplify_mesh, simplify_to
    from selfreconcode_amd.mesh_prep_ops import cell_means
    v, f = mq.shape("sphere_jitter")
    tv, tf = _t(v), _t(f)
    pm, pq, rq = [], [], {}
    mean = simplify_to(tv, tf, 400, probes=pm)
    quad = simplify_to(tv, tf, 400, probes=pq, placement="quadric", report=rq)
    assert mean.cell == quad.cell > 0 and pm == pq and len(pm) == 17
    assert torch.equal(mean.faces, quad.faces) and torch.equal(mean.vertex_map, quad.vertex_map) and 0 < quad.faces.shape[0] <= 400
    assert not torch.equal(mean.verts, quad.verts) and rq["placement"] == "quadric" and rq["cells"] == quad.verts.shape[0] and rq["max_shift"] > 0
    direct = simplify_mesh(tv, tf, quad.cell, placement="quadric")
    assert torch.equal(direct.verts, quad.verts)
    plain, named = simplify_mesh(tv, tf, mean.cell), simplify_mesh(tv, tf, mean.cell, placement="mean", reg=0.5)
    for a, b in ((plain, named), (plain, mean)):
        assert torch.equal(a.verts.view(torch.int32), b.verts.view(torch.int32)) and torch.equal(a.faces, b.faces) and torch.equal(a.vertex_map, b.vertex_map)
    assert torch.equal(plain.verts, cell_means(tv, plain.vertex_map, plain.verts.shape[0]))
    rep = {}
    same = simplify_to(tv, tf, len(f), placement="quadric", report=rep)                     # within the budget: nothing moves
    assert same.cell == 0. and torch.equal(same.verts, tv) and rep == dict(placement="quadric", cells=len(v), clamped=0, no_planes=0, flipped=0, zero_area=0, max_shift=0.)


def test_prepare_template_quadric_into_export_texture(tmp_path):
    import _texture_ref as tr
    from selfreconcode_amd.mesh_io import read_obj_uv
    from selfreconcode_amd.mesh_prep import prepare_template, simplify_quality
    from selfreconcode_amd.posed import FULL_RATIO
    from selfreconcode_amd.synthetic import build_synthetic_scene
    from selfreconcode_amd.texture import export_texture, texture_frames
    H = W = 96
    R = 256
    torch.manual_seed(0)
    net, ds, _ = build_synthetic_scene(device=DEV, frame_num=40, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)], lbs_volume_shape=(17, 57, 33),
                                       consistent_masks=False)
    fids = texture_frames(ds.frame_num, 6)
    views = [(int(f), tr.smooth_image(H, W, 0.3 * k), ds.batch(torch.tensor([int(f)], device=DEV))['mask'][0] > 0.5) for k, f in enumerate(fids)]
    TmpVs, Tmpfs = net.discretizeSDF(FULL_RATIO, None, 0.)
    quality, preps = {}, {}
    for placement in ("mean", "quadric"):
        root, rep = str(tmp_path / placement), {}
        prep = preps[placement] = prepare_template(net, root, target_faces=600, resolution=R, TmpVs=TmpVs, Tmpfs=Tmpfs, placement=placement, report=rep)
        assert rep["placement"] == placement and rep["cells"] == prep.mesh.verts.shape[0] and rep["zero_area"] == 0
        v, f, vt, ft = read_obj_uv(prep.obj_path)
        assert np.array_equal(v, prep.mesh.verts.cpu().numpy()) and np.array_equal(f, prep.mesh.faces.cpu().numpy())
        quality[placement] = simplify_quality(prep.mesh, TmpVs.detach(), Tmpfs, samples=20000)
    q, m = quality["quadric"], quality["mean"]
    print(f"template {TmpVs.shape[0]} -> {preps['quadric'].mesh.verts.shape[0]} vertices: volume ratio quadric {q['volume_ratio']:.5f}, mean {m['volume_ratio']:.5f}; "
          f"source -> simplified mean distance {q['source_to_simplified']['mean']:.4g}, {m['source_to_simplified']['mean']:.4g}")
    assert torch.equal(preps["mean"].mesh.faces, preps["quadric"].mesh.faces) and preps["mean"].mesh.cell == preps["quadric"].mesh.cell
    for d in (q, m):
        flat = [d["chamfer"], d["volume_source"], d["volume_simplified"], d["volume_ratio"]] + [d[k][s] for k in ("simplified_to_source", "source_to_simplified")
                                                                                                  for s in ("mean", "rms", "max")]
        assert np.isfinite(flat).all() and d["volume_source"] > 0
    assert abs(1. - q["volume_ratio"]) < abs(1. - m["volume_ratio"])
    prep = preps["quadric"]
    baked = export_texture(net, prep.obj_path, views, os.path.join(str(tmp_path / "quadric"), "template"), resolution=R, check_num=2)
    assert baked.tex_mask.any() and baked.mask_final.any() and not (baked.mask_final & ~baked.tex_mask).any()
    assert (baked.texture[baked.tex_mask] > 0).any(-1).all()
    with pytest.raises(ValueError, match="placement"):
        prepare_template(net, str(tmp_path / "bad"), TmpVs=TmpVs, Tmpfs=Tmpfs, placement="median")
    assert not os.path.exists(str(tmp_path / "bad"))


def test_quadric_abi_argument_checks():
    """The three new entry points refuse a null pointer, a zero or negative count and a value outside its domain with SR_EINVAL,
    before anything is launched."""
    from selfreconcode_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    P = _lib.ptr
    i32, i64 = torch.int32, torch.int64
    v = _t(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])); f = _t(np.int64([[0, 1, 2], [1, 3, 2]]))
    V, F, C = 4, 2, 1
    vmap = torch.zeros(V, dtype=i64, device=DEV); slot = torch.zeros(3 * F, dtype=i64, device=DEV)
    slots = torch.arange(3 * F, device=DEV); foff = _t(np.int64([0, 3 * F])); order = torch.arange(V, device=DEV); offs = _t(np.int64([0, V]))
    cells = torch.zeros(C, dtype=i64, device=DEV); lo = torch.zeros(3, device=DEV)
    out = torch.zeros(C, 3, device=DEV); flags = torch.zeros(C, dtype=i32, device=DEV); shift = torch.zeros(C, device=DEV)
    nv = v[:3].clone(); nf = _t(np.int64([[0, 1, 2]])); src = torch.zeros(1, dtype=i64, device=DEV); counts = torch.zeros(2, dtype=i64, device=DEV)
    calls = {
        "sr_meshprep_cell_faces": dict(f=P(f), F=F, m=P(vmap), V=V, C=C, slot=P(slot)),
        "sr_meshprep_cell_quadric": dict(a=P(v), V=V, f=P(f), F=F, fs=P(slots), fo=P(foff), o=P(order), off=P(offs), cells=P(cells), C=C, lo=P(lo), cell=2., nx=1, ny=1,
                                         reg=1e-3, out=P(out), flags=P(flags), shift=P(shift)),
        "sr_meshprep_face_flips": dict(a=P(v), V=V, f=P(f), F=F, nv=P(nv), Vn=3, nf=P(nf), src=P(src), Fn=1, counts=P(counts)),
    }
    extra = {"sr_meshprep_cell_faces": [dict(F=-1), dict(V=-1), dict(C=-1)],
             "sr_meshprep_cell_quadric": [dict(V=-1), dict(F=-1), dict(C=-1), dict(cell=-1.), dict(cell=float("nan")), dict(nx=-1), dict(ny=-1), dict(reg=-1e-3),
                                          dict(reg=float("nan")), dict(reg=float("inf")), dict(nx=1 << 31, ny=1 << 31)],
             "sr_meshprep_face_flips": [dict(V=-1), dict(F=-1), dict(Vn=-1), dict(Fn=-1)]}
    n = 0
    for name, args in calls.items():
        _lib.call(name, *args.values(), s)                                                           # the arguments as they are: accepted
        torch.cuda.synchronize()
        for change in [{k: 0} for k in args] + extra[name]:
            with pytest.raises(_lib.SrError, match="SR_EINVAL"):
                _lib.call(name, *{**args, **change}.values(), s)
                pytest.fail(f"{name} accepted {change}")
            n += 1
    torch.cuda.synchronize()
    assert n == 6 + 18 + 10 + 3 + 11 + 4
    assert slot.tolist() == [0, 1, 1, 0, 1, 1] and counts.tolist() == [0, 0] and out.isfinite().all() and int(flags) in (0, 1, 2, 3)   # (C = 1 is the empty slot here)


def test_texture_command_with_quadric_placement_and_report(tmp_path_factory):
    """`python -m selfreconcode_amd.texture --placement quadric --simplify-report` end to end on a copy of the folder a training run left
    (tests/_train_scene.py; the session's shared result folder is only read): the usual files plus template/simplify.json, one line."""
    import _train_scene as ts
    from selfreconcode_amd import texture
    from test_texture_cli_gpu import ARGS, WRITTEN
    capture, first = ts.folder(tmp_path_factory)
    rec_root = os.path.join(os.path.dirname(first.save_root), os.path.basename(first.save_root) + '_quadric')
    assert not os.path.exists(rec_root)
    shutil.copytree(first.save_root, rec_root, ignore=shutil.ignore_patterns('template', 'textured', 'turntable'))
    said = []
    assert texture.main(ARGS + ['--rec-root', rec_root, '--placement', 'quadric', '--simplify-report'],
                        out=lambda *a, **k: said.append(' '.join(str(x) for x in a)), resolutions=ts.PYRAMID) == 0
    folder = os.path.join(rec_root, 'template')
    assert sorted(os.listdir(folder)) == sorted(WRITTEN + ['simplify.json'])
    lines = [x for x in said if x.startswith('simplify:')]
    assert len(lines) == 1 and 'placement quadric' in lines[0] and 'simplify.json' in lines[0]
    with open(os.path.join(folder, 'simplify.json')) as fh:
        rep = json.load(fh)
    assert rep['placement'] == 'quadric' and rep['cells'] > 0 and rep['cell'] > 0 and rep['zero_area'] == 0 and rep['max_shift'] > 0
    assert set(rep) == {'placement', 'cells', 'clamped', 'no_planes', 'flipped', 'zero_area', 'max_shift', 'cell', 'quality'}
    assert np.isfinite(rep['quality']['volume_ratio']) and np.isfinite(rep['quality']['source_to_simplified']['mean'])
    assert sum(x.startswith('template:') for x in said) == 1 and sum('wrote' in x and 'uvmap.obj' in x for x in said) == 1
