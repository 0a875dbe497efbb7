"""Template preparation on the GPU (csrc/mesh_prep.hip, mesh_prep_ops, mesh_prep) against the float64 restatement of
tests/_meshprep_ref.py: vertex-clustering simplification, box-projection charts, the contested-texel count, and prepare_template into
export_texture.  The sizes are the smallest that reach each loop bound (a cell of 322 members, a 40 000-face strip for the component
search); nothing here is a full-size template."""
import os

import numpy as np
import pytest
import torch

import _meshprep_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELLS = (0.05, 0.11, 0.7, 3.0)
_CACHE = {}


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _sphere32(jittered):
    """cube_sphere(32): 6146 vertices (not a multiple of a 256-thread block) / 12 288 faces, plain or with a seeded jitter."""
    from selfreconcode_amd.synthetic import cube_sphere
    if jittered not in _CACHE:
        v, f = [x.numpy() for x in cube_sphere(32)]
        _CACHE[jittered] = (mr.jitter(v, 5, 0.004) if jittered else v, f)
    return _CACHE[jittered]


@pytest.mark.parametrize("jittered", [False, True])
@pytest.mark.parametrize("cell", CELLS)
def test_simplify_vs_restatement(cell, jittered):
    from selfreconcode_amd.mesh_prep import simplify_mesh
    v, f = _sphere32(jittered)
    assert len(v) == 6146 and len(v) % 256 and len(f) == 12288
    ref = mr.simplify(v, f, cell)
    got = simplify_mesh(_t(v), _t(f), cell)
    assert got.verts.dtype == torch.float32 and got.faces.dtype == torch.int64 and got.vertex_map.dtype == torch.int64
    assert got.cell == float(np.float32(cell))
    assert np.array_equal(got.vertex_map.cpu().numpy(), ref["vertex_map"]) and np.array_equal(got.faces.cpu().numpy(), ref["faces"])
    err = float(np.abs(got.verts.cpu().numpy().astype(np.float64) - ref["verts"]).max())
    bound = mr.position_bound(ref, v)
    print(f"simplify cell {cell} jitter {jittered}: {len(ref['verts'])} vertices, {len(ref['faces'])} faces, largest cell {ref['members'].max()}, "
          f"max position error {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    if not jittered:
        assert (len(ref["verts"]), len(ref["faces"])) == {0.05: (4955, 9930), 0.11: (1319, 2634), 0.7: (26, 48), 3.0: (1, 0)}[cell]
        if cell == 0.7:
            assert ref["members"].max() > 256                                                        # a cell larger than a workgroup
    again = simplify_mesh(_t(v), _t(f), cell)
    assert torch.equal(got.verts, again.verts) and torch.equal(got.faces, again.faces) and torch.equal(got.vertex_map, again.vertex_map)


def test_simplify_small_cases():
    """-1 rows, faces that collapse onto one triple or one set with the other winding, a repeated corner, a vertex on a cell boundary,
    an unreferenced vertex."""
    from selfreconcode_amd.mesh_prep import simplify_mesh
    v = np.float32([[0, 0, 0], [0.01, 0, 0], [1, 0, 0], [1.01, 0, 0], [0, 1, 0], [0.01, 1, 0], [0.5, 0, 0], [0.75, 0.75, 0]])
    f = np.int64([[4, 2, 0], [-1, -1, -1], [0, 2, 4], [1, 3, 5], [0, 1, 2], [0, 6, 4], [3, -1, 2], [5, 6, 1]])
    got = simplify_mesh(_t(v), _t(f), 0.5)
    ref = mr.simplify(v, f, 0.5)
    assert got.vertex_map.tolist() == ref["vertex_map"].tolist() == [0, 0, 2, 2, 4, 4, 1, 3]          # 0.5 / 0.5 = 1: the boundary vertex is in the upper cell
    assert got.faces.tolist() == ref["faces"].tolist() == [[4, 2, 0], [0, 1, 4]]                    # the lower index survives, with its own winding
    assert got.verts.shape == (5, 3)                                                                # vertex 3 (old 7) stays although no face uses it
    np.testing.assert_allclose(got.verts.cpu().numpy(), ref["verts"], atol=1e-7)


def test_simplify_refusals():
    from selfreconcode_amd.mesh_prep import simplify_mesh, simplify_to
    v, f = _sphere32(False)
    tv, tf = _t(v), _t(f)
    for cell in (0., -1., float("nan")):
        with pytest.raises(ValueError):
            simplify_mesh(tv, tf, cell)
    for bad in (float("nan"), float("inf")):
        w = v.copy(); w[4001, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            simplify_mesh(_t(w), tf, 0.1)
        with pytest.raises(ValueError, match="non-finite"):
            simplify_to(_t(w), tf, 10 ** 6)
    with pytest.raises(ValueError, match="2\\^62"):
        simplify_mesh(tv, tf, 1e-19)                                                                 # (2 / 1e-19)^3 = 8e57 cells
    w = v.copy(); w[0] = (3e38, -3e38, 0.)
    with pytest.raises(ValueError, match="2\\^62"):
        simplify_mesh(_t(w), tf, 1.)                                                                 # hi - lo overflows float32
    with pytest.raises(RuntimeError):
        simplify_mesh(tv.cpu(), tf.cpu(), 0.1)                                                       # no CPU fallback


def test_simplify_to():
    from selfreconcode_amd.mesh_prep import simplify_mesh, simplify_to
    v, f = _sphere32(True)
    f = np.concatenate([f[:100], np.full((3, 3), -1), f[100:]])
    tv, tf = _t(v), _t(f)
    target, probes = 2000, []
    got = simplify_to(tv, tf, target, probes=probes)
    assert len(probes) == 17 and probes[0][0] == pytest.approx(float(np.ptp(v, 0).max()) / 2, rel=1e-6)
    assert 0 < got.faces.shape[0] <= target
    hit = [c for c, k in probes if k <= target]
    assert got.cell == min(hit)
    smaller = [(c, k) for c, k in probes if c < got.cell]
    assert smaller and max(smaller)[1] > target                                                     # the next smaller probed cell is over the budget
    direct = simplify_mesh(tv, tf, got.cell)
    assert torch.equal(direct.verts, got.verts) and torch.equal(direct.faces, got.faces) and dict(probes)[got.cell] == got.faces.shape[0]
    ref = mr.simplify(v, f, got.cell)
    assert np.array_equal(got.faces.cpu().numpy(), ref["faces"])
    same = simplify_to(tv, tf, len(f) - 3)                                                          # within the budget: cleaned, identity map
    assert same.cell == 0. and torch.equal(same.verts, tv) and same.vertex_map.tolist() == list(range(len(v)))
    assert np.array_equal(same.faces.cpu().numpy(), f[(f >= 0).all(1)])
    with pytest.raises(ValueError, match="coarsest"):
        simplify_to(tv, tf, 3)


def _unwrap_meshes(name):
    from selfreconcode_amd.mesh_prep import simplify_mesh
    from selfreconcode_amd.synthetic import cube_sphere, icosphere
    if name == "cube":
        return [x.numpy() for x in cube_sphere(1)]
    if name == "icosphere":
        return [x.numpy() for x in icosphere(2)]
    if name == "sphere8":
        return [x.numpy() for x in cube_sphere(8)]
    if name == "sphere8_jitter":
        v, f = [x.numpy() for x in cube_sphere(8)]
        return mr.jitter(v, 3, 0.01), f
    m = simplify_mesh(_t(_sphere32(False)[0]), _t(_sphere32(False)[1]), 0.11)
    return m.verts.cpu().numpy(), m.faces.cpu().numpy()


CHARTS = {"cube": 6, "icosphere": 6, "sphere8": 6, "sphere8_jitter": 28, "simplified": 54}      # (what the restatement finds; it is the authority)


@pytest.mark.parametrize("name", list(CHARTS))
def test_unwrap_vs_restatement(name):
    from selfreconcode_amd.mesh_prep import unwrap_charts
    from selfreconcode_amd.mesh_prep_ops import uv_overlap_count
    v, f = _unwrap_meshes(name)
    R, padding = 256, 2
    ref = mr.charts(v, f)
    at = unwrap_charts(_t(v), _t(f), R, padding)
    F, C = len(f), len(ref["labels"])
    assert C == CHARTS[name]
    assert tuple(at.vt.shape) == (3 * F, 2) and at.vt.dtype == torch.float32 and torch.equal(at.ft, torch.arange(3 * F, device=DEV).view(F, 3))
    assert np.array_equal(at.chart.cpu().numpy(), ref["chart"]) and np.array_equal(at.labels.cpu().numpy(), ref["labels"])
    assert np.array_equal(at.bbox_min.cpu().numpy(), ref["bbox_min"]) and np.array_equal(at.extent.cpu().numpy(), ref["extent"])
    origin, size = at.origin.cpu().numpy(), at.size.cpu().numpy()
    vt = at.vt.cpu().numpy().astype(np.float64)
    want = mr.chart_uv(ref, at.scale, origin, at.bbox_min.cpu().numpy(), padding, R)
    err = float(np.abs(vt - want).max())
    print(f"unwrap {name}: {F} faces, {C} charts, scale {at.scale:.4f}, rounds {at.rounds}, max |vt - restatement| {err:.3g}, overlap {at.overlap_texels}")
    assert err <= 1e-6
    assert vt.min() >= 0. and vt.max() <= 1.
    # packing: the formula, inside the atlas, pairwise disjoint, and every face inside its chart's rectangle less the padding
    assert at.scale > 0 and np.array_equal(size, np.ceil(ref["extent"].astype(np.float64) * at.scale).astype(np.int64) + 2 * padding + 1)
    lo, hi = origin, origin + size
    assert (lo >= 0).all() and (hi <= R).all()
    apart = ((hi[:, None, :] <= lo[None, :, :]) | (hi[None, :, :] <= lo[:, None, :])).any(-1) | np.eye(C, dtype=bool)
    assert apart.all()
    tex = vt.reshape(F, 3, 2) * R
    assert (tex >= (lo[ref["chart"]] + padding)[:, None, :]).all() and (tex <= (hi[ref["chart"]] - padding)[:, None, :]).all()
    # areas: positive in UV, and UV area R^2 / (surface area scale^2) = |n_axis| / |n| in [1 / sqrt(3), 1]
    _, n = mr.face_classes(v, f)
    surface2 = np.linalg.norm(n, axis=1)
    uv2 = mr.tri_area2(vt.reshape(F, 3, 2))
    solid = surface2 > 1e-12
    assert solid.sum() >= 0.99 * F and (uv2[solid] > 0).all()
    ratio = uv2[solid] * R * R / (surface2[solid] * at.scale ** 2)
    print(f"   UV / surface area in [{ratio.min():.6f}, {ratio.max():.6f}]")
    assert ratio.min() >= 1 / np.sqrt(3.) - 1e-4 and ratio.max() <= 1 + 1e-4
    # contested texels: none, and the operator agrees with the restatement
    contested, doubtful = mr.overlap_count(vt, at.ft.cpu().numpy(), R)
    assert at.overlap_texels == uv_overlap_count(at.vt, at.ft, R) == 0 and contested == 0
    assert at.rounds <= 64
    again = unwrap_charts(_t(v), _t(f), R, padding)
    for a, b in zip(at, again):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_unwrap_long_strip_is_one_chart_in_few_rounds():
    """1 x 20 000 quads: a component search that advances one face per round would need 40 000 rounds; 64 = 4 log2(40 000)."""
    from selfreconcode_amd.mesh_prep import unwrap_charts
    v, f = mr.flat_strip(20000)
    assert len(f) == 40000
    at = unwrap_charts(_t(v), _t(f), 1680, 2)
    print(f"strip: rounds {at.rounds}")
    assert at.labels.tolist() == [0] and int(at.chart.max()) == 0 and 2 <= at.rounds <= 64
    assert at.extent.tolist() == [[20000., 1.]] and at.bbox_min.tolist() == [[0., 0.]]
    assert at.scale == pytest.approx((1680 - 5) / 20000., rel=1e-6)


def test_unwrap_edge_cases():
    from selfreconcode_amd.mesh_prep import unwrap_charts
    from selfreconcode_amd.mesh_prep_ops import face_classes
    v, f = mr.fan_on_edge()
    at = unwrap_charts(_t(v), _t(f), 64, 1)
    assert at.chart.tolist() == [0, 0, 0] and at.labels.tolist() == [0]                             # a non-manifold edge joins all its faces
    # classes: a zero-area face is +x; ties go to the lowest axis; the sign follows the dominant component
    pts = np.float32([[0, 0, 0], [1, 1, 1], [2, 2, 2], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1]])
    faces = np.int64([[0, 1, 2], [3, 4, 5], [3, 5, 4], [0, 3, 6], [0, 6, 3], [0, 4, 3], [0, 0, 0]])
    cls = face_classes(_t(pts), _t(faces)).tolist()
    assert cls == mr.face_classes(pts, faces)[0].tolist() == [0, 0, 1, 3, 2, 5, 0]
    with pytest.raises(ValueError):
        unwrap_charts(_t(v), _t(np.int64([[0, 1, 7]])), 64, 1)                                      # an index outside the vertices
    with pytest.raises(ValueError, match="3 charts"):
        unwrap_charts(_t(np.concatenate([v, v + 5, v + 9])), _t(np.concatenate([f[:1], f[:1] + 5, f[:1] + 10])), 8, 2)
    with pytest.raises(RuntimeError):
        unwrap_charts(torch.from_numpy(v), torch.from_numpy(f), 64, 1)


def test_overlap_count_on_a_spiral_ramp():
    """Two turns of a ramp are one chart of class +z that covers itself in projection: the unwrap reports it, and does not repair it."""
    from selfreconcode_amd.mesh_prep import unwrap_charts
    from selfreconcode_amd.mesh_prep_ops import uv_overlap_count
    from selfreconcode_amd.texture_ops import uv_texel_map
    v, f = mr.spiral_ramp(turns=2, segments=64, r0=1., r1=2., pitch=0.15)
    R = 256
    at = unwrap_charts(_t(v), _t(f), R, 1)
    assert at.labels.tolist() == [0]
    contested, doubtful = mr.overlap_count(at.vt.cpu().numpy(), at.ft.cpu().numpy(), R)
    covered = int((uv_texel_map(at.vt, at.ft, R).face >= 0).sum())
    print(f"spiral: contested {at.overlap_texels} (restatement {contested}, doubtful {doubtful}), covered {covered}")
    assert contested > 30000 and at.overlap_texels > 0
    assert abs(at.overlap_texels - contested) <= doubtful
    assert at.overlap_texels <= covered
    assert uv_overlap_count(at.vt, at.ft, R) == at.overlap_texels
    assert uv_overlap_count(at.vt, at.ft, R, eps=0.34) == 0                                         # no point has three barycentrics above 1/3
    with pytest.raises(RuntimeError):
        uv_overlap_count(at.vt.cpu(), at.ft.cpu(), R)


RATIO = {'sdfRatio': 1., 'deformerRatio': 1., 'renderRatio': 1.}


def _files(root):
    """{relative path: bytes}; an .npz as the bytes of its arrays (the zip container stamps each entry with the time of writing)."""
    out = {}
    for dp, _, fns in os.walk(root):
        for fn in fns:
            path = os.path.join(dp, fn)
            if fn.endswith(".npz"):
                with np.load(path) as z:
                    out[os.path.relpath(path, root)] = {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}
            else:
                with open(path, "rb") as fh:
                    out[os.path.relpath(path, root)] = fh.read()
    return out


def test_prepare_template_into_export_texture(tmp_path):
    import _texture_ref as tr
    from selfreconcode_amd.mesh_prep import prepare_template
    from selfreconcode_amd.synthetic import build_synthetic_scene
    from selfreconcode_amd.mesh_io import read_obj_uv
    from selfreconcode_amd.texture import export_texture, texture_frames
    from selfreconcode_amd.texture_ops import uv_texel_map
    H = W = 96
    R = 256
    torch.manual_seed(0)
    net, ds, _ = build_synthetic_scene(device=DEV, frame_num=40, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)], lbs_volume_shape=(17, 57, 33),
                                       consistent_masks=False)
    fids = texture_frames(ds.frame_num, 6)
    views = [(int(f), tr.smooth_image(H, W, 0.3 * k), ds.batch(torch.tensor([int(f)], device=DEV))['mask'][0] > 0.5) for k, f in enumerate(fids)]
    trees = []
    for run in ("a", "b"):
        root = str(tmp_path / run)
        prep = prepare_template(net, root, target_faces=600, resolution=R)
        assert prep.obj_path == os.path.join(root, "template", "uvmap.obj") and 0 < prep.mesh.faces.shape[0] <= 600
        v, f, vt, ft = read_obj_uv(prep.obj_path)                                                   # the OBJ round-trips
        assert np.array_equal(v, prep.mesh.verts.cpu().numpy()) and np.array_equal(f, prep.mesh.faces.cpu().numpy())
        assert np.array_equal(vt, prep.atlas.vt.cpu().numpy()) and np.array_equal(ft, prep.atlas.ft.cpu().numpy())
        baked = export_texture(net, prep.obj_path, views, os.path.join(root, "template"), resolution=R, check_num=2)
        trees.append(_files(root))
    print(f"template: {prep.mesh.vertex_map.shape[0]} -> {prep.mesh.verts.shape[0]} vertices, {prep.mesh.faces.shape[0]} faces, "
          f"{prep.atlas.labels.shape[0]} charts, scale {prep.atlas.scale:.2f}, overlap {prep.atlas.overlap_texels}, "
          f"mask_final {baked.mask_final.sum()} of {baked.tex_mask.sum()} texels")
    assert sorted(trees[0]) == sorted(os.path.join("template", n) for n in ("mask_final.png", "tex_mask.png", "tex_median.png", "tex_predata.npz", "texture.png",
                                                                           "uvmap.obj", "view_id.npy"))
    assert trees[0] == trees[1]                                                                     # a second run writes identical files
    tmap = uv_texel_map(prep.atlas.vt, prep.atlas.ft, R)
    assert np.array_equal(baked.tex_mask, (tmap.face >= 0).cpu().numpy()) and baked.tex_mask.any()
    assert baked.mask_final.any() and not (baked.mask_final & ~baked.tex_mask).any()
    assert (baked.texture[baked.tex_mask] > 0).any(-1).all()                                        # the whole atlas received a colour


def test_meshprep_abi_argument_checks():
    """Every entry point refuses a null pointer or a size outside its domain with SR_EINVAL, before anything is launched."""
    from selfreconcode_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    P = _lib.ptr
    i32, i64 = torch.int32, torch.int64
    v = _t(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])); f = _t(np.int64([[0, 1, 2], [1, 3, 2]]))
    V, F, C, R = 4, 2, 1, 8
    box = torch.zeros(8, dtype=i32, device=DEV); key = torch.zeros(V, dtype=i64, device=DEV); lo = torch.zeros(3, device=DEV)
    order = torch.arange(V, device=DEV); offs = _t(np.int64([0, V])); mean = torch.zeros(C, 3, device=DEV)
    vmap = torch.arange(V, device=DEV); of = torch.zeros(F, 3, dtype=i64, device=DEV); kh = torch.zeros(F, dtype=i64, device=DEV); kl = torch.zeros_like(kh)
    perm = torch.arange(F, device=DEV); keep = torch.zeros(F, dtype=torch.uint8, device=DEV)
    cls = torch.zeros(F, dtype=i32, device=DEV); ek = torch.zeros(3 * F, dtype=i64, device=DEV); ep = torch.arange(3 * F, device=DEV)
    par = torch.arange(F, dtype=i32, device=DEV); nxt = torch.zeros_like(par); chg = torch.zeros(1, dtype=i32, device=DEV)
    chart = torch.zeros(F, dtype=i64, device=DEV); cbox = torch.zeros(C, 4, dtype=i32, device=DEV); bmin = torch.zeros(C, 2, device=DEV); ext = torch.zeros(C, 2, device=DEV)
    org = torch.zeros(C, 2, dtype=i64, device=DEV); vt = torch.zeros(3 * F, 2, device=DEV); ft = torch.arange(3 * F, device=DEV).view(F, 3)
    cnt = torch.zeros(R, R, dtype=i32, device=DEV); tot = torch.zeros(1, dtype=i64, device=DEV)
    calls = {
        "sr_meshprep_bounds": dict(a=P(v), V=V, b=P(box)),
        "sr_meshprep_cell_keys": dict(a=P(v), V=V, lo=P(lo), cell=0.5, nx=3, ny=3, nz=2, k=P(key)),
        "sr_meshprep_cell_mean": dict(a=P(v), V=V, o=P(order), off=P(offs), C=C, out=P(mean)),
        "sr_meshprep_face_keys": dict(f=P(f), F=F, m=P(vmap), V=V, Vn=V, of=P(of), kh=P(kh), kl=P(kl)),
        "sr_meshprep_face_first": dict(kh=P(kh), kl=P(kl), p=P(perm), F=F, keep=P(keep)),
        "sr_chart_classify": dict(a=P(v), V=V, f=P(f), F=F, c=P(cls)),
        "sr_chart_edge_keys": dict(f=P(f), F=F, V=V, c=P(cls), k=P(ek)),
        "sr_chart_hook": dict(k=P(ek), p=P(ep), n=3 * F, par=P(par), nxt=P(nxt), F=F, chg=P(chg)),
        "sr_chart_jump": dict(par=P(par), F=F, nxt=P(nxt), chg=P(chg)),
        "sr_chart_bbox": dict(a=P(v), V=V, f=P(f), F=F, c=P(cls), ch=P(chart), C=C, box=P(cbox), bmin=P(bmin), ext=P(ext)),
        "sr_chart_uv": dict(a=P(v), V=V, f=P(f), F=F, c=P(cls), ch=P(chart), C=C, bmin=P(bmin), org=P(org), scale=1., pad=1, R=R, vt=P(vt)),
        "sr_uv_overlap_count": dict(vt=P(vt), ft=P(ft), Vt=3 * F, F=F, R=R, eps=1e-6, cnt=P(cnt), tot=P(tot)),
    }
    keeps_zero = {("sr_chart_uv", "scale"), ("sr_chart_uv", "pad"), ("sr_uv_overlap_count", "eps")}          # 0 is a valid value there
    extra = {"sr_meshprep_cell_keys": [dict(cell=-1.), dict(cell=float("nan")), dict(nx=1 << 31, ny=1 << 31, nz=2)], "sr_meshprep_face_keys": [dict(Vn=(1 << 31) + 1)],
             "sr_chart_edge_keys": [dict(V=(1 << 30) + 1)], "sr_chart_hook": [dict(n=3 * F + 1)], "sr_chart_uv": [dict(scale=-1.), dict(pad=-1), dict(scale=float("nan"))],
             "sr_uv_overlap_count": [dict(eps=-1.), dict(R=40000)]}
    n = 0
    for name, args in calls.items():
        _lib.call(name, *args.values(), s)                                                           # the arguments as they are: accepted
        torch.cuda.synchronize()
        bad = [{k: 0} for k in args if (name, k) not in keeps_zero] + extra.get(name, [])
        for change in bad:
            with pytest.raises(_lib.SrError, match="SR_EINVAL"):
                _lib.call(name, *{**args, **change}.values(), s)
                pytest.fail(f"{name} accepted {change}")
            n += 1
    torch.cuda.synchronize()
    assert n > 80 and vt.isfinite().all() and int(tot) == 0
