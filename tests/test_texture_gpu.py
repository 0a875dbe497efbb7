"""Texture baking on the GPU (csrc/texture.hip, texture_ops, texture.bake_texture / export_texture) against the float64 restatement of
tests/_texture_ref.py (opendr / Isomapper semantics restated; parity unpinned), closed forms, bit-reproducibility, the written files and
the ABI's argument checks.  The shares of ill-conditioned texels excluded below are capped, and the caps are checked on the CPU
(tests/test_texture_cpu.py)."""
import json
import os

import numpy as np
import pytest
import torch

import _texture_ref as tr
from _png import read_png

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tex_median against the restatement: at most half an 8-bit step, 1/510 (what the written PNG resolves).  Measured on the MI355X
# (profiles/texture_parity.json): 9.3e-7 on scene a, 9.51e-7 on scene b -- more than 10x below that cap, so the bound is 10x the larger
# measurement.
COLOUR_CAP = 1. / 510.
COLOUR_BOUND = 9.6e-6


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _cameras(cam, H):
    from selfreconcode_amd.model.CameraMine import RectifiedPerspectiveCameras
    f32 = torch.float32
    return RectifiedPerspectiveCameras(torch.tensor(cam["f"], dtype=f32).view(1, 2), torch.tensor(cam["c"], dtype=f32).view(1, 2),
                                       torch.tensor(cam["R"], dtype=f32).view(1, 3, 3), torch.tensor(cam["T"], dtype=f32).view(1, 3),
                                       image_size=[(H, H)]).to(DEV)


def _view_terms(sc):
    """what bake_texture computes per view, from the scene's posed vertices: (visible, alpha, xy_pix, images, pix_to_face as face indices)"""
    from selfreconcode_amd.ops import rasterize_meshes, vertex_normals
    from selfreconcode_amd.texture_ops import face_visibility, view_alpha
    H = sc["H"]
    cams = _cameras(sc["cam"], H)
    verts, faces = _t(sc["verts"]), _t(sc["faces"])
    xy_ndc, z = cams.project_ndc(verts)
    p2f = rasterize_meshes(xy_ndc, z, faces, H, H).pix_to_face[..., 0]
    xy_pix, _ = cams.project(verts)
    alpha = view_alpha(verts, vertex_normals(verts, faces), cams.cam_pos())
    vis = face_visibility(p2f, faces, xy_pix, _t(sc["masks"]))
    p = p2f.cpu().numpy()
    F = len(sc["faces"])
    p = np.where(p >= 0, p - np.arange(len(p))[:, None, None] * F, -1)
    assert p.max() < F and (p >= 0).mean() > 0.1
    return vis, alpha, xy_pix.contiguous(), _t(sc["images"]), p


@pytest.mark.parametrize("name", ["icosphere", "hand"])
def test_uv_texel_map_vs_restatement(name):
    from selfreconcode_amd.synthetic import icosphere, per_face_atlas
    from selfreconcode_amd.texture_ops import uv_texel_map
    R = 256
    if name == "icosphere":
        vt, ft = per_face_atlas(len(icosphere(3)[1]), R, tr.ATLAS_MARGIN)
        vt, ft = vt.numpy(), ft.numpy()
    else:
        vt, ft = tr.hand_atlas()
    m = uv_texel_map(_t(vt), _t(ft), R)
    face, bary = tr.texel_map(vt, ft, R)
    assert m.face.dtype == torch.int32 and tuple(m.face.shape) == (R, R) and tuple(m.bary.shape) == (R, R, 3)
    near = (face >= 0) & (np.abs(bary).min(-1) < 1e-6)
    assert near.sum() <= 0.005 * (face >= 0).sum()
    got_f, got_b = m.face.cpu().numpy(), m.bary.cpu().numpy()
    assert np.array_equal(got_f[~near], face[~near])
    err = np.abs(got_b - bary)[~near].max()
    print(f"uv_texel_map {name}: covered {(face >= 0).sum()}, excluded {near.sum()}, max barycentric error {err:.3g}")
    assert err <= 1e-5
    assert (got_b[got_f < 0] == 0).all()
    # the compacted list
    t = m.texel.long().cpu().numpy()
    assert np.array_equal(t, np.nonzero(got_f.reshape(-1) >= 0)[0]) and np.array_equal(m.tface.cpu().numpy(), got_f.reshape(-1)[t])
    assert np.array_equal(m.tbary.cpu().numpy(), got_b.reshape(-1, 3)[t])
    m2 = uv_texel_map(_t(vt), _t(ft), R)
    assert torch.equal(m.face, m2.face) and torch.equal(m.bary, m2.bary) and torch.equal(m.texel, m2.texel)


@pytest.mark.parametrize("name", ["a", "b"])
def test_accumulate_resolve_vs_restatement(name):
    """(a) K = 8, defaults: no eviction.  (b) K = 12, agg_num 4, check_num 2, normal_ang 80: eviction, first-minimum ties of the empty slots."""
    from selfreconcode_amd.texture_ops import TextureAccumulator, uv_texel_map
    sc, kw = (tr.scene_a(), dict(agg_num=50, check_num=5, normal_ang=68.)) if name == "a" else (tr.scene_b(), tr.SCENE_B)
    R = sc["R"]
    vis, alpha, xy_pix, images, p2f = _view_terms(sc)
    m = uv_texel_map(_t(sc["vt"]), _t(sc["ft"]), R)
    acc = TextureAccumulator(m, _t(sc["faces"]), kw["agg_num"], kw["normal_ang"])
    acc.accumulate(sc["fids"], vis, alpha, xy_pix, images)
    got = acc.resolve(kw["check_num"])
    ref = tr.bake(sc["verts"], sc["faces"], sc["vt"], sc["ft"], sc["cam"], sc["images"], sc["masks"], sc["fids"], R, p2f=p2f, **kw)
    assert np.array_equal(m.face.cpu().numpy(), ref["face"])
    cov = ref["tex_mask"]
    T = cov.sum()
    excl = tr.excluded(ref)
    assert excl.sum() <= 0.02 * T
    keep = np.zeros((R, R), bool)
    keep[ref["rows"][~excl], ref["cols"][~excl]] = True
    count, fin, vid, med = [x.cpu().numpy() for x in got]
    assert count.dtype == np.int32 and fin.dtype == bool and vid.dtype == np.int32 and med.dtype == np.float32
    assert np.array_equal(fin[keep], ref["mask_final"][keep]) and np.array_equal(count[keep], ref["count"][keep])
    assert np.array_equal(vid[keep], ref["view_id"][keep])
    assert (count[~cov] == 0).all() and not fin[~cov].any() and (vid[~cov] == -1).all() and (med[~cov] == 0).all()
    assert not np.isnan(med).any() and not torch.isnan(acc.slot_rgb).any()
    err = float(np.abs(med - ref["tex_median"])[keep].max())
    seen = (ref["cos_all"] > ref["cosv0"]).sum(0)
    print(f"scene {name}: covered {T}, excluded {excl.sum()} ({excl.sum() / T:.4f}), mask_final {ref['mask_final'].sum()}, "
          f"texels with more candidates than slots {(seen > kw['agg_num']).sum()}, max |tex_median - restatement| {err:.3g} (cap {COLOUR_CAP:.3g})")
    if os.environ.get("SELFRECON_WRITE_PROFILES"):
        path = os.path.join(ROOT, "profiles", "texture_parity.json")
        data = json.load(open(path)) if os.path.isfile(path) else {}
        data[f"scene_{name}"] = {"covered_texels": int(T), "excluded_texels": int(excl.sum()), "mask_final_texels": int(ref["mask_final"].sum()),
                                 "max_abs_tex_median_error": err, "cap": COLOUR_CAP, "device": torch.cuda.get_device_name(0)}
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    assert 0.05 * T < ref["mask_final"].sum() < 0.9 * T
    if name == "b":
        assert (seen > kw["agg_num"]).sum() > 0.1 * T and int(acc.count.max()) == kw["agg_num"]
    assert err <= COLOUR_BOUND <= COLOUR_CAP


def test_batch_equals_sequence():
    from selfreconcode_amd.texture_ops import TextureAccumulator, uv_texel_map
    sc = tr.scene_b()
    vis, alpha, xy_pix, images, _ = _view_terms(sc)
    m = uv_texel_map(_t(sc["vt"]), _t(sc["ft"]), sc["R"])
    faces = _t(sc["faces"])
    one = TextureAccumulator(m, faces, 4, 80.)
    one.accumulate(sc["fids"], vis, alpha, xy_pix, images)
    seq = TextureAccumulator(m, faces, 4, 80.)
    for k in range(len(sc["fids"])):
        seq.accumulate(sc["fids"][k:k + 1], vis[k:k + 1], alpha[k:k + 1], xy_pix[k:k + 1], images[k:k + 1])
    split = TextureAccumulator(m, faces, 4, 80.)
    split.accumulate(sc["fids"][:5], vis[:5], alpha[:5], xy_pix[:5], images[:5])
    split.accumulate(sc["fids"][5:], vis[5:], alpha[5:], xy_pix[5:], images[5:])
    for other in (seq, split):
        for field in ("slot_cos", "slot_rgb", "slot_view", "count", "min_cos", "min_idx"):
            assert torch.equal(getattr(one, field), getattr(other, field)), field
        for a, b in zip(one.resolve(2), other.resolve(2)):
            assert torch.equal(a, b)
    assert int(one.count.max()) == 4 and (one.slot_view >= 0).any()
    # the filled slots of a texel are its first `count` slots
    filled = (one.slot_view >= 0)
    assert torch.equal(filled.sum(0).int(), one.count) and torch.equal(filled, torch.arange(4, device=DEV).view(4, 1) < one.count.view(1, -1))


def test_one_view_closed_form():
    """A fronto-parallel square (two triangles) whose UVs are its own x, y: the baked texture is the (affine) image resampled by the known
    affine map texel -> point -> pixel, and cosv is the analytic cosine at the (symmetric) corners."""
    from selfreconcode_amd.ops import rasterize_meshes, vertex_normals
    from selfreconcode_amd.texture_ops import TextureAccumulator, face_visibility, uv_texel_map, view_alpha
    H, R, a, Tz, f = 64, 40, 0.5, 2.4, 80.
    cam = {"f": np.array([f, f]), "c": np.array([31.5, 30.5]), "R": np.diag([-1., 1., -1.]), "T": np.array([0., 0., Tz])}
    cams = _cameras(cam, H)
    verts = torch.tensor([[[-a, -a, 0.], [a, -a, 0.], [a, a, 0.], [-a, a, 0.]]], device=DEV)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], device=DEV)
    vt = torch.tensor([[0., 0.], [1., 0.], [1., 1.], [0., 1.]], device=DEV)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
    coef = np.array([[0.1, 0.004, 0.007], [0.8, -0.005, -0.003], [0.3, 0.009, -0.002]])
    img = np.stack([c[0] + c[1] * x + c[2] * y for c in coef], -1).astype(np.float32)
    xy_ndc, z = cams.project_ndc(verts)
    p2f = rasterize_meshes(xy_ndc, z, faces, H, H).pix_to_face[..., 0]
    xy_pix, _ = cams.project(verts)
    nrm = vertex_normals(verts, faces)
    assert torch.equal(nrm, torch.tensor([0., 0., 1.], device=DEV).expand(1, 4, 3))
    alpha = view_alpha(verts, nrm, cams.cam_pos())
    cos = Tz / np.sqrt(2 * a * a + Tz * Tz)
    np.testing.assert_allclose(alpha.cpu().numpy(), cos, atol=1e-6)
    vis = face_visibility(p2f, faces, xy_pix, torch.ones(1, H, H, dtype=torch.bool, device=DEV))
    assert vis.tolist() == [[1, 1]]
    m = uv_texel_map(vt, faces, R)
    assert bool((m.face >= 0).all())
    acc = TextureAccumulator(m, faces, 3, 68.)
    acc.accumulate([9], vis, alpha, xy_pix, _t(img)[None])
    got = acc.resolve(1)
    assert bool(got.mask_final.all()) and bool((got.view_id == 9).all()) and bool((got.count == 1).all())
    np.testing.assert_allclose(acc.slot_cos[0].cpu().numpy(), cos, atol=1e-6)
    assert bool((acc.slot_view[1:] == -1).all())
    r, c = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    X, Y = -a + 2 * a * (c + 0.5) / R, -a + 2 * a * (1 - (r + 0.5) / R)
    px, py = cam["c"][0] + f * X / Tz, cam["c"][1] - f * Y / Tz
    expect = coef[:, 0] + px[..., None] * coef[:, 1] + py[..., None] * coef[:, 2]
    # float32: pixel positions (< 64) carry ~4e-6, times slopes < 0.01, plus a few roundings of values < 1
    np.testing.assert_allclose(got.tex_median.cpu().numpy(), expect, atol=2e-6)
    # a view from behind (the normals flipped) adds nothing; a masked-out corner hides both faces
    back = view_alpha(verts, -nrm, cams.cam_pos())
    assert float(back.abs().max()) == 0.
    mask = torch.ones(1, H, H, dtype=torch.bool, device=DEV)
    cx, cy = [int(v) for v in torch.round(xy_pix[0, 2]).tolist()]
    mask[0, cy, cx] = False
    assert face_visibility(p2f, faces, xy_pix, mask).tolist() == [[0, 0]]


@pytest.mark.parametrize("R", [100, 75])
def test_fill(R):
    from selfreconcode_amd.synthetic import det_array
    from selfreconcode_amd.texture_ops import fill
    rr, cc = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    tex_mask = ((rr - 0.45 * R) ** 2 + (cc - 0.5 * R) ** 2 < (0.3 * R) ** 2) | ((rr > 0.8 * R) & (cc < 0.3 * R))
    noise = det_array((R, R), 5, 1.0)
    fin = tex_mask & (noise > -0.2) & (cc > 0.35 * R)                       # holes everywhere, and a part of the atlas never seen
    med = np.where(fin[..., None], 0.5 + 0.5 * det_array((R, R, 3), 6, 1.0), 0.).astype(np.float32)
    out = fill(_t(med), _t(fin), _t(tex_mask))
    ref = tr.fill(med, fin, tex_mask)
    got = out.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got[fin], med[fin])   # mask_final texels: bit for bit
    region = tr.dilate(tex_mask, int(0.1 * R)) & ~fin
    assert (got[~region & ~fin] == 0).all() and region.sum() > 0.1 * R * R
    err = np.abs(got - ref).max()
    print(f"fill R = {R}: region {region.sum()} texels, max |fill - restatement| {err:.3g}")
    assert err <= 1e-5
    assert got[region].min() > 0.                                            # every region texel received a colour
    const = np.where(fin[..., None], np.float32([0.25, 0.5, 0.75]), 0.).astype(np.float32)
    got = fill(_t(const), _t(fin), _t(tex_mask)).cpu().numpy()
    np.testing.assert_allclose(got[region | fin], np.broadcast_to([0.25, 0.5, 0.75], ((region | fin).sum(), 3)), atol=1e-6)
    assert (got[~(region | fin)] == 0).all()
    assert torch.equal(out, fill(_t(med), _t(fin), _t(tex_mask)))
    assert float(fill(_t(med), _t(np.zeros_like(fin)), _t(tex_mask)).abs().max()) == 0.
    assert torch.equal(fill(_t(med), _t(fin), _t(tex_mask), dilate=0)[_t(~tex_mask)], torch.zeros(int((~tex_mask).sum()), 3, device=DEV))


RATIO = {'sdfRatio': 1., 'deformerRatio': 1., 'renderRatio': 1.}


def test_export_texture_files_and_reproducibility(tmp_path):
    from selfreconcode_amd.synthetic import build_synthetic_scene, per_face_atlas
    from selfreconcode_amd.mesh_io import write_obj_uv
    from selfreconcode_amd.texture import export_texture, texture_frames
    H = W = 96
    R = 256
    torch.manual_seed(0)
    net, ds, _ = build_synthetic_scene(device=DEV, frame_num=40, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)], lbs_volume_shape=(17, 57, 33),
                                       consistent_masks=False)
    verts, faces = net.discretizeSDF(RATIO, None, 0.0)
    faces = faces[(faces >= 0).all(1)].contiguous()                          # (an OBJ cannot hold marching cubes' -1 border faces)
    vt, ft = per_face_atlas(faces.shape[0], R, tr.ATLAS_MARGIN)
    obj = str(tmp_path / "uvmap.obj")
    write_obj_uv(obj, verts.detach().cpu().numpy(), faces.cpu().numpy(), vt.numpy(), ft.numpy())
    fids = texture_frames(ds.frame_num, 6)
    assert fids.tolist() == [0, 7, 14, 20, 27, 34]
    views = [(int(f), tr.smooth_image(H, W, 0.3 * k), ds.batch(torch.tensor([int(f)], device=DEV))['mask'][0] > 0.5) for k, f in enumerate(fids)]
    out_root = str(tmp_path / "template")
    baked = export_texture(net, obj, views, out_root, resolution=R, check_num=2)
    assert sorted(os.listdir(out_root)) == ["mask_final.png", "tex_mask.png", "tex_median.png", "tex_predata.npz", "texture.png", "view_id.npy"]
    assert baked.tex_mask.shape == (R, R) and baked.tex_mask.dtype == bool and baked.texture.shape == (R, R, 3)
    nfin = baked.mask_final.sum()
    assert 0.02 * baked.tex_mask.sum() < nfin < baked.tex_mask.sum() and not (baked.mask_final & ~baked.tex_mask).any()
    assert set(np.unique(baked.view_id)) <= {-1, *fids.tolist()} and (baked.view_id[baked.mask_final] >= 0).all()
    assert 0. <= baked.texture.min() and baked.texture.max() <= 1. and np.array_equal(baked.texture[baked.mask_final], baked.tex_median[baked.mask_final])
    assert (baked.texture[baked.tex_mask] > 0).any(-1).all()                 # the whole atlas received a colour
    for name, arr in (("tex_mask", baked.tex_mask), ("mask_final", baked.mask_final), ("tex_median", baked.tex_median), ("texture", baked.texture)):
        png = read_png(os.path.join(out_root, name + ".png"))
        want = np.uint8(np.asarray(arr, np.float32) * 255)
        assert np.array_equal(png.reshape(want.shape), want), name
    assert np.array_equal(np.load(os.path.join(out_root, "view_id.npy")), baked.view_id)
    pre = np.load(os.path.join(out_root, "tex_predata.npz"))
    assert sorted(pre.files) == ["defVs", "fids", "fs", "ft", "tmpvs", "vt"]
    assert np.array_equal(pre["fids"], fids) and pre["defVs"].shape == (6, verts.shape[0], 3) and np.array_equal(pre["fs"], faces.cpu().numpy())
    with torch.no_grad():
        poses, trans, d_cond, _ = ds.get_grad_parameters(torch.tensor([14], device=DEV))
        dv = net.deformer(verts.detach()[None], [d_cond, [poses, trans]], ratio=RATIO)
    np.testing.assert_allclose(pre["defVs"][2], dv[0].cpu().numpy(), atol=1e-6)
    # a second full bake, through OptimNetwork.bake_texture and with another batching: identical bits
    again = net.bake_texture(verts.detach(), faces, vt.to(DEV), ft.to(DEV), iter(views), resolution=R, check_num=2, batch=4)
    for a, b in zip(baked, again):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        net.bake_texture(verts.detach(), faces, vt.to(DEV), ft.to(DEV), [], resolution=R)
    with pytest.raises(RuntimeError):
        net.bake_texture(verts.detach().cpu(), faces.cpu(), vt, ft, views, resolution=R)          # no CPU fallback


def test_texture_abi_argument_checks():
    from selfreconcode_amd import _lib
    from selfreconcode_amd.texture_ops import TextureAccumulator, fill, uv_texel_map
    s = torch.cuda.current_stream().cuda_stream
    P = _lib.ptr
    R, H, A, T = 8, 4, 2, 64
    vt = torch.tensor([[0., 0.], [1., 0.], [1., 1.], [0., 1.]], device=DEV)
    ft = torch.tensor([[0, 1, 2], [0, 2, 3]], device=DEV)
    face = torch.zeros(R, R, dtype=torch.int32, device=DEV); bary = torch.zeros(R, R, 3, device=DEV)
    p2f = torch.full((1, H, H), -1, dtype=torch.int64, device=DEV); xy = torch.ones(1, 4, 2, device=DEV)
    mask = torch.ones(1, H, H, dtype=torch.uint8, device=DEV); vis = torch.zeros(1, 2, dtype=torch.uint8, device=DEV)
    v = torch.zeros(1, 4, 3, device=DEV); cam = torch.ones(1, 3, device=DEV); alpha = torch.zeros(1, 4, device=DEV)
    img = torch.zeros(1, H, H, 3, device=DEV); fid = torch.zeros(1, dtype=torch.int32, device=DEV)

    def uv(a=P(vt), b=P(ft), Vt=4, F=2, R_=R, f=P(face), ba=P(bary)):
        _lib.call("sr_uv_rasterize", a, b, Vt, F, R_, f, ba, s)

    def visf(p=P(p2f), f=P(ft), N=1, V=4, F=2, x=P(xy), m=P(mask), H_=H, W_=H, o=P(vis)):
        _lib.call("sr_face_visibility", p, f, N, V, F, x, m, H_, W_, o, s)

    def alf(a=P(v), b=P(v), c=P(cam), N=1, V=4, o=P(alpha)):
        _lib.call("sr_view_alpha", a, b, c, N, V, o, s)
    uv(); visf(); alf()
    torch.cuda.synchronize()
    assert bool((face >= 0).all()) and T == R * R
    tf = face.view(-1).contiguous(); tb = bary.view(-1, 3).contiguous(); tex = torch.arange(T, dtype=torch.int32, device=DEV)
    sc = torch.full((A, T), 0.3, device=DEV); sr = torch.zeros(A, 3, T, device=DEV); sv = torch.full((A, T), -1, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(T, dtype=torch.int32, device=DEV); mc = torch.full((T,), 0.3, device=DEV); mi = torch.zeros(T, dtype=torch.int32, device=DEV)
    ocnt = torch.zeros(T, dtype=torch.int32, device=DEV); ofin = torch.zeros(T, dtype=torch.uint8, device=DEV)
    ovid = torch.zeros(T, dtype=torch.int32, device=DEV); omed = torch.zeros(T, 3, device=DEV)
    ws = torch.zeros(int(_lib.raw("sr_texture_fill_workspace_bytes")(R)) + 16, dtype=torch.uint8, device=DEV)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 16
    otex = torch.zeros(R, R, 3, device=DEV)

    def accf(T_=T, a=P(tf), b=P(tb), f=P(ft), F=2, V=4, N=1, vi=P(vis), al=P(alpha), x=P(xy), im=P(img), H_=H, W_=H, fi=P(fid), A_=A, c0=0.3,
             s0=P(sc), s1=P(sr), s2=P(sv), c=P(cnt), m0=P(mc), m1=P(mi)):
        _lib.call("sr_texture_accumulate", T_, a, b, f, F, V, N, vi, al, x, im, H_, W_, fi, A_, c0, s0, s1, s2, c, m0, m1, s)

    def resf(T_=T, t=P(tex), A_=A, c0=0.3, ck=1, s0=P(sc), s1=P(sr), s2=P(sv), c=P(ocnt), f=P(ofin), vi=P(ovid), m=P(omed)):
        _lib.call("sr_texture_resolve", T_, t, A_, c0, ck, s0, s1, s2, c, f, vi, m, s)

    def fillf(a=P(omed), b=P(ofin), c=P(ofin), R_=R, k=1, o=P(otex), w=wp):
        _lib.call("sr_texture_fill", a, b, c, R_, k, o, w, s)
    accf(); resf(); fillf()
    torch.cuda.synchronize()
    assert int(cnt.max()) == 0 and int(ofin.max()) == 0 and float(otex.abs().max()) == 0.
    bad = [lambda k=k: uv(**{k: 0}) for k in ("a", "b", "Vt", "F", "R_", "f", "ba")] + [lambda: uv(R_=-3), lambda: uv(F=-1)]
    bad += [lambda k=k: visf(**{k: 0}) for k in ("p", "f", "N", "V", "F", "x", "m", "H_", "W_", "o")]
    bad += [lambda k=k: alf(**{k: 0}) for k in ("a", "b", "c", "N", "V", "o")]
    bad += [lambda k=k: accf(**{k: 0}) for k in ("T_", "a", "b", "f", "F", "V", "N", "vi", "al", "x", "im", "H_", "W_", "fi", "A_", "s0", "s1", "s2", "c", "m0", "m1")]
    bad += [lambda: accf(A_=-1), lambda: accf(c0=-0.1), lambda: accf(c0=float("nan"))]
    bad += [lambda k=k: resf(**{k: 0}) for k in ("T_", "t", "A_", "ck", "s0", "s1", "s2", "c", "f", "vi", "m")] + [lambda: resf(A_=-2)]
    bad += [lambda k=k: fillf(**{k: 0}) for k in ("a", "b", "c", "R_", "o", "w")] + [lambda: fillf(k=-1), lambda: fillf(w=wp + 4), lambda: fillf(R_=-1)]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.SrError, match="SR_EINVAL"):
            call()
            pytest.fail(f"case {i} accepted")
    assert _lib.raw("sr_texture_fill_workspace_bytes")(0) < 0 and _lib.raw("sr_texture_fill_workspace_bytes")(-5) < 0
    torch.cuda.synchronize()
    # the operators: CPU tensors, bad parameters and non-square images raise
    m = uv_texel_map(vt, ft, R)
    with pytest.raises(RuntimeError):
        uv_texel_map(vt.cpu(), ft.cpu(), R)
    with pytest.raises(_lib.SrError):
        uv_texel_map(vt, ft, 0)
    with pytest.raises(RuntimeError):
        fill(omed.view(R, R, 3).cpu(), ofin.view(R, R).cpu(), ofin.view(R, R).cpu())
    for kw in (dict(agg_num=0), dict(normal_ang=95.), dict(normal_ang=-1.)):
        with pytest.raises(ValueError):
            TextureAccumulator(m, ft, **kw)
    acc = TextureAccumulator(m, ft, 2, 68.)
    with pytest.raises(ValueError):
        acc.resolve(0)
    with pytest.raises(RuntimeError, match="non-square"):
        acc.accumulate([0], vis, alpha, xy, torch.zeros(1, H, H + 2, 3, device=DEV))
    with pytest.raises(RuntimeError):
        acc.accumulate([0], vis.cpu(), alpha.cpu(), xy.cpu(), img.cpu())
