"""Shaded mesh previews (csrc/shade.hip, ops.vertex_normals / shade_phong, OptimNetwork.infer with shaded_previews): vertex normals
and Phong shading against float64 restatements of pytorch3d 0.4.0's Meshes.verts_normals_packed and HardPhongShader (third-party
semantics, restated here; parity unpinned), a closed-form pixel, the infer wiring, and the ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch
from oracle import fixtures as fx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIO = {'sdfRatio': 1., 'deformerRatio': 0.62, 'renderRatio': 1.}


def _camera(H, W, f=(130., 128.), c=(31.3, 32.6), T=(0.02, -0.03, 2.4)):
    from selfreconcode_amd.model.CameraMine import RectifiedPerspectiveCameras
    R = torch.tensor([[-1., 0., 0.], [0., 1., 0.], [0., 0., -1.]])
    return RectifiedPerspectiveCameras(torch.tensor([f]), torch.tensor([c]), R.view(1, 3, 3), torch.tensor([T]), image_size=[(W, H)]).to(DEV)


def _mesh():
    """The ragged mesh of test_raster_gpu (a -1 face) + an isolated vertex (40), a face with a repeated index and a zero-area face on
    three exactly collinear vertices (41-43)."""
    V, F = 40, 70
    verts = fx.det_tensor((2, V, 3), 1, 1.0) * torch.tensor([0.45, 0.45, 0.25])
    faces = (np.abs(fx.det_array((F, 3), 3, 1000.0)).astype(np.int64)) % V
    faces[5] = -1
    extra = torch.tensor([[0.3, 0.1, 0.0], [0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [-0.5, 0.0, 0.0]]).expand(2, 4, 3)
    verts = torch.cat([verts, extra], 1)
    faces = np.concatenate([faces, [[3, 3, 7], [41, 42, 43]]])
    return verts, faces


def _normals_ref(verts, faces):
    """float64 restatement: corner cross products summed per vertex, skipping faces with a -1, then n / max(|n|, 1e-6)."""
    v = verts.double().numpy()
    out = np.zeros_like(v)
    for f in faces:
        if (f < 0).any():
            continue
        for c in range(3):
            a, b, d = f[c], f[(c + 1) % 3], f[(c + 2) % 3]
            out[:, a] += np.cross(v[:, b] - v[:, a], v[:, d] - v[:, a])
    return out / np.maximum(np.linalg.norm(out, axis=-1, keepdims=True), 1e-6)


def test_vertex_normals_vs_restatement_and_reproducible():
    from selfreconcode_amd.ops import vertex_adjacency, vertex_normals
    verts, faces = _mesh()
    fd = torch.from_numpy(faces).to(DEV)
    n = vertex_normals(verts.to(DEV), fd)
    ref = _normals_ref(verts, faces)
    assert n.shape == verts.shape and n.dtype == torch.float32
    np.testing.assert_allclose(n.cpu().numpy(), ref, rtol=0, atol=1e-6)
    assert float(n[:, 40:].abs().max()) == 0.0                         # isolated vertex and the zero-area face: 0
    adj = vertex_adjacency(fd, verts.shape[1])
    assert int(adj.offsets[-1]) == 3 * (len(faces) - 1)                # every corner of every face without a -1
    n2 = vertex_normals(verts.to(DEV), fd, adj)
    adj2 = vertex_adjacency(fd, verts.shape[1])
    assert torch.equal(adj.offsets, adj2.offsets) and torch.equal(adj.nbr[:int(adj.offsets[-1])], adj2.nbr[:int(adj2.offsets[-1])])
    assert torch.equal(n, n2) and torch.equal(n2, vertex_normals(verts.to(DEV), fd, adj2))


def _normalize(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-6)


def _shade_ref(verts, normals, faces, p2f, bary, cam, light, ka=0.5, kd=0.3, ks=0.2, shin=64.):
    """float64 restatement of phong_shading + hard_rgb_blend on given fragments; returns RGB [N,H,W,3] and the covered mask."""
    N, H, W = p2f.shape
    F = faces.shape[0]
    out = np.ones((N, H, W, 3))
    cov = p2f >= 0
    i, r, c = np.nonzero(cov)
    pf = p2f[cov]
    fi, f = pf // F, pf % F
    b = bary[cov].astype(np.float64)
    fv = faces[f]
    p = np.einsum('pk,pkj->pj', b, verts[fi[:, None], fv])
    nn = _normalize(np.einsum('pk,pkj->pj', b, normals[fi[:, None], fv]))
    L = _normalize(light[i] - p)
    Vd = _normalize(cam[i] - p)
    cos = (nn * L).sum(-1)
    refl = -L + 2 * cos[:, None] * nn
    alpha = np.maximum((Vd * refl).sum(-1), 0) * (cos > 0)
    rgb = (ka + kd * np.maximum(cos, 0)) * b.sum(-1) + ks * alpha ** shin
    out[i, r, c] = rgb[:, None]
    return out, cov


def test_shade_phong_vs_restatement():
    from selfreconcode_amd.ops import rasterize_meshes, shade_phong, vertex_normals
    H = W = 48
    verts, faces = _mesh()
    fd = torch.from_numpy(faces).to(DEV)
    cam = _camera(H, W)
    xy, z = cam.project_ndc(verts.to(DEV))
    fr = rasterize_meshes(xy, z, fd, H, W)
    nrm = vertex_normals(verts.to(DEV), fd)
    campos = cam.cam_pos().view(1, 3).expand(2, 3)
    light = torch.tensor([[0., 1., 0.], [0.4, 0.8, 2.5]], device=DEV)              # one light per image
    rgba = shade_phong(verts.to(DEV), nrm, fd, fr, campos, light)
    assert rgba.shape == (2, H, W, 4) and rgba.dtype == torch.float32
    ref, cov = _shade_ref(verts.double().numpy(), nrm.double().cpu().numpy(), faces, fr.pix_to_face[..., 0].cpu().numpy(),
                          fr.bary_coords[..., 0, :].cpu().numpy(), campos.double().cpu().numpy(), light.double().cpu().numpy())
    out = rgba.cpu().numpy()
    assert cov.sum() > 300 and (~cov).sum() > 300
    np.testing.assert_allclose(out[..., :3][cov], ref[cov], rtol=0, atol=1e-4)
    assert (out[..., :3][~cov] == 1.0).all() and (out[..., 3] == 1.0).all()
    assert float(out[..., :3][cov].max()) > 0.85                                     # (some specular highlight is exercised)
    assert torch.equal(rgba, shade_phong(verts.to(DEV), nrm, fd, fr, campos, light))


def test_shade_phong_closed_form_quad():
    """A quad in z = 0 facing a camera on the z axis, light on the axis behind the camera: the centre pixel sees n = L = V, i.e.
    0.5 + 0.3 + 0.2; an off-centre pixel equals the formula evaluated by hand at the ray's intersection with the plane."""
    from selfreconcode_amd.ops import rasterize_meshes, shade_phong, vertex_normals
    H = W = 65
    f, Tz, Lz = 40., 2.4, 3.0
    cam = _camera(H, W, f=(f, f), c=((W - 1) / 2., (H - 1) / 2.), T=(0., 0., Tz))
    verts = torch.tensor([[[-1., -1.1, 0.], [1.3, -1.1, 0.], [1.3, 1., 0.], [-1., 1., 0.]]], device=DEV)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], device=DEV)
    xy, z = cam.project_ndc(verts)
    fr = rasterize_meshes(xy, z, faces, H, W)
    nrm = vertex_normals(verts, faces)
    assert torch.equal(nrm, torch.tensor([0., 0., 1.], device=DEV).expand(1, 4, 3))
    campos = cam.cam_pos()
    assert torch.allclose(campos, torch.tensor([0., 0., Tz], device=DEV))
    rgba = shade_phong(verts, nrm, faces, fr, campos, (0., 0., Lz)).cpu().numpy()
    np.testing.assert_allclose(rgba[0, 32, 32, :3], 1.0, atol=1e-4)
    for r, c in [(20, 45), (48, 18), (40, 30)]:
        assert int(fr.pix_to_face[0, r, c, 0]) >= 0
        xn, yn = 1. - (2. * c + 1.) / W, 1. - (2. * r + 1.) / H                     # pixel centre in NDC
        X, Y = -xn * Tz * W / (2. * f), yn * Tz * H / (2. * f)                    # camera frame (-X, Y, Tz): x_ndc = (2f/W) (-X) / Tz
        l = np.array([-X, -Y, Lz]); l /= np.linalg.norm(l)
        v = np.array([-X, -Y, Tz]); v /= np.linalg.norm(v)
        cos = l[2]
        refl = 2 * cos * np.array([0., 0., 1.]) - l
        expect = 0.5 + 0.3 * cos + 0.2 * max(float(v @ refl), 0.) ** 64
        np.testing.assert_allclose(rgba[0, r, c, :3], expect, atol=1e-4)
    assert (rgba[0, 0, 0] == 1.0).all()                                            # a corner is background: (1, 1, 1, 1)


def test_shade_abi_argument_checks():
    from selfreconcode_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    faces = torch.tensor([[0, 1, 2]], device=DEV)
    off = torch.zeros(4, dtype=torch.int64, device=DEV); cur = torch.zeros(3, dtype=torch.int32, device=DEV)
    nbr = torch.zeros(3, 2, dtype=torch.int32, device=DEV)
    v = torch.zeros(1, 3, 3, device=DEV); nrm = torch.zeros_like(v)
    p2f = torch.full((1, 2, 2), -1, dtype=torch.int64, device=DEV); bary = torch.zeros(1, 2, 2, 3, device=DEV)
    cam = torch.zeros(1, 3, device=DEV); rgba = torch.zeros(1, 2, 2, 4, device=DEV)
    coeffs = (ctypes.c_float * 13)(*([0.5] * 3 + [0.3] * 3 + [0.2] * 3 + [64.] + [1.] * 3))
    P = _lib.ptr
    adj = lambda f=P(faces), V=3, F=1, o=P(off), c=P(cur), n=P(nbr): _lib.call("sr_vertex_adjacency", f, V, F, o, c, n, s)
    nor = lambda vv=P(v), N=1, V=3, o=P(off), n=P(nbr), out=P(nrm): _lib.call("sr_vertex_normals", vv, N, V, o, n, out, s)

    def shade(vv=P(v), nn=P(nrm), f=P(faces), N=1, V=3, F=1, H=2, W=2, p=P(p2f), b=P(bary), c=P(cam), l=P(cam), h=coeffs, o=P(rgba)):
        _lib.call("sr_shade_phong", vv, nn, f, N, V, F, H, W, p, b, c, l, h, o, s)
    adj(); nor(); shade()
    torch.cuda.synchronize()
    assert (rgba == 1).all() and torch.equal(off, torch.tensor([0, 1, 2, 3], device=DEV))
    bad = [lambda: adj(f=0), lambda: adj(o=0), lambda: adj(c=0), lambda: adj(n=0), lambda: adj(V=0), lambda: adj(F=0), lambda: adj(F=1 << 32),
           lambda: adj(n=P(nbr) + 4),
           lambda: nor(vv=0), lambda: nor(o=0), lambda: nor(n=0), lambda: nor(out=0), lambda: nor(N=0), lambda: nor(V=0)]
    bad += [lambda k=k: shade(**{k: 0}) for k in ("vv", "nn", "f", "p", "b", "c", "l", "h", "o", "N", "V", "F", "H", "W")]
    bad += [lambda: shade(F=1 << 32), lambda: shade(F=-1), lambda: shade(o=P(rgba) + 4)]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.SrError, match="SR_EINVAL"):
            call()
            pytest.fail(f"case {i} accepted")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ infer with the previews on (the scene of test_infer_gpu.py)
H = W = 96


def _scene():
    from selfreconcode_amd.synthetic import build_synthetic_scene
    torch.manual_seed(0)
    net, ds, conf = build_synthetic_scene(device=DEV, frame_num=40, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)],
                                          lbs_volume_shape=(17, 57, 33), consistent_masks=False)
    net.point_radius = 0.03
    # the depth in the translations, as in the reference's data (the front camera of def1imgs has T = their mean); the frame camera
    # moves back by the same amount, so the frames see what test_infer_gpu's scene sees
    with torch.no_grad():
        ds.trans[:, 2] += 2.4
        ds.camera_params['world2cam_coord_trans'][2] += 2.4
    return net, ds


def test_infer_shaded_previews():
    from selfreconcode_amd.ops import shade_phong, vertex_normals, rasterize_meshes
    from selfreconcode_amd.model.CameraMine import RectifiedPerspectiveCameras
    net, ds = _scene()
    assert net.shaded_previews is False
    fids = torch.tensor([3, 11], device=DEV)
    verts, faces = net.discretizeSDF(RATIO, None, 0.0)
    gts0 = {'mask': ds.batch(fids)['mask']}
    c0, i0, d0, v0 = net.infer(verts, faces, H, W, RATIO, fids, gts=gts0)
    assert i0 is None and d0 is None
    net.shaded_previews = True
    gts1 = {'mask': gts0['mask'].clone()}
    c1, imgs, def1imgs, v1 = net.infer(verts, faces, H, W, RATIO, fids, gts=gts1)
    assert np.array_equal(c0, c1) and np.array_equal(v0, v1) and gts0['maskE'].tobytes() == gts1['maskE'].tobytes()
    assert imgs.dtype == np.uint8 and imgs.shape == (2, H, W, 3) and def1imgs.dtype == np.uint8 and def1imgs.shape == (2, H, W, 4)
    out = net.render_frames(fids, RATIO, TmpVs=verts, Tmpfs=faces, chunk=10000, with_normals=False)
    dv, fr = out['def_verts'], out['frags']
    cameras, _, _ = net._cameras(2, DEV)
    ref = shade_phong(dv, vertex_normals(dv, faces), faces, fr, cameras.cam_pos(), (0., 1., 0.))
    ref8 = torch.clamp(ref[..., :3] * 255., 0., 255.).cpu().numpy().astype(np.uint8)
    assert np.array_equal(imgs, ref8)
    cov = (out['mask'] > 0).cpu().numpy()
    assert 0.05 < cov.mean() < 0.9
    assert (imgs[~cov] == 255).all() and (imgs[cov] != 255).any(-1).mean() > 0.99
    # the front view of the template plus the non-rigid offset
    assert (def1imgs[..., 3] == 255).all()
    front_cov = (def1imgs[..., :3] != 255).any(-1).mean()
    assert 0.02 < front_cov < 0.9, front_cov
    with torch.no_grad():
        cv = net.deformer.defs[0](verts[None].expand(2, -1, 3), ds.get_grad_parameters(fids)[2], ratio=RATIO)
        T = ds.trans.detach().mean(0)
        fc = RectifiedPerspectiveCameras(ds.camera_params['focal_length'].view(1, 2), ds.camera_params['princeple_points'].view(1, 2),
                                         torch.diag(torch.tensor([-1., 1., -1.], device=DEV)).view(1, 3, 3), T.view(1, 3), image_size=[(W, H)])
        xy, z = fc.project_ndc(cv)
        d_ref = shade_phong(cv, vertex_normals(cv, faces), faces, rasterize_meshes(xy, z, faces, H, W), fc.cam_pos(), (0., 1., float(T[2])))
    assert np.array_equal(def1imgs, torch.clamp(d_ref * 255., 0., 255.).cpu().numpy().astype(np.uint8))
    # overlay: background pixels from the (BGR) image, RGB-swapped; everything else as without it
    image = torch.rand(2, H, W, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    gts2 = {'mask': gts0['mask'].clone(), 'image': image}
    c2, imgs2, def2, v2 = net.infer(verts, faces, H, W, RATIO, fids, gts=gts2)
    bg = torch.clamp(image[..., [2, 1, 0]] * 255., 0., 255.).cpu().numpy().astype(np.uint8)
    assert np.array_equal(imgs2[~cov], bg[~cov]) and np.array_equal(imgs2[cov], imgs[cov]) and np.array_equal(def2, def1imgs)
    assert np.array_equal(v2, v0)
    # notcolor: no colour pass, both previews
    gts3 = {'mask': gts0['mask'].clone()}
    c3, imgs3, def3, v3 = net.infer(verts, faces, H, W, RATIO, fids, notcolor=True, gts=gts3)
    assert c3 is None and np.array_equal(imgs3, imgs) and np.array_equal(def3, def1imgs) and np.array_equal(v3, v0)
    assert gts3['maskE'].tobytes() == gts0['maskE'].tobytes()
    # without gts: RGBA
    _, imgs4, _, _ = net.infer(verts, faces, H, W, RATIO, fids, notcolor=True)
    assert imgs4.shape == (2, H, W, 4) and np.array_equal(imgs4[..., :3], imgs) and (imgs4[..., 3] == 255).all()
