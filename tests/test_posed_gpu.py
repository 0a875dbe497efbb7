"""selfreconcode_amd/posed.py on the smallest synthetic scene: pose_template and rasterize_posed against the calls they stand for,
written out here as the stages used to write them."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIO = {'sdfRatio': 1., 'deformerRatio': 0.62, 'renderRatio': 1.}
H = W = 64


@pytest.fixture(scope="module")
def scene():
    from selfreconcode_amd.synthetic import build_synthetic_scene
    torch.manual_seed(0)
    net, ds, _ = build_synthetic_scene(device=DEV, frame_num=12, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)],
                                       lbs_volume_shape=(9, 29, 17), consistent_masks=False)
    verts, faces = net.discretizeSDF(RATIO, None, 0.0)
    return net, ds, verts.detach(), faces


@pytest.mark.parametrize("ids", [[7], [3, 11]])
def test_pose_template_is_the_deformer_call(scene, ids):
    from selfreconcode_amd.posed import FULL_RATIO, pose_template
    net, ds, verts, _ = scene
    fids = torch.tensor(ids, device=DEV)
    N = fids.numel()
    for ratio, used in ((RATIO, RATIO), (None, FULL_RATIO)):
        with torch.no_grad():
            poses, trans, d_cond, rendcond = [t.detach() for t in ds.get_grad_parameters(fids, fids.device)]
            want = net.deformer(verts[None, :, :].expand(N, -1, 3), [d_cond, [poses, trans]], ratio=used)
        got, defconds, got_rendcond = pose_template(net, verts, fids, ratio)
        assert got.shape == (N, verts.shape[0], 3) and got.is_contiguous() and not got.requires_grad
        assert torch.equal(got, want)
        assert torch.equal(defconds[0], d_cond) and torch.equal(defconds[1][0], poses) and torch.equal(defconds[1][1], trans)
        assert torch.equal(got_rendcond, rendcond)
    if N == 2:                                                       # the frames differ, so a per-frame indexing slip would show
        assert not torch.equal(want[0], want[1])


def test_rasterize_posed_is_project_rasterize_project(scene):
    from selfreconcode_amd.ops import rasterize_meshes
    from selfreconcode_amd.posed import pose_template, rasterize_posed
    net, _, verts, faces = scene
    fids = torch.tensor([3, 11], device=DEV)
    cameras, h, w = net._cameras(2, torch.device(DEV))
    defV = pose_template(net, verts, fids, RATIO)[0]
    with torch.no_grad():
        xy_ndc, z = cameras.project_ndc(defV)
        want = rasterize_meshes(xy_ndc, z, faces, h, w)
        want_pix, _ = cameras.project(defV)
    frags, xy_pix = rasterize_posed(defV, faces, cameras, h, w, pixels=True)
    assert int((want.pix_to_face >= 0).sum()) > 0
    assert torch.equal(frags.pix_to_face, want.pix_to_face) and torch.equal(frags.bary_coords, want.bary_coords)
    assert torch.equal(xy_pix, want_pix)
    frags0, none = rasterize_posed(defV, faces, cameras, h, w)
    assert none is None and torch.equal(frags0.pix_to_face, want.pix_to_face) and torch.equal(frags0.bary_coords, want.bary_coords)
