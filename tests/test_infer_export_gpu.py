"""export_frames (selfreconcode_amd/infer_export.py): the reference's infer.py loop on the synthetic scene -- the files it writes
hold exactly what OptimNetwork.infer returns, in the channel order cv2.imwrite would have written."""
import os

import numpy as np
import pytest
import torch

from _png import read_png

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIO = {'sdfRatio': 1., 'deformerRatio': 0.62, 'renderRatio': 1.}
H = W = 64


def test_export_frames_writes_what_infer_returns(tmp_path):
    from selfreconcode_amd.infer_export import export_frames
    from selfreconcode_amd.synthetic import build_synthetic_scene
    torch.manual_seed(0)
    net, ds, conf = build_synthetic_scene(device=DEV, frame_num=12, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)],
                                          lbs_volume_shape=(17, 57, 33), consistent_masks=False)
    net.point_radius = 0.03
    verts, faces = net.discretizeSDF(RATIO, None, 0.0)
    groups = [torch.tensor([2, 5]), torch.tensor([9, 0])]
    batches = [(g, {k: v.cpu() for k, v in ds.batch(g.to(DEV)).items()}) for g in groups]
    root = str(tmp_path / "rec")
    maskE = export_frames(net, verts, faces, batches, root, RATIO, color=True, overlay=True)
    assert net.shaded_previews is False                                   # restored
    assert sorted(os.listdir(root)) == ["colors", "def1meshs", "errors.txt", "meshs", "tmp.ply"]
    fids = [2, 5, 9, 0]
    assert sorted(os.listdir(os.path.join(root, "meshs"))) == sorted([f"{f}.npy" for f in fids] + [f"{f}.png" for f in fids])
    assert sorted(os.listdir(os.path.join(root, "def1meshs"))) == sorted(f"{f}.png" for f in fids)
    assert sorted(os.listdir(os.path.join(root, "colors"))) == sorted(f"{f}.png" for f in fids)
    net.shaded_previews = True
    expect = {}
    for g, outs in batches:
        gts = {'mask': outs['mask'].to(DEV), 'image': (outs['img'].to(DEV) + 1.) / 2.}
        colors, imgs, def1imgs, defVs = net.infer(verts, faces, H, W, RATIO, g.to(DEV), False, gts)
        for i, f in enumerate(g.tolist()):
            expect[f] = (colors[i], imgs[i], def1imgs[i], defVs[i], gts['maskE'][i])
    for f, (color, img, def1img, defV, e) in expect.items():
        npy = np.load(os.path.join(root, "meshs", f"{f}.npy"))
        assert npy.dtype == np.float32 and np.array_equal(npy, defV)
        assert np.array_equal(read_png(os.path.join(root, "meshs", f"{f}.png")), img[:, :, :3])
        assert np.array_equal(read_png(os.path.join(root, "def1meshs", f"{f}.png")), def1img[:, :, :3])
        assert np.array_equal(read_png(os.path.join(root, "colors", f"{f}.png")), color[:, :, ::-1])
        assert maskE[f] == e
    lines = open(os.path.join(root, "errors.txt")).read().split("\n")
    assert lines[0] == "      mask" and lines[-1].startswith("mask mean: ")
    rows = dict((int(a), float(b)) for a, b in (ln.split(":") for ln in lines[1:-1]))
    assert sorted(rows) == sorted(fids) and all(rows[f] == float("%.4f" % expect[f][4]) for f in fids)
    assert (maskE[[1, 3, 4, 6, 7, 8, 10, 11]] == -1).all()
    ply = open(os.path.join(root, "tmp.ply")).read().split("\n")
    assert f"element vertex {verts.shape[0]}" in ply and f"element face {faces.shape[0]}" in ply
