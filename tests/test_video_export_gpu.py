"""The videos of the export loops and the commands: `video=True` adds video.avi files whose frames are, exactly, JpegEncoder.encode of
the pixels the PNGs hold, in the order visited, and changes nothing else; `images=False` leaves the PNGs out.  export_frames runs on
the synthetic scene of tests/test_infer_export_gpu.py; the commands run on a copy of the folder a training run left
(tests/_train_scene.py), as tests/test_render_cli_gpu.py does: the session's shared result folder is only read."""
import os
import shutil

import numpy as np
import pytest
import torch

import _avi
import _train_scene as ts
from _png import read_png
from test_texture_cli_gpu import ARGS as TEXTURE_ARGS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIO = {'sdfRatio': 1., 'deformerRatio': 0.62, 'renderRatio': 1.}
H = W = 64
QUALITY = 85


def _tree(root):
    out = {}
    for dp, _, fns in os.walk(root):
        for fn in fns:
            with open(os.path.join(dp, fn), "rb") as fh:
                out[os.path.relpath(os.path.join(dp, fn), root).replace(os.sep, "/")] = fh.read()
    return out


def _encode_pngs(paths, quality):
    from selfreconcode_amd.video import JpegEncoder
    pixels = np.stack([read_png(p) for p in paths])
    return JpegEncoder(pixels.shape[1], pixels.shape[2], quality, DEV).encode(torch.from_numpy(pixels).to(DEV))


def test_export_frames_video(tmp_path):
    from selfreconcode_amd.infer_export import export_frames
    from selfreconcode_amd.synthetic import build_synthetic_scene
    torch.manual_seed(0)
    net, ds, conf = build_synthetic_scene(device=DEV, frame_num=12, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)],
                                          lbs_volume_shape=(17, 57, 33), consistent_masks=False)
    net.point_radius = 0.03
    verts, faces = net.discretizeSDF(RATIO, None, 0.0)
    groups = [torch.tensor([2, 5]), torch.tensor([9, 0])]
    fids = [2, 5, 9, 0]
    batches = [(g, {k: v.cpu() for k, v in ds.batch(g.to(DEV)).items()}) for g in groups]
    roots = {name: str(tmp_path / name) for name in ("plain", "video", "noimages")}
    export_frames(net, verts, faces, batches, roots["plain"], RATIO, color=True)
    export_frames(net, verts, faces, batches, roots["video"], RATIO, color=True, video=True, fps=12., quality=QUALITY)
    export_frames(net, verts, faces, batches, roots["noimages"], RATIO, color=True, video=True, images=False, fps=12., quality=QUALITY)
    plain, video, noimages = (_tree(roots[k]) for k in ("plain", "video", "noimages"))
    avis = [f"{sub}/video.avi" for sub in ("meshs", "def1meshs", "colors")]
    assert sorted(set(video) - set(plain)) == sorted(avis) and not [k for k in plain if plain[k] != video[k]]
    for sub in ("meshs", "def1meshs", "colors"):
        frames = _avi.frames(os.path.join(roots["video"], sub, "video.avi"))
        assert frames == _encode_pngs([os.path.join(roots["video"], sub, f"{f}.png") for f in fids], QUALITY)
    assert sorted(noimages) == sorted(avis + [f"meshs/{f}.npy" for f in fids] + ["tmp.ply", "errors.txt"])
    assert not [k for k in noimages if noimages[k] != video[k]]


def test_commands_with_video(tmp_path_factory):
    from selfreconcode_amd import infer, render, texture
    capture, first = ts.folder(tmp_path_factory)
    rec_root = os.path.join(os.path.dirname(first.save_root), os.path.basename(first.save_root) + '_video')
    assert not os.path.exists(rec_root)
    shutil.copytree(first.save_root, rec_root, ignore=shutil.ignore_patterns('template', 'textured', 'turntable', 'meshs', 'def1meshs', 'colors'))
    visited = (0, 1, 2)                                                     # --frames 2 at batch size 1

    def run(main, argv):
        said = []
        assert main(['--rec-root', rec_root] + argv, out=lambda *a, **k: said.append(' '.join(str(x) for x in a)), resolutions=ts.PYRAMID) == 0
        return said
    # infer: --video adds exactly the two .avi files and drops the "not written" line
    said = run(infer.main, ['--frames', '2', '--nColor'])
    assert sum('not written' in s for s in said) == 1
    before = _tree(rec_root)
    said = run(infer.main, ['--frames', '2', '--nColor', '--video', '--video-quality', str(QUALITY)])
    assert not any('not written' in s for s in said)
    after = _tree(rec_root)
    assert sorted(set(after) - set(before)) == ['def1meshs/video.avi', 'meshs/video.avi'] and not [k for k in before if before[k] != after[k]]
    for sub in ('meshs', 'def1meshs'):
        assert _avi.frames(os.path.join(rec_root, sub, 'video.avi')) == _encode_pngs([os.path.join(rec_root, sub, f'{i}.png') for i in visited], QUALITY)
    # --nI: no PNG
    for sub in ('meshs', 'def1meshs', 'colors'):
        shutil.rmtree(os.path.join(rec_root, sub))
    run(infer.main, ['--frames', '2', '--nColor', '--video', '--video-quality', str(QUALITY), '--nI'])
    left = _tree(rec_root)
    assert not [k for k in left if k.endswith('.png')]
    assert sorted(k for k in left if k.split('/')[0] in ('meshs', 'def1meshs', 'colors')) == sorted(
        ['meshs/video.avi', 'def1meshs/video.avi'] + [f'meshs/{i}.npy' for i in visited])
    assert all(left[k] == after[k] for k in ('meshs/video.avi', 'def1meshs/video.avi', 'errors.txt', 'tmp.ply'))
    # render: textured/video.avi and a turntable of 4 views
    assert texture.main(TEXTURE_ARGS + ['--rec-root', rec_root], out=lambda *a, **k: None, resolutions=ts.PYRAMID) == 0
    run(render.main, ['--frames', '2', '--turntable', '4', '--video', '--video-quality', str(QUALITY)])
    after = _tree(rec_root)
    assert sorted(k for k in after if k.split('/')[0] in ('textured', 'turntable')) == sorted(
        [f'textured/{i}.png' for i in visited] + ['textured/errors.txt', 'textured/video.avi', 'turntable/video.avi'] + [f'turntable/{k}.png' for k in range(4)])
    textured = _avi.frames(os.path.join(rec_root, 'textured', 'video.avi'))
    turntable = _avi.frames(os.path.join(rec_root, 'turntable', 'video.avi'))
    assert textured == _encode_pngs([os.path.join(rec_root, 'textured', f'{i}.png') for i in visited], QUALITY)
    assert turntable == _encode_pngs([os.path.join(rec_root, 'turntable', f'{k}.png') for k in range(4)], QUALITY)
    assert len(turntable) == 4 and turntable[0] == textured[0] and turntable[2] != turntable[0]
