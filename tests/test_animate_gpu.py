"""The animate stage on a copy of the folder a training run left (tests/_train_scene.py: five frames, 128 x 128, the 200-vertex body), as
tests/test_render_cli_gpu.py does: the session's shared result folder is only read.

Training optimises the capture's poses and translations, so "a frame's own pose" is a row of the trained tables, not of the capture's
smpl_rec.npz: the bit-for-bit checks play a motion file that holds the trained tables in smpl_rec.npz's layout, and the command plays
the capture's own smpl_rec.npz as it is.  (The scene's images are noise and its masks an ellipse, so error values mean nothing here:
format and range only.)"""
import json
import os
import re
import shutil

import numpy as np
import pytest
import torch

import _avi
import _train_scene as ts
from _png import read_png
from test_texture_cli_gpu import ARGS as TEXTURE_ARGS

pytestmark = pytest.mark.gpu
QUIET = lambda *a, **k: None


def _tree(root):
    out = {}
    for dp, _, fns in os.walk(root):
        for fn in fns:
            with open(os.path.join(dp, fn), "rb") as fh:
                out[os.path.relpath(os.path.join(dp, fn), root).replace(os.sep, "/")] = fh.read()
    return out


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from selfreconcode_amd.infer import load_network
    from selfreconcode_amd.posed import FULL_RATIO
    capture, first = ts.folder(tmp_path_factory)
    rec_root = os.path.join(os.path.dirname(first.save_root), os.path.basename(first.save_root) + '_animate')
    assert not os.path.exists(rec_root)
    shutil.copytree(first.save_root, rec_root, ignore=shutil.ignore_patterns('template', 'animation'))
    net, ds, _ = load_network(rec_root, ts.DEV, 1, QUIET, ts.PYRAMID)
    verts, faces = net.discretizeSDF(FULL_RATIO, None, 0.)
    trained = str(tmp_path_factory.mktemp("animate_motion") / "trained.npz")
    np.savez(trained, poses=ds.poses.detach().cpu().numpy().reshape(-1, 72), trans=ds.trans.detach().cpu().numpy())
    return {'capture': capture, 'rec_root': rec_root, 'net': net, 'ds': ds, 'verts': verts.detach(), 'faces': faces, 'trained': trained}


@pytest.mark.parametrize("ids", [[2], [0, 4]])
def test_pose_with_own_parameters_is_pose_template(stage, ids):
    from selfreconcode_amd.posed import pose_template, pose_with
    net, ds, verts = stage['net'], stage['ds'], stage['verts']
    fids = torch.tensor(ids, device=ts.DEV)
    want, defconds, _ = pose_template(net, verts, fids)
    poses, trans, d_cond = ds.poses.detach()[fids], ds.trans.detach()[fids], ds.conds[0].detach()[fids]
    got, got_conds = pose_with(net, verts, poses, trans, d_cond)
    assert got.shape == (len(ids), verts.shape[0], 3) and got.is_contiguous() and not got.requires_grad and torch.equal(got, want)
    assert torch.equal(got_conds[0], defconds[0]) and torch.equal(got_conds[1][0], defconds[1][0]) and torch.equal(got_conds[1][1], defconds[1][1])
    assert not torch.equal(pose_with(net, verts, poses, trans, torch.zeros_like(d_cond))[0], want)      # the code matters


def test_animate_reproduces_the_captured_frames(stage):
    from selfreconcode_amd import posecond_ops as po
    from selfreconcode_amd.animate import animate, plan_motion, read_motion
    from selfreconcode_amd.posed import pose_template
    net, ds, verts = stage['net'], stage['ds'], stage['verts']
    assert ds.frame_num == ts.FRAMES
    # the fixture's poses are distinct in pose space: every frame's second neighbour is farther than itself
    _, d2 = po.pose_neighbors(ds.poses.detach(), po.PoseIndex.build(ds.poses.detach()), 2)
    assert bool((d2[:, 0] == 0.).all()) and bool((d2[:, 1] > 0.).all())
    motion = read_motion(stage['trained'])
    assert motion['poses'].tobytes() == ds.poses.detach().cpu().numpy().tobytes()
    want = pose_template(net, verts, torch.arange(ts.FRAMES, device=ts.DEV))[0]
    for cond in ('frames', 'nearest'):
        got = animate(net, verts, motion, cond=cond, sigma=1., batch_size=2)
        assert tuple(got.shape) == (ts.FRAMES, verts.shape[0], 3) and torch.equal(got, want), cond
    info = plan_motion(net, motion, 'nearest', sigma=1.)[3]
    assert info['idx'][:, 0].tolist() == list(range(ts.FRAMES)) and not bool(info['d2'].any()) and bool((info['weights'] == 1.).all())
    # blending and a zero code pose other meshes; the translation policies differ by the translation
    blend = animate(net, verts, motion, cond='blend', K=4, sigma=1.)
    assert bool(torch.isfinite(blend).all()) and not torch.equal(blend, want)
    assert not torch.equal(animate(net, verts, motion, cond='zero'), want)
    anchored = animate(net, verts, motion, cond='frames', trans='anchor')
    shift = ds.trans.detach()[:ts.FRAMES].mean(0)[None, :] - ds.trans.detach()[:ts.FRAMES]
    assert float((anchored - (want + shift[:, None, :])).abs().max()) < 1e-5
    # the capture's own smpl_rec.npz is a motion file as it is; without its translation the anchor is the default
    own = read_motion(os.path.join(stage['capture'], 'smpl_rec.npz'))
    assert own['poses'].shape == (ts.FRAMES, 24, 3) and own['trans'].shape == (ts.FRAMES, 3)
    assert bool(torch.isfinite(animate(net, verts, own, sigma=1.)).all())
    assert torch.equal(animate(net, verts, (motion['poses'], None), cond='frames'), anchored)
    with pytest.raises(ValueError, match="cond='frames'"):
        animate(net, verts, (np.zeros((ts.FRAMES + 1, 24, 3), np.float32), None), cond='frames')
    with pytest.raises(ValueError, match="explicit sigma"):                # five frames lie inside the calibration window
        animate(net, verts, motion, cond='blend')


def _encode_pngs(paths, quality=90):
    from selfreconcode_amd.video import JpegEncoder
    pixels = np.stack([read_png(p) for p in paths])
    return JpegEncoder(pixels.shape[1], pixels.shape[2], quality, ts.DEV).encode(torch.from_numpy(pixels).to(ts.DEV))


def test_animate_command(stage, tmp_path):
    from selfreconcode_amd import animate, texture
    from selfreconcode_amd.mesh_io import read_obj_uv
    capture, rec_root = stage['capture'], stage['rec_root']
    folder = os.path.join(rec_root, 'animation')
    argv = ['--rec-root', rec_root, '--motion', os.path.join(capture, 'smpl_rec.npz'), '--video', '--self-check', '--cond-exclude', '0', '--cond-sigma', '1']

    def run(extra):
        said = []
        assert animate.main(argv + extra, out=lambda *a, **k: said.append(' '.join(str(x) for x in a)), resolutions=ts.PYRAMID) == 0
        return said
    skip = os.path.abspath(folder)
    before = {k: v for k, v in _tree(capture).items() if not os.path.abspath(os.path.join(capture, k)).startswith(skip)}
    said = run(['--shaded'])
    assert len(said) == 1 and said[0].startswith('animation: 5 frames shaded, cond blend (K 4, sigma2 1,') and 'self check over 5 frames' in said[0]
    assert {k: v for k, v in _tree(capture).items() if not os.path.abspath(os.path.join(capture, k)).startswith(skip)} == before
    shaded = _tree(folder)
    frames = range(ts.FRAMES)
    assert sorted(shaded) == sorted([f'{k}.png' for k in frames] + [f'meshs/{k}.npy' for k in frames] + ['video.avi', 'conditioning.json', 'selfcheck.txt'])
    V = stage['verts'].shape[0]
    for k in frames:
        assert read_png(os.path.join(folder, f'{k}.png')).shape == (ts.SIZE, ts.SIZE, 3)
        mesh = np.load(os.path.join(folder, 'meshs', f'{k}.npy'))
        assert mesh.shape == (V, 3) and mesh.dtype == np.float32 and np.isfinite(mesh).all()
    assert shaded['0.png'] != shaded['3.png']
    # the video's frames are the PNGs' pixels
    film = _avi.frames(os.path.join(folder, 'video.avi'))
    assert len(film) == ts.FRAMES and film == _encode_pngs([os.path.join(folder, f'{k}.png') for k in frames])
    record = json.loads(shaded['conditioning.json'])
    assert record['cond'] == 'blend' and record['K'] == 4 and record['sigma2'] == 1. and len(record['frames']) == ts.FRAMES
    for row in record['frames']:
        assert len(set(row['idx'])) == 4 and all(0 <= i < ts.FRAMES for i in row['idx'])
        assert row['d2'] == sorted(row['d2']) and abs(sum(row['weights']) - 1.) < 1e-6
    assert record['max_d2_over_sigma2'] == max(row['d2'][0] for row in record['frames'])
    lines = shaded['selfcheck.txt'].decode().splitlines()
    assert lines[0] == '      mask  blended  dist mean  dist max' and len(lines) == 1 + ts.FRAMES + 2
    for k, line in zip(frames, lines[1:]):
        m = re.fullmatch(r' *(\d+): (\d\.\d{4}) (\d\.\d{4}) (\d+\.\d{6}) (\d+\.\d{6})', line)
        assert m and int(m.group(1)) == k and float(m.group(4)) <= float(m.group(5)) and float(m.group(5)) > 0., line
    assert lines[-2].startswith('blended mask mean: ') and lines[-1].startswith('dist mean mean: ') and 'maxinds:' in lines[-1]
    # two runs write identical bytes
    run(['--shaded'])
    assert _tree(folder) == shaded
    # frame k's own code needs a frame k
    six = str(tmp_path / "six.npz")
    np.savez(six, poses=np.zeros((ts.FRAMES + 1, 72), np.float32))
    with pytest.raises(SystemExit):
        animate.main(['--rec-root', rec_root, '--motion', six, '--cond', 'frames'], out=QUIET, resolutions=ts.PYRAMID)
    assert _tree(folder) == shaded
    # after the texture command the same command draws the textured avatar
    assert texture.main(TEXTURE_ARGS + ['--rec-root', rec_root], out=QUIET, resolutions=ts.PYRAMID) == 0
    said = run([])
    assert len(said) == 1 and said[0].startswith('animation: 5 frames textured, cond blend')
    textured = _tree(folder)
    assert sorted(textured) == sorted(shaded) and all(textured[f'{k}.png'] != shaded[f'{k}.png'] for k in frames)
    Vt = read_obj_uv(os.path.join(rec_root, 'template', 'uvmap.obj'))[0].shape[0]
    assert np.load(os.path.join(folder, 'meshs', '0.npy')).shape == (Vt, 3)
    film = _avi.frames(os.path.join(folder, 'video.avi'))
    assert film == _encode_pngs([os.path.join(folder, f'{k}.png') for k in frames])
    assert textured['conditioning.json'] == shaded['conditioning.json']
