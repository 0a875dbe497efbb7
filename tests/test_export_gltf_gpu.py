"""The export stage on a copy of the folder a training run left (tests/_train_scene.py: five frames, 128 x 128, the 200-vertex body), as
tests/test_animate_gpu.py does: the session's shared result folder is only read.  (The scene's images are noise, so distances mean
nothing as quality here: structure, and the inequality the fit guarantees.)"""
import json
import os
import re
import shutil

import numpy as np
import pytest
import torch

import _train_scene as ts
from test_animate_gpu import _tree
from test_texture_cli_gpu import ARGS as TEXTURE_ARGS

pytestmark = pytest.mark.gpu
QUIET = lambda *a, **k: None


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    from selfreconcode_amd.infer import load_network
    from selfreconcode_amd.posed import FULL_RATIO
    capture, first = ts.folder(tmp_path_factory)
    rec_root = os.path.join(os.path.dirname(first.save_root), os.path.basename(first.save_root) + '_export')
    assert not os.path.exists(rec_root)
    shutil.copytree(first.save_root, rec_root, ignore=shutil.ignore_patterns('template', 'animation', 'export'))
    net, ds, _ = load_network(rec_root, ts.DEV, 1, QUIET, ts.PYRAMID)
    verts, faces = net.discretizeSDF(FULL_RATIO, None, 0.)
    return {'capture': capture, 'rec_root': rec_root, 'net': net, 'ds': ds, 'verts': verts.detach(), 'faces': faces}


def test_two_step_evaluation_is_pose_with(stage):
    from selfreconcode_amd.animate import training_tables
    from selfreconcode_amd.export_gltf import evaluate_deformer
    from selfreconcode_amd.posed import pose_with
    net, verts = stage['net'], stage['verts']
    poses, trans, codes = training_tables(net)
    for ids in ([2], [0, 4], list(range(ts.FRAMES))):
        q, y, A = evaluate_deformer(net, verts, poses[ids], trans[ids], codes[ids])
        assert torch.equal(y, pose_with(net, verts, poses[ids], trans[ids], codes[ids])[0])
        assert q.shape == y.shape == (len(ids), verts.shape[0], 3) and A.shape == (len(ids), 24, 4, 4) and not torch.equal(q, y)
        assert not torch.equal(q, verts[None].expand_as(q))                      # the translator moves the points


def test_fit_skin_on_the_trained_avatar(stage):
    from selfreconcode_amd import skinfit_ops as so
    from selfreconcode_amd.export_gltf import evaluate_deformer, fit_morphs, fit_skin
    from selfreconcode_amd.animate import training_tables
    net, verts = stage['net'], stage['verts']
    V = verts.shape[0]
    fit = fit_skin(net, verts, K=4, batch_size=2)
    poses, trans, codes = training_tables(net)
    q = evaluate_deformer(net, verts, poses, trans, codes)[0]
    # the rest shape: the mean of q_t, summed in float64 in ascending frame order and rounded once
    total = torch.zeros((V, 3), dtype=torch.float64, device=ts.DEV)
    for t in range(ts.FRAMES):
        total += q[t].double()
    assert torch.equal(fit['rest'], (total / ts.FRAMES).float()) and torch.equal(fit['q'], q) and fit['frames'] == list(range(ts.FRAMES))
    assert fit['joints'].shape == fit['weights'].shape == (V, 4) and fit['cands'].shape == (V, 8)
    assert bool((fit['cands'].sort(1)[0][:, 1:] != fit['cands'].sort(1)[0][:, :-1]).all())       # distinct candidates
    assert bool(((fit['weights'].sum(1) - 1.).abs() <= 2. ** -22).all())
    # the composed path fits the same skin (five frames: the objective, to rounding)
    other = fit_skin(net, verts, K=4, batch_size=5, method="composed")
    assert torch.allclose(other['objective'], fit['objective'], rtol=1e-7, atol=1e-30)
    # never worse than the naive weights where their support lies inside the candidates
    inside = (fit['naive_joints'][:, :, None] == fit['cands'][:, None, :]).any(2) | (fit['naive_weights'] == 0.)
    inside = inside.all(1)
    assert float(inside.float().mean()) > 0.9
    x = so.scatter_weights(torch.where(inside[:, None], fit['naive_joints'], fit['joints']),
                           torch.where(inside[:, None], fit['naive_weights'], fit['weights']), fit['cands'])       # (the others: the fit's own)
    naive = so.objective_of(fit['H'], fit['xbar'], fit['lambda'], x)
    assert bool((fit['objective'] <= naive * (1. + 1e-6) + 1e-30).all())             # (1e-6: the float32 rounding of the weights compared)
    # frames evenly strided, and K = 8 writes eight columns
    three = fit_skin(net, verts, K=8, fit_frames=3)
    assert three['frames'] == [0, 1, 3] and three['weights'].shape == (V, 8)
    # T - 1 directions span the residual of T frames about their mean; the rest shape is that mean rounded to float32, and the
    # rounding, the same in every frame, is the one direction left over: at most T 3V (2^-24 max |r|)^2 of |D|^2
    morph = fit_morphs(fit['q'], fit['rest'], ts.FRAMES - 1)
    left = ts.FRAMES * 3 * V * (2. ** -24 * float(fit['rest'].abs().max())) ** 2
    print("morphs: kept %.9f of |D|^2 = %.3g; the rest shape's rounding may take %.3g of it" % (morph['kept'], morph['energy'], left / morph['energy']))
    assert -1e-12 <= 1. - morph['kept'] <= left / morph['energy'] + 1e-12


def _main(argv):
    from selfreconcode_amd import export_gltf
    said = []
    assert export_gltf.main(argv, out=lambda *a, **k: said.append(' '.join(str(x) for x in a)), resolutions=ts.PYRAMID) == 0
    return said


def _outside(root, skip):
    skip = os.path.abspath(skip)
    return {k: v for k, v in _tree(root).items() if not os.path.abspath(os.path.join(root, k)).startswith(skip)}


def test_export_command(stage, tmp_path):
    from selfreconcode_amd import gltf, texture
    from selfreconcode_amd.animate import animate, read_motion
    from selfreconcode_amd.export_gltf import fit_skin
    from selfreconcode_amd.mesh_io import read_obj_uv
    capture, rec_root, net, verts = stage['capture'], stage['rec_root'], stage['net'], stage['verts']
    folder = os.path.join(rec_root, 'export')
    before = _outside(capture, folder)
    # untextured: the extracted template, the capture's own frames
    said = _main(['--rec-root', rec_root, '--morphs', str(ts.FRAMES - 1), '--self-check', '--batch-size', '2'])
    assert len(said) == 1 and said[0].startswith('export: %d vertices (%d in the file) untextured, 5 frames, K 4, 4 morphs' % (verts.shape[0], verts.shape[0]))
    assert _outside(capture, folder) == before
    assert sorted(os.listdir(folder)) == ['avatar.glb', 'export.json', 'selfcheck.txt']
    glb = gltf.validate_glb(os.path.join(folder, 'avatar.glb'))
    doc = glb['json']
    prim = doc['meshes'][0]['primitives'][0]
    assert 'TEXCOORD_0' not in prim['attributes'] and 'images' not in doc and len(prim['targets']) == ts.FRAMES - 1
    assert len(doc['skins'][0]['joints']) == 24 and len(doc['animations'][0]['channels']) == 26
    skinner = net.deformer.defs[1]
    ibm = glb['accessors'][doc['skins'][0]['inverseBindMatrices']].reshape(24, 4, 4).transpose(0, 2, 1)
    assert np.array_equal(ibm, skinner.init_pose.cpu().numpy())
    for i in range(1, 24):
        assert i in doc['nodes'][skinner.parents[i]]['children']
    record = json.load(open(os.path.join(folder, 'export.json')))
    assert record['frames'] == ts.FRAMES and record['fit_frames'] == ts.FRAMES and record['K'] == 4 and record['B'] == ts.FRAMES - 1
    rest = glb['accessors'][prim['attributes']['POSITION']]
    left = ts.FRAMES * 3 * len(rest) * (2. ** -24 * float(np.abs(rest).max())) ** 2        # (the rest shape's rounding: test_fit_skin_on_the_trained_avatar)
    assert -1e-12 <= 1. - record['kept_variance'] <= left / record['cloth_energy'] + 1e-12
    assert sum(record['influences_used'].values()) == verts.shape[0] and len(record['joint_use']) == 24
    assert record['lambda']['min'] > 0. and not record['textured']
    lines = open(os.path.join(folder, 'selfcheck.txt')).read().splitlines()
    assert lines[0].split() == ['naive', 'mean', 'naive', 'max', 'fitted', 'mean', 'fitted', 'max', 'written', 'mean', 'written', 'max']
    assert len(lines) == 1 + ts.FRAMES + 3 and [ln.split()[0] for ln in lines[-3:]] == ['naive', 'fitted', 'written']
    for k, line in enumerate(lines[1:1 + ts.FRAMES]):
        m = re.fullmatch(r' *(\d+):' + r' (\d+\.\d{6})' * 6, line)
        assert m and int(m.group(1)) == k and all(float(m.group(2 + 2 * i)) <= float(m.group(3 + 2 * i)) for i in range(3)), line
    # The file against animate's meshes of the same frames.  With T - 1 morphs the cloth motion is spanned exactly, so what is left is
    # the skin: per vertex the fit guarantees x^T H x + lambda |x - xbar|^2 <= the same of the naive weights wherever their support
    # lies inside the candidates, hence residual_fit <= residual_naive + lambda |naive - xbar|^2 <= residual_naive + 2 lambda, and
    # lambda = reg trace(H) / C + floor.  Summed: S_fit <= S_naive (1 + margin), margin = 2 reg sum_v trace(H_v) / (C S_naive) (+ the floor),
    # with reg = 1e-6.  The file's float32 storage adds at most (2 D + 8) 2^-24 E per vertex distance (tests/test_gltf_cpu.py), E <= 8 m
    # here, which enters through the triangle inequality on the root of the sums.
    trained = str(tmp_path / "trained.npz")
    np.savez(trained, poses=stage['ds'].poses.detach().cpu().numpy().reshape(-1, 72), trans=stage['ds'].trans.detach().cpu().numpy())
    want = animate(net, verts, read_motion(trained), cond='frames', batch_size=2).double().cpu().numpy()
    fit = fit_skin(net, verts, K=4, batch_size=2)
    inside = ((fit['naive_joints'][:, :, None] == fit['cands'][:, None, :]).any(2) | (fit['naive_weights'] == 0.)).all(1).cpu().numpy()
    written = ((gltf.replay_glb(glb) - want) ** 2).sum(-1)[:, inside].sum()
    naive = ((gltf.replay_glb(glb, joints_weights=(fit['naive_joints'].cpu().numpy(), fit['naive_weights'].cpu().numpy())) - want) ** 2).sum(-1)[:, inside].sum()
    trace = sum(fit['H'][k * (k + 1) // 2 + k] for k in range(8)).cpu().numpy()[inside].sum()
    margin = 2. * (1e-6 * trace / 8. + 1e-24 * inside.sum()) / naive
    storage = 26. * 2. ** -24 * 8. * np.sqrt(ts.FRAMES * inside.sum())
    print("export: summed squared distance %.6g as written, %.6g with the naive weights (%d of %d vertices), margin %.3g, storage %.3g"
          % (written, naive, inside.sum(), len(inside), margin, storage))
    assert inside.mean() > 0.9
    assert np.sqrt(written) <= np.sqrt(naive * (1. + margin)) + 2. * storage
    # a motion file: the clip has the motion's frames (here four of the capture's own smpl_rec.npz)
    out = str(tmp_path / "motion.glb")
    said = _main(['--rec-root', rec_root, '--motion', os.path.join(capture, 'smpl_rec.npz'), '--cond-sigma', '1', '--frames', '4', '--morphs', '2', '--out', out,
                  '--influences', '6', '--fps-in', '15'])
    clip = gltf.validate_glb(out)
    anim = clip['json']['animations'][0]
    assert np.array_equal(clip['accessors'][anim['samplers'][0]['input']][:, 0], (np.arange(4) / 15.).astype(np.float32))
    assert 'JOINTS_1' in clip['json']['meshes'][0]['primitives'][0]['attributes'] and gltf.replay_glb(clip).shape == (4, verts.shape[0], 3)
    assert sorted(os.listdir(folder)) == ['avatar.glb', 'export.json', 'selfcheck.txt'] and json.load(open(os.path.join(folder, 'export.json')))['frames'] == 4
    full = read_motion(os.path.join(capture, 'smpl_rec.npz'))['poses'].shape[0]
    _main(['--rec-root', rec_root, '--motion', os.path.join(capture, 'smpl_rec.npz'), '--cond-sigma', '1', '--morphs', '0', '--out', out])
    assert gltf.replay_glb(gltf.validate_glb(out)).shape[0] == full
    # after the texture command the same command writes the textured avatar, split at the seams
    assert texture.main(TEXTURE_ARGS + ['--rec-root', rec_root], out=QUIET, resolutions=ts.PYRAMID) == 0
    before = _outside(rec_root, folder)
    said = _main(['--rec-root', rec_root, '--morphs', '2'])
    assert ' textured, 5 frames' in said[0] and _outside(rec_root, folder) == before
    tex = gltf.validate_glb(os.path.join(folder, 'avatar.glb'))
    v, f, vt, ft = read_obj_uv(os.path.join(rec_root, 'template', 'uvmap.obj'))
    tprim = tex['json']['meshes'][0]['primitives'][0]
    uv = tex['accessors'][tprim['attributes']['TEXCOORD_0']]
    faces = tex['accessors'][tprim['indices']].reshape(-1, 3)
    assert len(uv) >= len(v) and faces.shape == f.shape and np.array_equal(uv[faces], gltf.gltf_uv(vt[ft]))
    image = tex['json']['bufferViews'][tex['json']['images'][0]['bufferView']]
    with open(os.path.join(rec_root, 'template', 'texture.png'), 'rb') as fh:
        assert tex['bin'][image['byteOffset']:image['byteOffset'] + image['byteLength']] == fh.read()
    assert tex['json']['materials'][0]['pbrMetallicRoughness']['baseColorTexture'] == {'index': 0}
    assert 'selfcheck.txt' in os.listdir(folder)                                 # (the earlier run's: this one did not ask for a check)
