"""The training driver on a miniature capture folder (tests/_train_scene.py): the files and rows of a run over all three stages, the
device-side log against the blocking one, a resumed run against the straight one bit for bit, and --model without --resume."""
import copy
import os

import numpy as np
import pytest
import torch

import _train_scene as ts

pytestmark = pytest.mark.gpu
REFERENCE_KEYS = {'epoch', 'model_state_dict', 'focal_length', 'princeple_points', 'cam2world_coord_quat', 'world2cam_coord_trans',
                  'poses', 'trans', 'shape', 'dcond', 'rcond'}
ITERS = (3, 3, 5)                      # len(loader) of the three epochs: five frames in batches of 2, 2 and 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_checkpoints(a, b, skip=()):
    ta, ea = ts.checkpoint_tensors(a)
    tb, eb = ts.checkpoint_tensors(b)
    assert ea == eb and set(ta) == set(tb)
    return [k for k in ta if not any(s in k for s in skip) and not (ta[k].dtype == tb[k].dtype and torch.equal(ta[k], tb[k]))]


def test_files_and_rows(tmp_path_factory):
    from selfreconcode_amd.config import load_config
    from selfreconcode_amd.train import LOG_COLUMNS, deformer_ratio
    root, first = ts.folder(tmp_path_factory)
    conf = ts.train_conf()
    assert load_config(os.path.join(first.save_root, 'config.conf')) == conf
    for name in ('coarse.pth', 'medium.pth', 'latest.pth'):
        saved = torch.load(os.path.join(first.save_root, name), map_location='cpu', weights_only=False)
        assert set(saved) == REFERENCE_KEYS, name
        assert any(k.startswith('sdf.lin0.') for k in saved['model_state_dict']) and any(k.startswith('deformer.defs.0.') for k in saved['model_state_dict'])
    assert [torch.load(os.path.join(first.save_root, n), map_location='cpu', weights_only=False)['epoch'] for n in ('coarse.pth', 'medium.pth', 'latest.pth')] == [1, 2, 2]
    assert os.path.isfile(os.path.join(first.save_root, 'latest.state.pth')) and os.path.isdir(os.path.join(first.save_root, 'debug'))
    for name in ('initial_sdf_idr_6_1.ply', 'initial_sdf_idr_6_1.pth', 'initial_skinner_1.pth'):
        assert os.path.isfile(os.path.join(root, name)), name
    with open(os.path.join(root, 'initial_sdf_idr_6_1.ply')) as fh:
        assert fh.readline().strip() == 'ply'

    col = {n: i for i, n in enumerate(LOG_COLUMNS)}
    rows = first.rows
    assert rows.shape == (sum(ITERS), len(LOG_COLUMNS)) and rows.dtype == np.float32 and len(first.lines) == sum(ITERS)
    assert rows[:, col['epoch']].tolist() == [e for e, n in enumerate(ITERS) for _ in range(n)]
    assert rows[:, col['data_index']].tolist() == [i for n in ITERS for i in range(n)]
    for name in ('loss', 'color_loss', 'grad_loss', 'normal_loss', 'def_loss', 'offset_loss', 'pc_loss_sdf', 'mask_loss', 'defconst_loss'):
        assert np.isfinite(rows[:, col[name]]).all(), name
    assert np.isnan(rows[:, col['dct_loss']]).all() and np.isnan(rows[:, col['pc_loss_norm']]).all()      # terms this configuration does not compute
    assert (rows[:, col['ray_num']] > 0).all() and (rows[:, col['ray_converged']] <= rows[:, col['ray_num']]).all()
    assert (rows[:, col['inv_ok']] <= rows[:, col['inv_num']]).all()
    # closed forms: the three ratios, the learning rate of MultiStepLR([1], 0.333) and the remesh clock
    assert np.array_equal(_bits(rows[:, col['deformerRatio']]), _bits([np.float32(deformer_ratio(float(k))) for k in range(sum(ITERS))]))
    assert (rows[:, col['sdfRatio']] == 1.).all() and (rows[:, col['renderRatio']] == 1.).all()
    lr0 = conf.get_float('train.learning_rate')
    want_lr = [np.float32(lr0)] * ITERS[0] + [np.float32(lr0 * 0.333)] * (ITERS[1] + ITERS[2])
    assert np.array_equal(_bits(rows[:, col['lr']]), _bits(want_lr))
    assert first.net_state['point_radius'] == conf.get_float('train.fine.point_render.radius')
    assert first.net_state['remesh_intersect'] == 2 and first.net_state['draw'] is True
    assert first.net_state['stage_conf'] == dict(conf.get_config('loss_fine'))
    assert any(line == 'enable medium hierarchical' for line in first.text) and any(line == 'enable fine hierarchical' for line in first.text)


def test_log_modes_agree(tmp_path_factory):
    """The rows the log kernel gathered and the rows read value by value through .item(), from the same seeds."""
    ts.folder(tmp_path_factory)
    a = ts.run(tmp_path_factory, 'straight_a')
    item = ts.run(tmp_path_factory, 'item', log='item')
    assert a.rows.shape == item.rows.shape == (sum(ITERS), a.rows.shape[1])
    assert np.array_equal(_bits(a.rows), _bits(item.rows))
    assert a.lines == item.lines and a.text == item.text
    off = ts.run(tmp_path_factory, 'off', log='off', stop_after_epoch=0)
    assert off.rows.shape[0] == 0 and off.text == []


def test_resume_is_exact(tmp_path_factory):
    ts.folder(tmp_path_factory)
    a = ts.run(tmp_path_factory, 'straight_a')
    a2 = ts.run(tmp_path_factory, 'straight_b')
    # the premise: the same seeds give the same run.  If THIS fails the step is not reproducible and nothing below is about resume.
    assert np.array_equal(_bits(a.rows), _bits(a2.rows)), "two straight runs from the same seeds differ: not a resume bug"
    differing = _same_checkpoints(os.path.join(a.save_root, 'latest.pth'), os.path.join(a2.save_root, 'latest.pth'))
    assert not differing, f"two straight runs from the same seeds differ in {differing}: not a resume bug"

    b0 = ts.run(tmp_path_factory, 'resumed_head', save_folder='resumed', stop_after_epoch=0)
    assert b0.next_epoch == 1 and np.array_equal(_bits(b0.rows), _bits(a.rows[:ITERS[0]]))
    b1 = ts.run(tmp_path_factory, 'resumed_tail', save_folder='resumed', resume=True)          # a freshly built dataset and network
    assert any(line.startswith('resume at epoch 1 ') for line in b1.text)
    assert b1.rows.shape[0] == ITERS[1] + ITERS[2]
    assert np.array_equal(_bits(b1.rows), _bits(a.rows[ITERS[0]:]))
    assert b1.lines == a.lines[ITERS[0]:]
    for name in ('coarse.pth', 'medium.pth', 'latest.pth'):
        assert not _same_checkpoints(os.path.join(a.save_root, name), os.path.join(b1.save_root, name)), name


def test_model_without_resume_restarts_at_the_loaded_weights(tmp_path_factory):
    from selfreconcode_amd.train import LOG_COLUMNS
    ts.folder(tmp_path_factory)
    a = ts.run(tmp_path_factory, 'straight_a')
    conf = ts.train_conf()
    conf['train']['learning_rate'] = 0.                             # Adam then moves nothing: the checkpoint shows what was loaded
    m = ts.run(tmp_path_factory, 'from_model', conf=conf, model=os.path.join(a.save_root, 'latest.pth'), stop_after_epoch=0)
    col = {n: i for i, n in enumerate(LOG_COLUMNS)}
    assert m.rows.shape[0] == ITERS[0] and m.rows[:, col['epoch']].tolist() == [0.] * ITERS[0]
    assert m.rows[0, col['deformerRatio']] == 0.5 and m.next_epoch == 1
    assert any(line.startswith('load model: ') for line in m.text) and not any(line.startswith('resume') for line in m.text)
    ta, _ = ts.checkpoint_tensors(os.path.join(a.save_root, 'latest.pth'))
    tm, epoch = ts.checkpoint_tensors(os.path.join(m.save_root, 'latest.pth'))
    assert epoch == 0 and set(ta) == set(tm)
    moved = [k for k in ta if 'engine.' not in k and not torch.equal(ta[k], tm[k])]         # (the engine's buffers are the stage's pyramid)
    assert not moved, moved
    assert m.net_state['point_radius'] == conf.get_float('train.coarse.point_render.radius')
    assert not np.array_equal(_bits(m.rows[:, col['loss']]), _bits(a.rows[:ITERS[0], col['loss']]))     # not the fresh network's losses
