"""The host half of the train / infer drivers, without a GPU: configuration text, the argument parsers, the stage schedule, the log line
against the reference's own expression, and the key set of the resume sidecar."""
import copy

import numpy as np
import pytest
import torch


def test_dump_hocon_round_trip():
    from selfreconcode_amd.config import Conf, default_config, dump_hocon, loose_config, parse_hocon
    for conf in (default_config(), loose_config()):
        text = dump_hocon(conf)
        back = parse_hocon(text)
        assert back == conf and isinstance(back.get_config('train.opt_camera'), Conf)
        assert back.get_list('train.scheduler.milestones') == conf.get_list('train.scheduler.milestones')
        assert type(back.get('train.nepoch')) is int and type(back.get('train.learning_rate')) is float and back.get('train.shuffle') is True
        assert dump_hocon(back) == text
    odd = Conf(a=Conf(), names=["x", "y"], s="MultiStepLR", empty=[], tiny=1e-05, neg=-10., t=(1, 2), deep=Conf(b=Conf(c=False)))
    back = parse_hocon(dump_hocon(odd))
    assert back == dict(odd, t=[1, 2]) and back['deep']['b']['c'] is False
    for bad in (Conf(s="true"), Conf(s="12"), Conf(s='say "hi"'), Conf(**{"a b": 1}), Conf(x=object())):
        with pytest.raises((ValueError, TypeError)):
            dump_hocon(bad)


def test_argument_parsers(capsys):
    from selfreconcode_amd import infer, train
    a = train.parse_args(['--gpu-ids', '2', '3', '--conf', 'c.conf', '--data', 'd', '--save-folder', 'result', '--model', 'm.pth',
                          '--model-rm-prefix', 'sdf.', 'netRender.', '--sdf-model', 's.pth'])
    assert (a.gpu_ids, a.conf, a.data, a.save_folder, a.model, a.model_rm_prefix, a.sdf_model) == ([2, 3], 'c.conf', 'd', 'result', 'm.pth', ['sdf.', 'netRender.'], 's.pth')
    assert a.resume is False and a.log_every == 1 and a.log == 'device'
    a = train.parse_args(['--conf', 'c', '--data', 'd', '--save-folder', 'r', '--resume', '--log-every', '10', '--log', 'item'])
    assert a.resume is True and a.log_every == 10 and a.log == 'item' and a.gpu_ids == [] and a.model is None
    for bad in (['--conf', 'c', '--data', 'd'], ['--conf', 'c', '--data', 'd', '--save-folder', 'r', '--log-every', '0'],
                ['--data', 'd', '--save-folder', 'r'], ['--conf', 'c', '--data', 'd', '--save-folder', 'r', '--log', 'loud']):
        with pytest.raises(SystemExit) as e:
            train.parse_args(bad)
        assert e.value.code == 2
    assert 'save-folder' in capsys.readouterr().err
    b = infer.build_parser().parse_args(['--gpu-ids', '1', '--batch-size', '4', '--rec-root', 'r', '--frames', '7', '--nV', '--C', '--nColor'])
    assert (b.gpu_ids, b.batch_size, b.rec_root, b.frames, b.nV, b.nI, b.C, b.nColor) == ([1], 4, 'r', 7, True, False, True, True)
    b = infer.build_parser().parse_args(['--rec-root', 'r'])
    assert (b.batch_size, b.frames, b.nV, b.nI, b.C, b.nColor) == (1, -1, False, False, False, False)
    with pytest.raises(SystemExit):
        infer.main(['--frames', '2'])                               # no --rec-root
    # the loader's cut of infer.py:133: batches 0, 1, ... while index * batch_size <= frames
    cut = lambda bs, frames: [i for i in infer.limited(range(10), bs, frames)]
    assert cut(1, 2) == [0, 1, 2] and cut(2, 2) == [0, 1] and cut(1, -1) == list(range(10)) and cut(3, 0) == [0]


def test_stage_schedule():
    from selfreconcode_amd.config import default_config
    from selfreconcode_amd.train import stage_schedule
    conf = default_config()                                         # medium from epoch 6, fine from epoch 12
    hits = {e: stage_schedule(conf, e) for e in range(0, conf.get_int('train.nepoch') + 1)}
    assert hits[6] == [('medium', 'coarse.pth')] and hits[12] == [('fine', 'medium.pth')]
    assert all(not v for e, v in hits.items() if e not in (6, 12))
    never = copy.deepcopy(conf)
    never['train']['medium']['start_epoch'] = -1
    assert all(stage_schedule(never, e) == ([('fine', 'medium.pth')] if e == 12 else []) for e in range(-1, 20))
    same = copy.deepcopy(conf)
    same['train']['medium']['start_epoch'] = same['train']['fine']['start_epoch'] = 3
    assert stage_schedule(same, 3) == [('medium', 'coarse.pth'), ('fine', 'medium.pth')] and stage_schedule(same, 2) == [] and stage_schedule(same, 4) == []
    first = copy.deepcopy(conf)
    first['train']['medium']['start_epoch'] = 0
    assert stage_schedule(first, 0) == [('medium', 'coarse.pth')]


def _reference_line(epoch, data_index, loss, info, ratio):
    """train.py:172-182 of the reference, restated with `info` holding plain numbers."""
    outinfo = '(%d/%d): loss = %.5f; color_loss: %.5f, eikonal_loss: %.5f' % (epoch, data_index, loss, info['color_loss'], info['grad_loss']) + \
              (' normal_loss: %.5f,' % info['normal_loss'] if 'normal_loss' in info else '') + \
              (' def_loss: %.5f,' % info['def_loss'] if 'def_loss' in info else '') + \
              (' offset_loss: %.5f,' % info['offset_loss'] if 'offset_loss' in info else '') + \
              (' dct_loss: %.5f,' % info['dct_loss'] if 'dct_loss' in info else '')
    outinfo += '\n'
    outinfo += '\tpc_sdf_l: %.5f' % (info['pc_loss_sdf'])
    outinfo += ';\tpc_norm_l: %.5f; ' % (info['pc_loss_norm']) if 'pc_loss_norm' in info else '; '
    for k, v in info['pc_loss'].items():
        outinfo += k + ': %.5f\t' % v
    outinfo += '\n\trayInfo(%d,%d)\tinvInfo(%d,%d)\tratio: (%.2f,%.2f,%.2f)\tremesh: %.3f' % (
        *info['rayInfo'], *info['invInfo'], ratio['sdfRatio'], ratio['deformerRatio'], ratio['renderRatio'], info['remesh'])
    return outinfo


def test_format_log_line_is_the_references_text():
    from selfreconcode_amd.train import LOG_COLUMNS, PC_LOSS_KEYS, deformer_ratio, format_log_line, log_values, _item_row
    f = lambda x: float(np.float32(x))                              # what a float32 device scalar gives through .item()
    full = {'color_loss': f(0.123456), 'grad_loss': f(0.000049), 'normal_loss': f(1.5), 'def_loss': f(2.25e-3), 'offset_loss': f(0.0317),
            'dct_loss': f(7.0), 'pc_loss_sdf': f(0.01234), 'pc_loss_norm': f(0.5),
            'pc_loss': {'mask_loss': f(0.25), 'lap_loss': f(1e-3), 'edge_loss': f(0.2), 'norm_loss': f(0.3), 'defconst_loss': f(0.045)},
            'rayInfo': (6144, 6001), 'invInfo': (6001, 5999), 'remesh': 3. + 7. / 30.}
    bare = {'color_loss': -1.0, 'grad_loss': f(0.02), 'pc_loss_sdf': f(0.4), 'pc_loss': {'mask_loss': f(0.6)}, 'rayInfo': (512, 0),
            'invInfo': (-1, -1), 'remesh': 1.}
    some = dict(bare, normal_loss=f(0.75), offset_loss=f(0.), pc_loss={'mask_loss': f(0.6), 'defconst_loss': f(0.01)})
    for (epoch, data_index, loss, opt_times), info in zip(((12, 345, f(3.14159), 2500.), (0, 0, f(61.5), 0.), (199, 7, f(-0.5), 123.)), (full, bare, some)):
        ratio = {'sdfRatio': 1., 'deformerRatio': deformer_ratio(opt_times), 'renderRatio': 1.}
        row = _item_row(log_values(epoch, data_index, torch.tensor(loss), info, ratio, 1e-4))
        assert row.dtype == np.float32 and row.shape == (len(LOG_COLUMNS),)
        assert format_log_line(row) == _reference_line(epoch, data_index, loss, info, ratio)
    assert np.isnan(row[LOG_COLUMNS.index('dct_loss')]) and row[LOG_COLUMNS.index('lr')] == np.float32(1e-4)
    assert set(PC_LOSS_KEYS) < set(LOG_COLUMNS) and len(LOG_COLUMNS) <= 32 and len(set(LOG_COLUMNS)) == len(LOG_COLUMNS)


def test_sidecar_key_set():
    """What latest.state.pth holds, from stand-ins on the CPU (the generators' device state aside), and that a sidecar with another
    key set is refused instead of half restored."""
    from selfreconcode_amd import train
    from selfreconcode_amd.config import default_config
    cfg = default_config()

    class Net:
        forward_time, remesh_time, remesh_intersect, point_radius, sdfShrinkRadius, angThred = 7, 2.5, 30, 0.006, 0.0, torch.tensor(0.05)
        conf, next_conf, next_train_conf = cfg.get_config('loss_coarse'), cfg.get_config('loss_medium'), cfg.get_config('train.medium')
        TmpVs, Tmpfs, draw = torch.zeros(4, 3, requires_grad=True), torch.zeros(2, 3, dtype=torch.int64), True
    net = Net()
    net.TmpOptimizer = torch.optim.SGD([net.TmpVs], lr=0.05, momentum=0.9)
    w = torch.zeros(3, requires_grad=True)
    opt = torch.optim.Adam([w], lr=1e-4)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, [1], gamma=0.333)
    real = torch.cuda.get_rng_state
    torch.cuda.get_rng_state = lambda device=None: torch.zeros(16, dtype=torch.uint8)
    try:
        state = train.capture_state(4, 99., 'medium', False, net, opt, sch, 'cuda:0')
    finally:
        torch.cuda.get_rng_state = real
    assert set(state) == set(train.SIDECAR_KEYS) and len(train.SIDECAR_KEYS) == len(set(train.SIDECAR_KEYS))
    for key in ('optimizer', 'scheduler', 'epoch', 'opt_times', 'stage', 'forward_time', 'remesh_time', 'remesh_intersect', 'point_radius',
                'sdfShrinkRadius', 'loss_conf', 'pending_loss_conf', 'pending_train_conf', 'TmpVs', 'Tmpfs', 'TmpOptimizer', 'draw',
                'rng_python', 'rng_torch_cpu', 'rng_torch_gpu'):
        assert key in state, key
    assert (state['epoch'], state['opt_times'], state['stage'], state['forward_time'], state['draw']) == (4, 99., 'medium', 7, True)
    fresh = Net()
    fresh.conf = fresh.next_conf = fresh.next_train_conf = None
    fresh.forward_time, fresh.draw = 0, False
    assert train.restore_state(state, fresh, opt, sch, 'cpu') == (4, 99., False)
    assert fresh.conf == cfg.get_config('loss_coarse') and fresh.next_conf == cfg.get_config('loss_medium') and fresh.next_train_conf == cfg.get_config('train.medium')
    assert fresh.forward_time == 7 and fresh.draw is True and fresh.TmpVs.requires_grad and fresh.TmpVs.is_leaf
    with pytest.raises(ValueError):
        train.restore_state({k: v for k, v in state.items() if k != 'TmpOptimizer'}, fresh, opt, sch, 'cpu')
    with pytest.raises(ValueError):
        train.restore_state(dict(state, format=0), fresh, opt, sch, 'cpu')
