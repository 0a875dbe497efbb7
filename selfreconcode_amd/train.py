"""The training driver: the reference's train.py over this package's pieces, with the per-iteration log kept on the device and a
resume that continues bit for bit.

    python -m selfreconcode_amd.train --gpu-ids 0 --conf config.conf --data <capture folder> --save-folder result [--resume]

`train()` follows train.py line by line -- the three resolution pyramids, save_root/config.conf and debug/, getDatasetAndLoader ->
getOptNet -> set_hierarchical_config('coarse'), the optional load_model, the SDF pre-fit and its .ply, the two parameter groups,
MultiStepLR, the epoch loop over range(0, nepoch + 1) with the medium / fine switches (coarse.pth / medium.pth), deformerRatio =
opt_times / 2500 + 0.5, draw = True in the fine stage, latest.pth and scheduler.step() at the end of every epoch -- and takes the step
itself from bench.py's timed loop (OptimNetwork.forward's eager contract): zero_grad -> forward -> backward -> propagateTmpPsGrad ->
FusedAdam step, with deferred weight gradients.

The log.  The reference prints ~15 values per iteration through .item().  Here the row is appended to a trainlog.TrainLog after
propagateTmpPsGrad -- `invInfo` is set there, and the ray branch (whose stream made color_loss / normal_loss / invInfo) has joined the
main stream there -- and the text is printed when the row has arrived on the host, usually an iteration or two later.  `log='item'` is
the reference's blocking style, kept for debugging and as the comparison of the tests; `log='off'` prints nothing.

Resume.  Next to latest.pth (the reference's format, unchanged) every epoch writes latest.state.pth (SIDECAR_KEYS): what a fresh
process needs beyond the weights and tables to continue with the same bits -- optimiser and scheduler, counters, the stage, the
template mesh and its SGD momentum, the active and the pending loss configuration, the three random generators.
"""
import argparse
import os
import os.path as osp
import random

import numpy as np
import torch

from .config import dump_hocon, load_config, parse_hocon

# train.py:27-60
RESOLUTIONS = {
    'coarse': [(14 + 1, 20 + 1, 8 + 1), (28 + 1, 40 + 1, 16 + 1), (56 + 1, 80 + 1, 32 + 1), (112 + 1, 160 + 1, 64 + 1), (224 + 1, 320 + 1, 128 + 1)],
    'medium': [(18 + 1, 24 + 1, 12 + 1), (36 + 1, 48 + 1, 24 + 1), (72 + 1, 96 + 1, 48 + 1), (144 + 1, 192 + 1, 96 + 1), (288 + 1, 384 + 1, 192 + 1)],
    'fine': [(20 + 1, 26 + 1, 14 + 1), (40 + 1, 52 + 1, 28 + 1), (80 + 1, 104 + 1, 56 + 1), (160 + 1, 208 + 1, 112 + 1), (320 + 1, 416 + 1, 224 + 1)],
}
STAGES = ('coarse', 'medium', 'fine')

# One row per logged iteration.  The optional terms of the reference's print are columns of their own; a term the iteration did not
# compute is NaN in the row and absent from the text.
PC_LOSS_KEYS = ('mask_loss', 'lap_loss', 'edge_loss', 'norm_loss', 'defconst_loss')       # info['pc_loss'], in the order computeTmpPcLoss fills it
LOG_COLUMNS = ('epoch', 'data_index', 'loss', 'color_loss', 'grad_loss', 'normal_loss', 'def_loss', 'offset_loss', 'dct_loss',
               'pc_loss_sdf', 'pc_loss_norm') + PC_LOSS_KEYS + ('ray_num', 'ray_converged', 'inv_num', 'inv_ok',
                                                                'sdfRatio', 'deformerRatio', 'renderRatio', 'remesh', 'lr')
_COL = {name: i for i, name in enumerate(LOG_COLUMNS)}

SIDECAR_KEYS = ('format', 'epoch', 'opt_times', 'stage', 'in_fine_hie', 'optimizer', 'scheduler', 'forward_time', 'remesh_time', 'remesh_intersect',
                'point_radius', 'sdfShrinkRadius', 'angThred', 'loss_conf', 'pending_loss_conf', 'pending_train_conf', 'TmpVs', 'Tmpfs',
                'TmpOptimizer', 'draw', 'rng_python', 'rng_torch_cpu', 'rng_torch_gpu')
SIDECAR_FORMAT = 1


def stage_schedule(conf, epoch):
    """The stage switches the loop makes at the START of `epoch` (train.py:147-157), in order: [(stage, checkpoint written before it)].
    A start epoch of -1 (any negative) never switches; equal start epochs switch twice in one epoch, medium first."""
    out = []
    for stage, pth in (('medium', 'coarse.pth'), ('fine', 'medium.pth')):
        start = conf.get_int('train.%s.start_epoch' % stage)
        if start >= 0 and epoch == start:
            out.append((stage, pth))
    return out


def deformer_ratio(opt_times):
    return opt_times / 2500. + 0.5                                  # train.py:164


def format_log_line(row):
    """The text train.py:172-182 prints for one iteration, from a row of LOG_COLUMNS (a sequence of floats; NaN = term absent)."""
    v = {name: float(row[i]) for name, i in _COL.items()}
    has = lambda name: not np.isnan(v[name])
    outinfo = '(%d/%d): loss = %.5f; color_loss: %.5f, eikonal_loss: %.5f' % (v['epoch'], v['data_index'], v['loss'], v['color_loss'], v['grad_loss']) + \
              (' normal_loss: %.5f,' % v['normal_loss'] if has('normal_loss') else '') + \
              (' def_loss: %.5f,' % v['def_loss'] if has('def_loss') else '') + \
              (' offset_loss: %.5f,' % v['offset_loss'] if has('offset_loss') else '') + \
              (' dct_loss: %.5f,' % v['dct_loss'] if has('dct_loss') else '')
    outinfo += '\n'
    outinfo += '\tpc_sdf_l: %.5f' % v['pc_loss_sdf']
    outinfo += ';\tpc_norm_l: %.5f; ' % v['pc_loss_norm'] if has('pc_loss_norm') else '; '
    for k in PC_LOSS_KEYS:
        if has(k):
            outinfo += k + ': %.5f\t' % v[k]
    outinfo += '\n\trayInfo(%d,%d)\tinvInfo(%d,%d)\tratio: (%.2f,%.2f,%.2f)\tremesh: %.3f' % (
        v['ray_num'], v['ray_converged'], v['inv_num'], v['inv_ok'], v['sdfRatio'], v['deformerRatio'], v['renderRatio'], v['remesh'])
    return outinfo


def log_values(epoch, data_index, loss, info, ratio, lr):
    """The dict TrainLog.append takes for one iteration: device tensors stay device tensors, host numbers stay host numbers."""
    vals = {'epoch': epoch, 'data_index': data_index, 'loss': loss.detach(), 'lr': lr, 'remesh': info['remesh'],
            'sdfRatio': ratio['sdfRatio'], 'deformerRatio': ratio['deformerRatio'], 'renderRatio': ratio['renderRatio']}
    for k in ('color_loss', 'grad_loss', 'normal_loss', 'def_loss', 'offset_loss', 'dct_loss', 'pc_loss_sdf', 'pc_loss_norm'):
        if k in info:
            vals[k] = info[k]
    for k in PC_LOSS_KEYS:
        if k in info['pc_loss']:
            vals[k] = info['pc_loss'][k]
    (vals['ray_num'], vals['ray_converged']), (vals['inv_num'], vals['inv_ok']) = info['rayInfo'], info['invInfo']
    return vals


def _item_row(vals):
    """log='item': the row of `vals` read value by value, each device tensor through .item() -- the reference's blocking style."""
    row = np.full((len(LOG_COLUMNS),), np.nan, np.float32)
    for k, x in vals.items():
        row[_COL[k]] = np.float32(x.item() if isinstance(x, torch.Tensor) else x)
    return row


def _log_tensor(x):
    """A value of `info` in the form TrainLog takes: a one-element float32 / int64 device tensor as it is (a bool count becomes int64)."""
    if isinstance(x, torch.Tensor) and x.dtype not in (torch.float32, torch.int64):
        return x.long() if not x.dtype.is_floating_point else x.float()
    return x


def contiguous_tables(dataset):
    """FusedAdam updates dense contiguous tensors.  The per-frame codes are made as a transpose (dataset.py:18-24) and come back from a
    checkpoint with the strides they were saved with: each learnable table that is not contiguous is replaced by a contiguous leaf
    with the same values.  Before the optimiser takes dataset.learnable_weights()."""
    def fix(t):
        return t if t.is_contiguous() else t.detach().contiguous().requires_grad_(t.requires_grad)
    dataset.conds = [fix(c) for c in dataset.conds]
    dataset.poses, dataset.trans = fix(dataset.poses), fix(dataset.trans)
    dataset.camera_params = {k: fix(v) for k, v in dataset.camera_params.items()}
    return dataset


# ------------------------------------------------------------------------------------------------ exact resume
def sidecar_path(save_root):
    return osp.join(save_root, 'latest.state.pth')


def capture_state(next_epoch, opt_times, stage, in_fine_hie, optNet, optimizer, scheduler, device):
    """The sidecar of latest.pth (SIDECAR_KEYS), taken at the end of an epoch after scheduler.step().  Configurations travel as text."""
    text = lambda c: None if c is None else dump_hocon(c)
    tmp_opt = getattr(optNet, 'TmpOptimizer', None)
    return {'format': SIDECAR_FORMAT, 'epoch': int(next_epoch), 'opt_times': float(opt_times), 'stage': stage, 'in_fine_hie': bool(in_fine_hie),
            'optimizer': optimizer.state_dict(), 'scheduler': scheduler.state_dict(),
            'forward_time': int(optNet.forward_time), 'remesh_time': float(optNet.remesh_time), 'remesh_intersect': int(optNet.remesh_intersect),
            'point_radius': float(optNet.point_radius), 'sdfShrinkRadius': float(optNet.sdfShrinkRadius),
            'angThred': optNet.angThred.detach().cpu().clone() if torch.is_tensor(optNet.angThred) else optNet.angThred,   # (a host double: kept as it is)
            'loss_conf': text(optNet.conf), 'pending_loss_conf': text(optNet.next_conf), 'pending_train_conf': text(optNet.next_train_conf),
            'TmpVs': None if optNet.TmpVs is None else optNet.TmpVs.detach().cpu().clone(),
            'Tmpfs': None if optNet.Tmpfs is None else optNet.Tmpfs.detach().cpu().clone(),
            'TmpOptimizer': None if tmp_opt is None else tmp_opt.state_dict(), 'draw': bool(getattr(optNet, 'draw', False)),
            'rng_python': random.getstate(), 'rng_torch_cpu': torch.get_rng_state(), 'rng_torch_gpu': torch.cuda.get_rng_state(device)}


def restore_state(state, optNet, optimizer, scheduler, device):
    """Everything of a sidecar except the stage switch itself (the caller has re-made the stage's loader and engine with
    set_hierarchical_config) and the random generators (restore_rng, right before the loop).  -> (next epoch, opt_times, in_fine_hie)"""
    if state.get('format') != SIDECAR_FORMAT or set(state) != set(SIDECAR_KEYS):
        raise ValueError(f"latest.state.pth: format {state.get('format')!r} with keys {sorted(set(state) ^ set(SIDECAR_KEYS))} missing or unknown")
    optimizer.load_state_dict(state['optimizer'])
    scheduler.load_state_dict(state['scheduler'])
    conf = lambda t: None if t is None else parse_hocon(t)
    optNet.conf, optNet.next_conf, optNet.next_train_conf = conf(state['loss_conf']), conf(state['pending_loss_conf']), conf(state['pending_train_conf'])
    optNet.forward_time, optNet.remesh_time, optNet.remesh_intersect = state['forward_time'], state['remesh_time'], state['remesh_intersect']
    optNet.point_radius, optNet.sdfShrinkRadius = state['point_radius'], state['sdfShrinkRadius']
    optNet.angThred = state['angThred']
    if state['draw']:
        optNet.draw = True
    if state['TmpVs'] is not None:
        optNet._mesh_topo = None
        optNet.TmpVs = state['TmpVs'].to(device).requires_grad_(True)
        optNet.Tmpfs = state['Tmpfs'].to(device)
        optNet.TmpOptimizer = torch.optim.SGD([optNet.TmpVs], lr=0.05, momentum=0.9)          # as _remesh_if_due makes it
        if state['TmpOptimizer'] is not None:
            optNet.TmpOptimizer.load_state_dict(state['TmpOptimizer'])
    return state['epoch'], state['opt_times'], state['in_fine_hie']


def prime_weight_packs(optNet):
    """Makes the packed weights of the three networks exist BEFORE a checkpoint is loaded into them.  A pack is first built by torch's
    weight-norm operator and from then on re-filled in place by sr_pack_weights whenever its parameters have changed
    (mlp_engine.refresh_packs); the two agree to the last ulp or so, not to the bit.  A run that goes straight through evaluates its
    networks with re-filled packs from the second iteration on -- so must the run that resumes it: with the packs in place, loading
    the weights makes them stale and the first iteration re-fills them like every later one."""
    from .mlp_engine import packed_weights_of
    with torch.no_grad():
        for module in (optNet.sdf, optNet.deformer.defs[0], optNet.netRender):
            packed_weights_of(module, len(module.spec.layers))


def restore_rng(state, device):
    random.setstate(state['rng_python'])
    torch.set_rng_state(state['rng_torch_cpu'])
    torch.cuda.set_rng_state(state['rng_torch_gpu'], device)


# ------------------------------------------------------------------------------------------------ the iteration and its log
def step(optNet, optimizer, outs, sample_pix_num, ratio, frame_ids, root=None):
    """One iteration in the order of OptimNetwork.forward's eager contract (bench.py's timed loop): zero_grad -> forward -> backward ->
    propagateTmpPsGrad (which also flushes the deferred weight gradients) -> optimiser step.  -> the loss, a device tensor."""
    optimizer.zero_grad(set_to_none=True)
    loss = optNet(outs, sample_pix_num, ratio, frame_ids, root)
    loss.backward()
    optNet.propagateTmpPsGrad(frame_ids, ratio)
    optimizer.step()
    return loss


class LoopLog:
    """The three log modes behind one call.  record() is called after step(): every tensor of `info` is ordered before the main stream
    there -- the template branch and the sampled terms were made on it; color_loss, normal_loss and invInfo are made on the ray
    branch's stream, which _finish_ray_branch (the end of propagateTmpPsGrad) joins to the main stream; rayInfo's count is taken on
    the main stream after it has waited for the refiner's stream (_sampled_terms)."""

    def __init__(self, mode, device, out=print, ring_rows=256):
        from .trainlog import TrainLog
        if mode not in ('device', 'item', 'off'):
            raise ValueError(f"log = {mode!r} ('device', 'item' or 'off')")
        self.mode, self.out, self.rows, self.lines = mode, out, [], []
        self.tlog = TrainLog(LOG_COLUMNS, ring_rows, device) if mode == 'device' else None

    def _emit(self, new_rows):
        for row in new_rows:
            self.rows.append(row)
            self.lines.append(format_log_line(row))
            self.out(self.lines[-1])

    def record(self, epoch, data_index, loss, info, ratio, lr):
        if self.mode == 'off':
            return
        vals = {k: _log_tensor(x) for k, x in log_values(epoch, data_index, loss, info, ratio, lr).items()}
        if self.tlog is not None:
            self.tlog.append(vals)
            self._emit(self.tlog.drain())
        else:
            self._emit([_item_row(vals)])

    def flush(self):
        """End of an epoch / exit: wait for the rows still on their way."""
        if self.tlog is not None:
            self._emit(self.tlog.drain(block=True))

    @property
    def stalls(self):
        return 0 if self.tlog is None else self.tlog.stalls

    def array(self):
        return np.stack(self.rows) if self.rows else np.empty((0, len(LOG_COLUMNS)), np.float32)


# ------------------------------------------------------------------------------------------------ the driver
class TrainResult:
    """What train() hands back: `rows` float32 [iterations logged, len(LOG_COLUMNS)], `lines` the printed text of each, the network,
    dataset and save folder, the next epoch, and the log's stall count (log='device')."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def train(data_root, conf, save_folder, device="cuda:0", model=None, sdf_model=None, model_rm_prefix=None, resume=False, log='device',
          log_every=1, stop_after_epoch=None, out=print, resolutions=None, smpl_model=None, skinner_resolution=None, bmins=None, bmaxs=None,
          log_ring_rows=256):
    """The reference's train.py (see the module docstring).  `conf`: a config.Conf or the path of a .conf file.  `resume`: continue from
    save_folder's latest.pth + latest.state.pth.  `log`: 'device' | 'item' | 'off'; `log_every`: log the iterations whose data index is
    a multiple of it.  `stop_after_epoch`: leave the loop after that epoch's checkpoint (what an interrupted run looks like).
    Extensions for small scenes: `resolutions` {stage: pyramid} instead of train.py's three, `smpl_model` (the dataset's body-model hook,
    see getOptNet), `skinner_resolution`, and a fixed box `bmins` / `bmaxs` (None: the adaptive box, as train.py sets it)."""
    from . import mlp_engine
    from .MCAcc import Seg3dLossless
    from .dataset import getDatasetAndLoader
    from .mesh_io import write_ply
    from .model import getOptNet
    from .optim import FusedAdam
    from .utils.checkpoint import load_model, save_model, set_hierarchical_config
    if log not in ('device', 'item', 'off'):
        raise ValueError(f"train: log = {log!r} ('device', 'item' or 'off')")
    if int(log_every) < 1:
        raise ValueError(f"train: log_every = {log_every}")
    if save_folder is None:
        raise ValueError('please set save-folder...')
    config = load_config(conf) if isinstance(conf, (str, os.PathLike)) else conf
    device = torch.device(device)
    resolutions = dict(RESOLUTIONS, **(resolutions or {}))
    say = out if log != 'off' else (lambda *a, **k: None)

    save_root = osp.join(data_root, save_folder)
    debug_root = osp.join(save_root, 'debug')
    os.makedirs(save_root, exist_ok=True)
    os.makedirs(debug_root, exist_ok=True)
    with open(osp.join(save_root, 'config.conf'), 'w') as ff:
        ff.write(dump_hocon(config))
    condlen = {'deformer': config.get_int('mlp_deformer.condlen'), 'renderer': config.get_int('render_net.condlen')}
    batch_size = config.get_int('train.coarse.point_render.batch_size')
    dataset, dataloader = getDatasetAndLoader(data_root, condlen, batch_size, config.get_bool('train.shuffle'), config.get_int('train.num_workers'),
                                              config.get_bool('train.opt_pose'), config.get_bool('train.opt_trans'),
                                              config.get_config('train.opt_camera'), device=device)
    if smpl_model is not None:
        dataset.smpl_model = smpl_model
    use_initial_sdf = config.get_int('train.initial_iters') <= 0
    kw = {} if skinner_resolution is None else {'skinner_resolution': skinner_resolution}
    optNet, sdf_initialized = getOptNet(dataset, batch_size, bmins, bmaxs, resolutions['coarse'], device, config, use_initial_sdf, **kw)
    optNet, dataloader = set_hierarchical_config(config, 'coarse', optNet, dataloader, resolutions['coarse'])

    state = None
    if resume:
        model = osp.join(save_root, 'latest.pth')
        if not osp.isfile(model) or not osp.isfile(sidecar_path(save_root)):
            raise FileNotFoundError(f"--resume: {model} and {sidecar_path(save_root)} are both needed")
        state = torch.load(sidecar_path(save_root), map_location='cpu', weights_only=False)
        sdf_model, model_rm_prefix, sdf_initialized = None, None, -1
        prime_weight_packs(optNet)
    if model is not None and osp.isfile(model):
        msg = 'load model: ' + model
        if sdf_model is not None:
            msg += ' and substitute sdf model with: ' + sdf_model
            sdf_initialized = -1
        say(msg)
        optNet, dataset = load_model(model, optNet, dataset, device, sdf_model, model_rm_prefix)

    say('box:')
    say(optNet.engine.b_min.view(-1).tolist())
    say(optNet.engine.b_max.view(-1).tolist())
    optNet.train()

    if sdf_initialized > 0:
        name = osp.join(data_root, 'initial_sdf_idr' + '_%d_%d' % (config.get_int('sdf_net.multires'), config.get_int('train.skinner_pose_type')))
        optNet.initializeTmpSDF(sdf_initialized, name + '.pth', True)
        engine = Seg3dLossless(query_func=None, b_min=optNet.engine.b_min, b_max=optNet.engine.b_max, resolutions=resolutions['coarse'],
                               align_corners=False, balance_value=0.0, use_cuda_impl=getattr(optNet.engine, 'use_cuda_impl', True)).to(device)
        verts, faces = optNet.discretizeSDF(-1, engine)
        write_ply(name + '.ply', verts.cpu().numpy(), faces.cpu().numpy())

    learnable_ws = contiguous_tables(dataset).learnable_weights()
    deferred_before = mlp_engine.DEFERRED_PARAM_GRADS
    mlp_engine.set_deferred_param_grads(True)                       # one weight-norm backward + gradient add per layer and step (bench.py)
    try:
        optimizer = FusedAdam([{'params': learnable_ws}, {'params': [p for p in optNet.parameters() if p.requires_grad]}],
                              lr=config.get_float('train.learning_rate'))
        scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, config.get_list('train.scheduler.milestones'),
                                                         gamma=config.get_float('train.scheduler.factor'))
        ratio = {'sdfRatio': None, 'deformerRatio': None, 'renderRatio': None}
        opt_times, first_epoch, stage, in_fine_hie = 0., 0, 'coarse', False
        nepochs = config.get_int('train.nepoch')
        sample_pix_num = config.get_int('train.sample_pix_num')
        if state is not None:
            stage = state['stage']
            if stage != 'coarse':
                optNet, dataloader = set_hierarchical_config(config, stage, optNet, dataloader, resolutions[stage])
            first_epoch, opt_times, in_fine_hie = restore_state(state, optNet, optimizer, scheduler, device)
            restore_rng(state, device)
            say('resume at epoch %d (%s stage, %d iterations done)' % (first_epoch, stage, int(opt_times)))

        optNet._side_stream(device)                                 # (the network's side stream is taken before the log takes its copy stream)
        looplog = LoopLog(log, device, say, log_ring_rows)

        epoch = first_epoch - 1
        for epoch in range(first_epoch, nepochs + 1):
            for new_stage, pth in stage_schedule(config, epoch):
                optNet, dataloader = set_hierarchical_config(config, new_stage, optNet, dataloader, resolutions[new_stage])
                torch.cuda.empty_cache()
                say('enable %s hierarchical' % new_stage)
                save_model(osp.join(save_root, pth), epoch, optNet, dataset)
                stage = new_stage
                in_fine_hie = in_fine_hie or new_stage == 'fine'
            for data_index, (frame_ids, outs) in enumerate(dataloader):
                frame_ids = frame_ids.long().to(device)
                ratio['sdfRatio'] = 1.
                ratio['deformerRatio'] = deformer_ratio(opt_times)
                ratio['renderRatio'] = 1.
                loss = step(optNet, optimizer, outs, sample_pix_num, ratio, frame_ids, debug_root)
                if data_index % log_every == 0:
                    looplog.record(epoch, data_index, loss, optNet.info, ratio, optimizer.param_groups[0]['lr'])
                opt_times += 1.
            if in_fine_hie:
                optNet.draw = True
            save_model(osp.join(save_root, 'latest.pth'), epoch, optNet, dataset)
            scheduler.step()
            torch.save(capture_state(epoch + 1, opt_times, stage, in_fine_hie, optNet, optimizer, scheduler, device), sidecar_path(save_root))
            looplog.flush()
            if stop_after_epoch is not None and epoch >= stop_after_epoch:
                break
        looplog.flush()
    finally:
        mlp_engine.set_deferred_param_grads(deferred_before)
    return TrainResult(rows=looplog.array(), lines=looplog.lines, optNet=optNet, dataset=dataset, save_root=save_root, next_epoch=epoch + 1,
                       stalls=looplog.stalls, log=looplog.tlog)


def build_parser():
    parser = argparse.ArgumentParser(prog='python -m selfreconcode_amd.train', description='neu video body rec')
    parser.add_argument('--gpu-ids', nargs='+', type=int, metavar='IDs', default=[], help='gpu ids')
    parser.add_argument('--conf', default=None, metavar='M', help='config file')
    parser.add_argument('--data', default=None, metavar='M', help='data root')
    parser.add_argument('--model', default=None, metavar='M', help='pretrained scene model')
    parser.add_argument('--model-rm-prefix', nargs='+', type=str, metavar='rm prefix', help='rm model prefix')
    parser.add_argument('--sdf-model', default=None, metavar='M', help='substitute sdf model')
    parser.add_argument('--save-folder', default=None, metavar='M', help='save folder')
    parser.add_argument('--resume', action='store_true', help='continue from <data>/<save-folder>/latest.pth and latest.state.pth, bit for bit')
    parser.add_argument('--log-every', default=1, type=int, metavar='N', help='print the iterations whose index in the epoch is a multiple of N')
    parser.add_argument('--log', default='device', choices=('device', 'item', 'off'), help="'device': rows gathered on the GPU and printed "
                        "when they arrive; 'item': a blocking read per value, as the reference; 'off'")
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.save_folder is None:
        parser.error('please set save-folder...')
    if args.conf is None or args.data is None:
        parser.error('--conf and --data are required')
    if args.log_every < 1:
        parser.error('--log-every must be at least 1')
    return args


def main(argv=None):
    args = parse_args(argv)
    device = torch.device('cuda', args.gpu_ids[0] if args.gpu_ids else 0)
    train(args.data, args.conf, args.save_folder, device=device, model=args.model, sdf_model=args.sdf_model,
          model_rm_prefix=args.model_rm_prefix, resume=args.resume, log=args.log, log_every=args.log_every)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
