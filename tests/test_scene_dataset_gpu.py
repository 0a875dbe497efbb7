"""Frames resident on the GPU: the expansion kernel (ops.frames_fetch / sr_frames_fetch) bit for bit against the reference's float32
numpy expressions at every alignment path, dataset.SceneDataset on the committed capture folder against the reference's own class
(tests/golden/scene_dataset.npz, tools/gen_scene_dataset_golden.py), and one training step from a folder written by the test."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from selfreconcode_amd import _lib, ops
from selfreconcode_amd.dataset import FrameLoader, RandomSampler, SceneDataset, getDatasetAndLoader

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLDER = os.path.join(ROOT, "tests", "golden", "scene_folder")
CONDS_LENS = {'deformer': 8, 'renderer': 16}
F = 5
SENTINEL, GUARD = -7.0, 64
# (H, W): 105 bytes per frame (odd: padded tail, no output frame after the first 16-byte aligned), 180 (a multiple of 4, not of 16), 384
# (fully aligned), 3 (the minimum), 4653 (several workgroups' worth of chunks with a tail), 874 800 (the workload's size: index width)
SHAPES = [(5, 7), (6, 10), (8, 16), (1, 1), (33, 47), (540, 540)]
ID_LISTS = [[4, 0, 4, 2], [3], [(7 * i + 3) % F for i in range(17)]]         # repeat / order / last frame; N = 1; N = 17 > SR_FRAMES_MAX_BATCH


class _Case:
    """Seeded random stores of F frames (a permutation of all 256 byte values leads each store that has room for it) and, per frame, what
    the reference's expressions give in numpy float32 (dataset.py:88, 97, 101-102) -- computed once per shape, never by the code under test."""

    def __init__(self, H, W):
        rng = np.random.default_rng(1000 * H + W)
        self.H, self.W = H, W
        self.img = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
        self.normal = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
        for a in (self.img, self.normal):
            if a.size >= 256:
                a.reshape(-1)[:256] = rng.permutation(256).astype(np.uint8)
        self.mask = rng.integers(0, 2, (F, H, W), dtype=np.uint8)
        self.want_img = torch.from_numpy((self.img.astype(np.float32) / 255. - 0.5) * 2).to(DEV)
        self.want_normal = torch.from_numpy(np.ascontiguousarray(2. * self.normal[:, :, :, ::-1].astype(np.float32) / 255. - 1.)).to(DEV)
        self.want_mask = torch.from_numpy(self.mask.astype(np.float32)).to(DEV)
        assert self.want_img.dtype == self.want_normal.dtype == torch.float32

    def stores(self, normals=True, poison=False):
        def store(a):
            nbytes = int(np.prod(a.shape[1:]))
            s = torch.full((F, ops.frames_pitch(nbytes)), 255 if poison else 0, dtype=torch.uint8, device=DEV)
            s[:, :nbytes] = torch.from_numpy(a.reshape(F, nbytes)).to(DEV)
            return s
        return store(self.img), store(self.normal) if normals else None, store(self.mask)

    def want(self, ids, normals=True):
        ids = torch.as_tensor(ids, device=DEV)
        return self.want_img[ids], self.want_normal[ids] if normals else None, self.want_mask[ids]


_CASES = {}


def _case(H, W):
    if (H, W) not in _CASES:
        _CASES[(H, W)] = _Case(H, W)
    return _CASES[(H, W)]


def _guarded(shape, offset=0):
    """A float32 tensor of `shape` filled with a sentinel, `offset` floats into a buffer that goes on for GUARD floats behind it."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[offset:offset + n].view(shape)


def _side_stream():
    """A stream that is not the default one: the process's weight-gradient stream, which exists anyway.  Not a fresh torch.cuda.Stream():
    torch hands those out of a fixed pool in turn and the runtime multiplexes them onto a few hardware queues, so every stream a test
    takes moves the ones the tests after it get -- and tests/test_streams_gpu.py needs its side stream on another queue than the default
    stream's."""
    from selfreconcode_amd import mlp_engine
    return mlp_engine._tn_stream(torch.device(DEV))


def _same(got, want):
    return all((g is None and w is None) or (g is not None and w is not None and torch.equal(g, w)) for g, w in zip(got, want))


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("H,W", SHAPES)
def test_fetch_is_bit_exact_on_both_id_routes(H, W, normals):
    case = _case(H, W)
    stores = case.stores(normals)
    side = _side_stream()
    for ids in ID_LISTS:
        N = len(ids)
        want = case.want(ids, normals)
        bufs, outs = zip(*[_guarded(s) if s is not None else (None, None)
                           for s in ((N, H, W, 3), (N, H, W, 3) if normals else None, (N, H, W))])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                               # by value, on a stream that is not the default one
            got = ops.frames_fetch(*stores, H, W, ids, out=list(outs))
        torch.cuda.current_stream().wait_stream(side)
        assert _same(got, want), (H, W, normals, ids)
        assert all(b is None or bool((b[-GUARD:] == SENTINEL).all()) for b in bufs)
        by_device = ops.frames_fetch(*stores, H, W, torch.tensor(ids, device=DEV))
        assert _same(by_device, got), (H, W, normals, ids)
        if N == 1:
            assert _same(ops.frames_fetch(*stores, H, W, torch.tensor(ids)), got)          # a CPU tensor travels by value as well


@pytest.mark.parametrize("H,W", [(5, 7), (6, 10), (1, 1), (33, 47)])
def test_padding_bytes_never_reach_the_output(H, W):
    case = _case(H, W)
    ids = [4, 0, 4, 2]
    stores = case.stores(poison=True)
    assert all(bool((s[:, -1] == 255).all()) for s in stores)       # (these shapes do have padding)
    assert _same(ops.frames_fetch(*stores, H, W, ids), case.want(ids))
    assert _same(ops.frames_fetch(*stores, H, W, torch.tensor(ids, device=DEV)), case.want(ids))


def test_outputs_that_are_not_16_byte_aligned_take_the_narrow_path():
    """H W % 4 == 0 but the caller's buffers start 4 bytes off a 16-byte boundary."""
    H, W = 8, 16
    case, ids = _case(H, W), [4, 0, 4, 2]
    bufs, outs = zip(*[_guarded(s, offset=1) for s in ((4, H, W, 3), (4, H, W, 3), (4, H, W))])
    assert all(o.data_ptr() % 16 == 4 for o in outs)
    assert _same(ops.frames_fetch(*case.stores(), H, W, ids, out=list(outs)), case.want(ids))
    assert all(bool((b[-GUARD:] == SENTINEL).all()) and float(b[0]) == SENTINEL for b in bufs)


def test_every_byte_value_in_every_channel_phase():
    """All 256 values at each of the three channel positions of img and normal: 111 of them come out wrong with b * (1/255)."""
    H, W = 16, 16
    b = np.arange(256, dtype=np.uint8)
    img = np.stack([np.stack([np.roll(b, s), np.roll(b, s + 85), np.roll(b, s + 170)], -1).reshape(H, W, 3) for s in (0, 1)])
    store = torch.zeros((2, ops.frames_pitch(H * W * 3)), dtype=torch.uint8, device=DEV)
    store[:, :H * W * 3] = torch.from_numpy(img.reshape(2, -1)).to(DEV)
    mask = torch.ones((2, ops.frames_pitch(H * W)), dtype=torch.uint8, device=DEV)
    got_img, got_normal, got_mask = ops.frames_fetch(store, store, mask, H, W, [1, 0])
    assert np.array_equal(got_img.cpu().numpy(), ((img.astype(np.float32) / 255. - 0.5) * 2)[[1, 0]])
    assert np.array_equal(got_normal.cpu().numpy(), (2. * img[..., ::-1].astype(np.float32) / 255. - 1.)[[1, 0]])
    assert bool((got_mask == 1).all())
    r, x = np.float32(1.) / np.float32(255.), b.astype(np.float32)
    assert int(((x * r - np.float32(0.5)) * 2 != (x / np.float32(255.) - np.float32(0.5)) * 2).sum()) == 111


def test_ids_out_of_range():
    H, W = 6, 10
    case = _case(H, W)
    stores = case.stores()
    img, normal, mask = ops.frames_fetch(*stores, H, W, torch.tensor([-1, 5, 2], device=DEV))
    assert bool(torch.isnan(img[:2]).all()) and bool(torch.isnan(normal[:2]).all()) and bool((mask[:2] == 0).all())
    assert _same((img[2:], normal[2:], mask[2:]), case.want([2]))
    with pytest.raises(IndexError):                                 # the host route checks before any launch
        ops.frames_fetch(*stores, H, W, [-1, 5, 2])
    with pytest.raises(IndexError):
        ops.frames_fetch(*stores, H, W, torch.tensor([0, 5]))


def test_argument_errors():
    H, W = 5, 7
    case = _case(H, W)
    img, normal, mask = case.stores()
    out = [torch.empty((1, H, W, 3), device=DEV), torch.empty((1, H, W, 3), device=DEV), torch.empty((1, H, W), device=DEV)]
    packed, ids = _lib.SrFrameIds(), torch.zeros(1, dtype=torch.int64, device=DEV)

    def raw(by_value, by_device, N=1, p3=img.shape[1], p1=mask.shape[1]):
        _lib.launch("sr_frames_fetch", img, img, normal, mask, p3, p1, F, H, W, by_value, by_device, N, *out)
    raw(ctypes.byref(packed), None)
    raw(None, ids)
    for bad in (lambda: raw(ctypes.byref(packed), ids), lambda: raw(None, None), lambda: raw(None, ids, N=0), lambda: raw(None, ids, N=-3),
                lambda: raw(ctypes.byref(packed), None, N=_lib.SR_FRAMES_MAX_BATCH + 1), lambda: raw(None, ids, p3=104), lambda: raw(None, ids, p3=96),
                lambda: raw(None, ids, p1=40), lambda: raw(None, ids, p1=32), lambda: ops.frames_fetch(img, normal, mask, H, W, []),
                lambda: ops.frames_fetch(img[:, :104].contiguous(), None, mask, H, W, [0]),
                lambda: ops.frames_fetch(img[:, :96].contiguous(), None, mask, H, W, [0]),
                lambda: ops.frames_fetch(img, None, mask[:, :32].contiguous(), H, W, [0])):
        with pytest.raises(_lib.SrError, match="SR_EINVAL"):
            bad()
    with pytest.raises(RuntimeError, match="non-GPU"):
        ops.frames_fetch(img.cpu(), normal.cpu(), mask.cpu(), H, W, [0])
    with pytest.raises(RuntimeError):
        ops.frames_fetch(img, normal, mask.cpu(), H, W, [0])
    assert ctypes.sizeof(_lib.SrFrameIds) == 4 * _lib.SR_FRAMES_MAX_BATCH == 64 and ops.FRAMES_MAX_BATCH == 16


# ------------------------------------------------------------------------------------------------ the committed folder
@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "scene_dataset.npz")) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def ds():
    torch.manual_seed(0)
    return SceneDataset(FOLDER, CONDS_LENS, device=DEV)


def _frames_equal(outs, gold, ids):
    return set(outs) == {'img', 'mask', 'normal'} and all(
        outs[k].is_cuda and outs[k].dtype == torch.float32 and np.array_equal(outs[k].cpu().numpy(), gold[k][ids]) for k in outs)


def test_folder_frames_are_the_references(ds, gold):
    assert _frames_equal(ds.batch(range(12)), gold, list(range(12)))
    assert _frames_equal(ds.batch(torch.tensor([11, 0, 5], device=DEV)), gold, [11, 0, 5])
    for i in range(12):
        idx, out = ds[i]
        assert idx == i and tuple(out['img'].shape) == (6, 10, 3) and tuple(out['mask'].shape) == (6, 10)
        assert all(np.array_equal(out[k].cpu().numpy(), gold[k][i]) for k in ('img', 'mask', 'normal'))
    assert ds.img_u8.is_cuda and tuple(ds.img_u8.shape) == (12, 192) and tuple(ds.mask_u8.shape) == (12, 64)


def test_folder_tables_and_camera(ds, gold):
    ids = torch.from_numpy(gold['grad_ids']).to(DEV)
    poses, trans, dcond, rcond = ds.get_grad_parameters(ids, DEV)
    assert np.array_equal(poses.detach().cpu().numpy(), gold['grad_poses']) and np.array_equal(trans.detach().cpu().numpy(), gold['grad_trans'])
    for k, rows in enumerate((dcond, rcond)):                        # the float32 dot-product bound of tests/test_scene_dataset_cpu.py
        a, b = gold[f'cond_coef_{k}'].astype(np.float64), gold['dct_space'].astype(np.float64)
        bound = 4 * a.shape[1] * 2.0 ** -24 * (np.abs(a) @ np.abs(b)).max()
        assert rows.is_cuda and np.abs(rows.detach().cpu().numpy().astype(np.float64) - gold[f'grad_cond_{k}']).max() <= bound
    focal, centre, R, T, H, W = ds.get_camera_parameters(2, DEV)
    assert np.array_equal(focal.cpu().numpy(), gold['cam_focal']) and np.array_equal(centre.cpu().numpy(), gold['cam_centre'])
    assert np.array_equal(T.cpu().numpy(), gold['cam_T']) and [H, W] == gold['cam_hw'].tolist() and R.is_cuda
    assert np.abs(R.cpu().numpy() - gold['cam_R']).max() <= 8 * 2.0 ** -24      # same formula; at most seven float32 roundings of numbers <= 1 per entry
    assert ds.get_camera_parameters(3)[2].data_ptr() == R.data_ptr()           # the rotation of a fixed quaternion is built once
    windows, offsets = ds.get_batchframe_data('poses', torch.from_numpy(gold['window_fids']).to(DEV), int(gold['window']))
    assert np.array_equal(windows.detach().cpu().numpy(), gold['window_split']) and np.array_equal(offsets.cpu().numpy(), gold['window_split_offsets'])


def test_gradients_reach_the_tables(ds):
    for t in (ds.poses, ds.trans):
        t.requires_grad_(True)
    poses, trans, dcond, rcond = ds.get_grad_parameters(torch.tensor([3, 0, 3], device=DEV))
    (poses.sum() + 2 * dcond.sum()).backward()
    want = torch.zeros(12, device=DEV)
    want[3], want[0] = 2., 1.
    assert torch.equal(ds.poses.grad, want.view(12, 1, 1).expand(12, 24, 3)) and torch.equal(ds.conds[0].grad, 2 * want.view(12, 1).expand(12, 8))
    assert ds.trans.grad is None and ds.conds[1].grad is None
    ds.poses.grad = ds.conds[0].grad = None


def test_checkpoint_round_trip(ds, tmp_path):
    from selfreconcode_amd.utils.checkpoint import load_model, save_model
    net = torch.nn.Linear(2, 2)
    keep = ds.poses.detach().clone(), ds.camera_params['focal_length'].detach().clone()
    with torch.no_grad():
        ds.poses.add_(0.25); ds.camera_params['focal_length'].mul_(1.5)
    ds.opt_camera_params(True)
    path = str(tmp_path / "latest.pth")
    save_model(path, 3, net, ds)
    torch.manual_seed(5)
    fresh = SceneDataset(FOLDER, CONDS_LENS, device=DEV)
    fresh.poses.requires_grad_(True)
    assert not torch.equal(fresh.conds[0], ds.conds[0]) and not torch.equal(fresh.poses, ds.poses)
    _, loaded = load_model(path, net, fresh, DEV)
    assert loaded is fresh
    for name in ('poses', 'trans', 'shape'):
        assert torch.equal(getattr(fresh, name), getattr(ds, name)) and getattr(fresh, name).is_cuda and getattr(fresh, name).is_leaf
    assert fresh.poses.requires_grad and not fresh.trans.requires_grad
    assert all(torch.equal(a, b) and a.is_leaf and a.requires_grad for a, b in zip(fresh.conds, ds.conds))
    assert all(torch.equal(fresh.camera_params[k], v) and not fresh.camera_params[k].requires_grad for k, v in ds.camera_params.items())
    assert torch.equal(fresh.get_camera_parameters(1)[0], ds.get_camera_parameters(1)[0].detach())
    with torch.no_grad():
        ds.poses.copy_(keep[0]); ds.camera_params['focal_length'].copy_(keep[1])
    ds.opt_camera_params(False)


def test_an_ordered_epoch_visits_every_frame(ds, gold):
    loader = FrameLoader(ds, 5, RandomSampler(ds, 1, False))
    seen = []
    for frame_ids, outs in loader:
        assert frame_ids.dtype == torch.int64 and not frame_ids.is_cuda and _frames_equal(outs, gold, frame_ids.tolist())
        seen += frame_ids.tolist()
    assert seen == list(range(12)) and len(loader) == 3


# ------------------------------------------------------------------------------------------------ one training step from a folder
NV = 200
RESOLUTIONS = [(15, 21, 9), (29, 41, 17), (57, 81, 33)]
SKINNER_GRID = (17, 29, 9)
RATIO = {'sdfRatio': 1., 'deformerRatio': 0.5, 'renderRatio': 1.}


def _write_training_folder(root, frames=5, S=128):
    """Five frames of 128 x 128: the camera SyntheticSequence builds for that size, masks = a centred ellipse around the projected body,
    noise images and normals, small smooth poses."""
    from PIL import Image
    import _smpl_ref as twin
    rng = np.random.default_rng(11)
    for sub in ("imgs", "masks", "normals"):
        os.makedirs(os.path.join(root, sub))
    f, Tz, Ty = 1.2 * S, 2.4, 0.15
    ys, xs = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing='ij')
    ellipse = ((xs - S / 2.0) / (f * 0.56 / Tz)) ** 2 + ((ys - (S / 2.0 - f * Ty / Tz)) / (f * 0.63 / Tz)) ** 2 < 1.0
    for i in range(frames):
        Image.fromarray(rng.integers(0, 256, (S, S, 3), dtype=np.uint8), "RGB").save(os.path.join(root, "imgs", f"{i}.png"))
        Image.fromarray(rng.integers(0, 256, (S, S, 3), dtype=np.uint8), "RGB").save(os.path.join(root, "normals", f"{i}.png"))
        Image.fromarray(ellipse.astype(np.uint8) * 255, "L").save(os.path.join(root, "masks", f"{i}.png"))
    t = np.linspace(0., 1., frames)[:, None]
    np.savez(os.path.join(root, "smpl_rec.npz"),
             poses=(0.12 * np.sin(2 * np.pi * t + rng.uniform(-3, 3, (1, 72))) * rng.uniform(-1, 1, (1, 72))).astype(np.float32),
             trans=(0.02 * np.sin(2 * np.pi * t + rng.uniform(-3, 3, (1, 3)))).astype(np.float32), shape=twin.golden_inputs(1, seed=50)[0][0])
    np.savez(os.path.join(root, "camera.npz"), fx=f, fy=f, cx=S / 2.0, cy=S / 2.0, quat=np.array([0., 0., 1., 0.]), T=np.array([0., Ty, Tz]))
    return twin.GOLDEN_SEED


def test_one_training_step_from_a_folder(tmp_path):
    from selfreconcode_amd.config import default_config
    from selfreconcode_amd.model import getOptNet
    from selfreconcode_amd.synthetic import LBS_BMAX, LBS_BMIN, synthetic_smpl_model
    root = tmp_path / "subject"
    os.makedirs(root)
    model_seed = _write_training_folder(str(root))
    conf = copy.deepcopy(default_config())
    conf['loss_coarse']['dct_weight'] = 0.                          # the DCT term needs windows of 30 frames; the folder has five
    conds_lens = {'deformer': conf.get_int('mlp_deformer.condlen'), 'renderer': conf.get_int('render_net.condlen')}
    torch.manual_seed(0)
    ds, loader = getDatasetAndLoader(str(root), conds_lens, 2, False, conf.get_int('train.num_workers'), True, True,
                                     conf.get_config('train.opt_camera'), device=DEV)
    assert ds.gender == 'neutral' and (ds.H, ds.W, ds.frame_num) == (128, 128, 5)
    ds.smpl_model = synthetic_smpl_model(NV, model_seed)
    net, _ = getOptNet(ds, 2, LBS_BMIN, LBS_BMAX, RESOLUTIONS, DEV, conf, skinner_resolution=SKINNER_GRID)
    assert os.path.isfile(os.path.join(root, "initial_skinner_1.pth"))
    frame_ids, outs = next(iter(loader))
    assert frame_ids.tolist() == [0, 1] and tuple(outs['img'].shape) == (2, 128, 128, 3) and 0.2 < float(outs['mask'].mean()) < 0.6
    opt = torch.optim.Adam([{'params': ds.learnable_weights()}, {'params': [p for p in net.parameters() if p.requires_grad]}], lr=1e-4)
    fids = frame_ids.to(DEV)
    loss = net(outs, 512, RATIO, fids)
    loss.backward()
    net.propagateTmpPsGrad(fids, RATIO)
    opt.step()
    assert torch.isfinite(loss).item() and net.TmpVs.shape[0] > 100
    assert all(torch.isfinite(p.grad).all().item() for p in net.parameters() if p.grad is not None)
    assert any(p.grad is not None for p in net.parameters())
    assert ds.poses.grad is not None and torch.isfinite(ds.poses.grad).all().item() and float(ds.poses.grad[:2].abs().max()) > 0
    assert ds.conds[0].grad is not None and torch.isfinite(ds.conds[0].grad).all().item()
    assert bool((ds.poses.grad[2:] == 0).all())                     # frames outside the batch receive exactly nothing
