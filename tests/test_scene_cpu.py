"""oracle/scene.py on the CPU: the one statement of the parity scene that the generators and the GPU tests both build from.  What is
pinned here is what the two sides rely on without looking: the frame window of dataset/dataset.py:128-147, that `draws` regenerates what
`KeyedDraws` handed the reference, that an observation depends on its frame id alone, the ground-truth mask, the parameter order Adam
sees, and that the module loads where there is no reference."""
import importlib
import sys
import pytest
import torch
from oracle import scene

F, H, W = 36, 64, 64


def _window_as_the_reference_writes_it(data, fids, batchsize, frame_num):
    """dataset/dataset.py:128-147 for an unsegmented video, frame by frame in plain Python."""
    rows, offs = [], []
    for f in fids.tolist():
        start = f - batchsize // 2
        end = start + batchsize
        if start < 0:
            start, end = 0, end - start
        if end > frame_num:
            start, end = start - (end - frame_num), frame_num
        rows.append(torch.stack([data[i] for i in range(start, end)]))
        offs.append(f - start)
    return torch.stack(rows), torch.tensor(offs)


@pytest.mark.parametrize("batchsize", [30, F])
def test_batchframe_window_is_the_references(batchsize):
    ds = scene.Sequence(F, H, W)
    fids = torch.tensor([0, 1, 14, 15, 20, 21, 35])
    for name in ("poses", "trans"):
        got, off = ds.get_batchframe_data(name, fids, batchsize)
        want, woff = _window_as_the_reference_writes_it(getattr(ds, name).detach(), fids, batchsize, F)
        assert got.shape[:2] == (fids.numel(), batchsize)
        assert torch.equal(got.detach(), want) and torch.equal(off, woff)
    starts = fids - ds.get_batchframe_data("trans", fids, batchsize)[1]
    assert int(starts.min()) == 0 and int(starts.max()) == F - batchsize           # both clamp edges are reached


@pytest.mark.parametrize("spare", [0, 64])
@pytest.mark.parametrize("six", [True, False])
def test_draws_regenerate_what_keyed_draws_handed_out(spare, six):
    base, k = 9000, 7
    kd = scene.KeyedDraws(base, k)
    handed = ([kd.rand(11)] if six else []) + [kd.rand((5,)), kd.randn_like(torch.zeros(6, 3)), kd.rand(6, 3), kd.rand(9), kd.randn_like(torch.zeros(4, 3, dtype=torch.float32))]
    names = scene.DRAW_NAMES if six else scene.DRAW_NAMES[1:]                       # no ray_select: the six-draw case minus the first
    assert [kind for kind, _ in kd.calls] == list(scene.DRAW_KINDS if six else scene.DRAW_KINDS[1:])
    rows = kd.shape_rows(pad_to=6)
    assert len(rows) == 6 and all(len(r) == 2 for r in rows)
    again = scene.draws(k, rows, base, spare)
    assert tuple(again) == tuple(names)
    for name, t in zip(names, handed):
        assert again[name].shape == (t.shape[0] + spare,) + t.shape[1:] and again[name].dtype == t.dtype
        assert torch.equal(again[name][:t.shape[0]], t), name
    other = scene.draws(k + 1, rows, base, spare)
    assert not torch.equal(other[names[0]], again[names[0]])                        # keyed by the iteration
    assert 0. <= float(handed[0].min()) and float(handed[0].max()) <= 1.           # a `rand`


def test_an_observation_depends_on_its_frame_alone():
    cache = {}
    batch = scene.noise_observations([5, 30, 5], H, W, cache=cache)
    cached = scene.noise_observations(torch.tensor([30]), H, W, cache=cache)
    alone = scene.noise_observations([30], H, W)
    for key in ("img", "normal", "mask"):
        assert torch.equal(alone[key][0], batch[key][1]) and torch.equal(cached[key][0], batch[key][1]), key
        assert torch.equal(batch[key][0], batch[key][2])
    assert not torch.equal(batch["img"][0], batch["img"][1])
    assert batch["img"].shape == (3, H, W, 3) and batch["mask"].shape == (3, H, W)
    assert float(batch["normal"][:, ::5].abs().max()) == 0. and float(batch["normal"][:, 1::5].abs().max()) > 0.
    assert torch.equal(batch["mask"][0], scene.elliptic_mask(H, W))


def test_elliptic_mask_is_the_mask_the_goldens_were_made_on():
    """No committed golden stores the mask itself (iteration.npz ran on an all-ones mask), so: the pixel count and the four extreme
    pixels with their outer neighbours, computed with the generators' former `mask_image` before it moved here."""
    m = scene.elliptic_mask(64, 64)
    assert m.shape == (64, 64) and m.dtype == torch.float32 and float(m.sum()) == 1300.0
    for inside, outside in (((7, 32), (6, 32)), ((50, 32), (51, 32)), ((28, 14), (28, 13)), ((28, 50), (28, 51))):
        assert float(m[inside]) == 1.0 and float(m[outside]) == 0.0, (inside, outside)
    assert float(scene.elliptic_mask(540, 540).sum()) == 92983.0


def test_both_camera_spellings_are_the_same_tensors_and_adam_sees_the_reference_order():
    ds = scene.Sequence(F, H, W)
    cp = ds.camera_params
    assert cp['focal_length'] is ds.focal and cp['princeple_points'] is ds.princ and cp['world2cam_coord_trans'] is ds.T
    want = [ds.conds[0], ds.conds[1], ds.focal, ds.princ, ds.T, ds.poses, ds.trans]
    for got in (ds.learnable_weights(), ds.learnable()):
        assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    assert all(t.is_leaf and t.requires_grad for t in want) and not ds.R.requires_grad
    assert ds.frame_num == F and ds.video_segmented_index == []
    focal, princ, R, T, h, w = ds.get_camera_parameters(3)
    assert focal.shape == (3, 2) and princ.shape == (3, 2) and R.shape == (3, 3, 3) and T.shape == (3, 3) and (h, w) == (H, W)
    loose = scene.Sequence(F, H, W, learn_cam=("focal",))
    assert [a is b for a, b in zip(loose.learnable_weights(), [loose.conds[0], loose.conds[1], loose.focal, loose.poses, loose.trans])] == [True] * 5
    assert not loose.princ.requires_grad and not loose.T.requires_grad
    stored = dict(poses=torch.zeros(4, 24, 3), trans=torch.ones(4, 3), dcond=torch.zeros(4, 128), rcond=torch.zeros(4, 256), focal=torch.tensor([58., 60.]),
                  princ=torch.tensor([23., 33.5]), T=torch.tensor([0.03, -0.1, 2.5]), R=torch.eye(3))
    given = scene.Sequence(4, 64, 48, tensors=stored)
    assert torch.equal(given.trans.detach(), stored["trans"]) and given.trans is not stored["trans"] and torch.equal(given.focal.detach(), stored["focal"])
    assert given.R.shape == (1, 3, 3) and given.get_camera_parameters(2)[4:] == (64, 48)


def test_scene_loads_where_there_is_no_reference(monkeypatch):
    from oracle import ref_harness

    def no_reference():
        raise RuntimeError("the reference is not on this machine")
    monkeypatch.setattr(ref_harness, "load_reference", no_reference)
    monkeypatch.setattr(sys.modules["oracle"], "scene", scene)                      # (restored afterwards: the import below rebinds it)
    for name in [n for n in sys.modules if n in ("oracle.scene", "oracle.gen_iteration_golden", "oracle.ref_scene")]:
        monkeypatch.delitem(sys.modules, name)
    fresh = importlib.import_module("oracle.scene")
    assert fresh.Sequence(4, 8, 8).frame_num == 4
    assert "oracle.gen_iteration_golden" not in sys.modules and "oracle.ref_scene" not in sys.modules
