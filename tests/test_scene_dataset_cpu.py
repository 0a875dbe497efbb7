"""The host half of dataset.SceneDataset against the reference's own dataset/dataset.py, recorded by tools/gen_scene_dataset_golden.py on
the committed capture folder tests/golden/scene_folder (12 frames of 6 x 10): reading the folder, its errors, the conditioning codes,
the frame windows, the samplers, the loader and the stage switch.  No GPU: the tables live on the CPU here."""
import os
import random

import numpy as np
import pytest
import torch

from selfreconcode_amd.dataset import (ClipSampler, FrameLoader, RandomSampler, SceneDataset, getDatasetAndLoader, make_conds,
                                       read_scene_folder)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLDER = os.path.join(ROOT, "tests", "golden", "scene_folder")
CONDS_LENS = {'deformer': 8, 'renderer': 16}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "scene_dataset.npz")) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def scene():
    return read_scene_folder(FOLDER)


@pytest.fixture(scope="module")
def ds():
    torch.manual_seed(0)
    return SceneDataset(FOLDER, CONDS_LENS, device="cpu")


def test_folder_header(scene, gold):
    assert scene['frame_num'] == 12 == int(gold['frame_num']) and (scene['H'], scene['W']) == (6, 10) == (int(gold['H']), int(gold['W']))
    assert scene['gender'] == 'male' == str(gold['gender']) and scene['video_segmented_index'] == [7] == gold['video_segmented_index'].tolist()
    assert [os.path.basename(p) for p in scene['img_ns']] == [f"{i}.png" for i in range(12)]
    assert [os.path.basename(p) for p in scene['mask_ns']] == [f"{i}.png" for i in range(12)] and len(scene['normal_ns']) == 12
    for key, value in scene['camera'].items():
        assert value.dtype == np.float32 and np.array_equal(value, gold['camera_' + key]), key
    assert scene['camera']['focal_length'].tolist() == [12.5, 12.25] and scene['camera']['princeple_points'].tolist() == [5.25, 2.5]
    for key in ('poses', 'trans', 'shape'):
        assert scene[key].dtype == np.float32 and np.array_equal(scene[key], gold[key]), key
    assert scene['poses'].shape == (12, 24, 3) and scene['trans'].shape == (12, 3) and scene['shape'].shape == (10,)


def test_decoded_bytes_give_the_reference_frames(scene, gold):
    """The reference's expressions (dataset.py:88, 97, 101-102) in numpy on the decoded bytes: img stays B, G, R, the normal is reversed
    to R, G, B, a mask pixel is set when any channel is."""
    img, normal, mask = scene['img'], scene['normal'], scene['mask']
    assert img.dtype == normal.dtype == mask.dtype == np.uint8 and set(np.unique(mask)) == {0, 1}
    assert np.array_equal((img.astype(np.float32) / 255. - 0.5) * 2, gold['img'])
    assert np.array_equal(2. * normal[..., ::-1].astype(np.float32) / 255. - 1., gold['normal'])
    assert np.array_equal(mask.astype(np.float32), gold['mask'])
    assert not np.array_equal((img[..., ::-1].astype(np.float32) / 255. - 0.5) * 2, gold['img'])       # (the channel order is visible in the data)
    assert 0.05 < mask.mean() < 0.95


def _write_folder(root, names, size=(4, 6), masks=None, normals=(), sizes=None):
    """A capture folder with images `names` (e.g. '0.png'), masks for the stems `masks` (default: all) and normals for `normals`."""
    from PIL import Image
    rng = np.random.default_rng(5)
    for sub in ("imgs", "masks", "normals"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    stems = [n.split('.')[0] for n in names]

    def picture(stem):
        h, w = (sizes or {}).get(stem, size)
        return Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB")
    for name in names:
        picture(name.split('.')[0]).save(os.path.join(root, "imgs", name))
    for stem in (stems if masks is None else masks):
        Image.fromarray(rng.integers(0, 2, size, dtype=np.uint8) * 255, "L").save(os.path.join(root, "masks", stem + ".png"))
    for stem in normals:
        picture("normal").save(os.path.join(root, "normals", stem + ".png"))
    n = len(names)
    np.savez(os.path.join(root, "smpl_rec.npz"), poses=np.zeros((n, 72), np.float32), trans=np.zeros((n, 3), np.float32), shape=np.zeros(10, np.float32))
    np.savez(os.path.join(root, "camera.npz"), fx=10., fy=10., cx=3., cy=2., quat=np.array([1., 0., 0., 0.]), T=np.array([0., 0., 2.]))
    return str(root)


def test_folder_errors_name_the_file(tmp_path):
    with pytest.raises(ValueError, match=r"masks.1\.png"):
        read_scene_folder(_write_folder(tmp_path / "a", ["0.png", "1.png", "2.png"], masks=["0", "2"]))
    with pytest.raises(ValueError, match=r"imgs.3\.png"):
        read_scene_folder(_write_folder(tmp_path / "b", ["0.png", "1.png", "3.png"]))
    with pytest.raises(ValueError, match=r"imgs.1\.png"):
        read_scene_folder(_write_folder(tmp_path / "c", ["0.png", "1.png", "2.png"], sizes={"1": (4, 7)}))
    with pytest.raises(ValueError, match=r"normals.1\.png"):
        read_scene_folder(_write_folder(tmp_path / "d", ["0.png", "1.png", "2.png"], normals=["0", "2"]))


def test_sixteen_bit_files_are_refused(tmp_path):
    from PIL import Image
    root = _write_folder(tmp_path / "e", ["0.png", "1.png"])
    Image.fromarray((np.arange(24, dtype=np.uint16) * 1000).reshape(4, 6)).save(os.path.join(root, "imgs", "1.png"))
    with pytest.raises(ValueError, match=r"imgs.1\.png"):
        read_scene_folder(root)


def test_defaults_and_mixed_extensions(tmp_path):
    """.jpg and .png side by side sort by integer stem (names and shapes only: no value of a JPEG is pinned); without the optional keys
    the gender is neutral and there is no split; without normals/ there is no normal."""
    scene = read_scene_folder(_write_folder(tmp_path / "f", ["0.jpg", "1.png", "2.jpg"] + [f"{i}.png" for i in range(3, 11)]))
    assert [os.path.basename(p) for p in scene['img_ns']] == ["0.jpg", "1.png", "2.jpg"] + [f"{i}.png" for i in range(3, 11)]
    assert [os.path.basename(p) for p in scene['mask_ns']] == [f"{i}.png" for i in range(11)]
    assert scene['img'].shape == (11, 4, 6, 3) and scene['mask'].shape == (11, 4, 6) and scene['normal'] is None and scene['normal_ns'] is None
    assert scene['gender'] == 'neutral' and scene['video_segmented_index'] == []


def test_conds_after_a_seed_are_the_references(ds, gold):
    """Equal to the reference's codes within the float32 dot-product bound 4 K 2^-24 max_row sum |a||b| (K = F // 5 = 2 terms; the bound
    is computed in float64 from the golden's own factors): the CPU BLAS of another machine may order the sum differently.
    Observed where the golden was made: 0 (bit-equal) for both codes, against bounds of 4.5e-8 and 5.2e-8."""
    assert ds.cond_ns == ['deformer', 'renderer'] == gold['cond_names'].tolist()
    torch.manual_seed(0)
    again, _ = make_conds(CONDS_LENS, 12)
    for k, length in enumerate(CONDS_LENS.values()):
        a, b = gold[f'cond_coef_{k}'].astype(np.float64), gold['dct_space'].astype(np.float64)
        K = a.shape[1]
        assert K == 12 // 5
        bound = 4 * K * 2.0 ** -24 * (np.abs(a) @ np.abs(b)).max()
        got = ds.conds[k].detach().numpy()
        err = np.abs(got.astype(np.float64) - gold[f'cond_{k}']).max()
        print(f"cond {k}: max |difference| {err:.3e}, bound {bound:.3e}")
        assert got.shape == (12, length) and err <= bound
        assert ds.conds[k].is_leaf and ds.conds[k].requires_grad and torch.equal(again[k], ds.conds[k].detach())


def test_tables_are_leaves_and_albedo_is_refused(ds):
    assert ds.root == FOLDER and len(ds) == ds.frame_num == 12 and (ds.H, ds.W) == (6, 10) and ds.gender == 'male' and ds.smpl_model is None
    assert ds.video_segmented_index == [7] and ds.require_albedo is False
    for t in [ds.poses, ds.trans, ds.shape, *ds.conds, *ds.camera_params.values()]:
        assert t.is_leaf and t.dtype == torch.float32
    assert list(ds.camera_params) == ['focal_length', 'princeple_points', 'cam2world_coord_quat', 'world2cam_coord_trans']
    with pytest.raises(NotImplementedError):
        ds.require_albedo = True
    # the stores: one padded row per frame, 16-byte pitch, zero padding
    assert tuple(ds.img_u8.shape) == (12, 192) and tuple(ds.normal_u8.shape) == (12, 192) and tuple(ds.mask_u8.shape) == (12, 64)
    assert ds.resident_bytes == 12 * (192 * 2 + 64) and not ds.img_u8[:, 180:].any() and not ds.mask_u8[:, 60:].any()
    with pytest.raises(RuntimeError):                                # no CPU fallback for the expansion
        ds.batch([0])


def test_frame_windows(ds, gold):
    fids = torch.from_numpy(gold['window_fids'])
    keep = fids.clone()
    for tag, split in (("unsplit", []), ("split", [7])):
        ds.video_segmented_index = split
        windows, offsets = ds.get_batchframe_data('poses', fids, int(gold['window']))
        assert np.array_equal(windows.detach().numpy(), gold[f'window_{tag}']) and np.array_equal(offsets.numpy(), gold[f'window_{tag}_offsets'])
        assert torch.equal(fids, keep)
    assert not np.array_equal(gold['window_unsplit_offsets'], gold['window_split_offsets'])          # (the split changes the answer here)
    ds.video_segmented_index = [7]
    with pytest.raises(ValueError):
        ds.get_batchframe_data('poses', fids, 5)                      # the second segment has five frames
    ds.video_segmented_index = [4, 7]
    with pytest.raises(NotImplementedError):
        ds.get_batchframe_data('poses', fids, 2)
    ds.video_segmented_index = []
    with pytest.raises(ValueError):
        ds.get_batchframe_data('poses', fids, 12)
    ds.video_segmented_index = [7]
    assert torch.equal(fids, keep)


def test_grad_and_camera_parameters_on_the_cpu(ds, gold):
    rows = ds.get_grad_parameters(torch.from_numpy(gold['grad_ids']))
    assert len(rows) == 4
    for name, row in zip(("poses", "trans"), rows):
        assert np.array_equal(row.detach().numpy(), gold['grad_' + name])
    focal, centre, R, T, H, W = ds.get_camera_parameters(2)
    assert np.array_equal(focal.numpy(), gold['cam_focal']) and np.array_equal(centre.numpy(), gold['cam_centre'])
    assert np.array_equal(T.numpy(), gold['cam_T']) and [H, W] == gold['cam_hw'].tolist()
    assert np.abs(R.numpy() - gold["cam_R"]).max() <= 8 * 2.0 ** -24          # same formula; at most seven float32 roundings of numbers <= 1 per entry
    torch.manual_seed(1)
    one = SceneDataset(FOLDER, {'deformer': 4}, device="cpu").get_grad_parameters([1, 2])
    assert len(one) == 4 and one[3] is None and tuple(one[2].shape) == (2, 4)


def test_samplers_give_the_references_id_lists(ds, gold):
    cases = {"random_1": (RandomSampler, 1), "random_3": (RandomSampler, 3), "clip_4": (ClipSampler, 4)}
    for tag, (cls, arg) in cases.items():
        for shuffle in (True, False):
            sampler = cls(ds, arg, shuffle)
            random.seed(0); torch.manual_seed(0)
            key = f"sampler_{tag}_{'shuffle' if shuffle else 'ordered'}"
            assert list(iter(sampler)) == gold[key].tolist(), key
            assert len(sampler) == int(gold[key + "_len"]) == len(gold[key])
    assert gold['sampler_random_1_shuffle'].tolist() != list(range(12)) and sorted(gold['sampler_random_1_shuffle'].tolist()) == list(range(12))


class _Frames:
    """A dataset stand-in whose batch() needs no GPU."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def batch(self, ids):
        return {'ids': list(ids)}


@pytest.mark.parametrize("batch_size", [1, 2, 3, 5])
def test_frame_loader_length_and_short_last_batch(batch_size):
    frames = _Frames(12)
    sampler = RandomSampler(frames, 1, False)
    loader = FrameLoader(frames, batch_size, sampler, num_workers=4)
    got = list(loader)
    assert len(got) == len(loader) == -(-12 // batch_size)
    assert all(ids.dtype == torch.int64 and ids.device.type == 'cpu' and ids.dim() == 1 and outs['ids'] == ids.tolist() for ids, outs in got)
    assert [len(ids) for ids, _ in got] == [batch_size] * (12 // batch_size) + ([12 % batch_size] if 12 % batch_size else [])
    assert torch.cat([ids for ids, _ in got]).tolist() == list(range(12))
    other = loader.with_batch_size(4)
    assert other.dataset is frames and other.sampler is sampler and other.batch_size == 4 and other.num_workers == 4 and loader.batch_size == batch_size


def test_stage_switch_remakes_either_loader():
    import torch.nn as nn
    from selfreconcode_amd.config import default_config
    from selfreconcode_amd.MCAcc import Seg3dLossless
    from selfreconcode_amd.model.optim_network import OptimNetwork
    from selfreconcode_amd.synthetic import STAGE_RESOLUTIONS
    from selfreconcode_amd.utils.checkpoint import set_hierarchical_config
    conf = default_config()
    engine = Seg3dLossless(query_func=None, b_min=[-1., -1.2, -0.5], b_max=[1., 1.2, 0.5], resolutions=STAGE_RESOLUTIONS['coarse'][:2],
                           align_corners=False, balance_value=0.0, use_cuda_impl=False)
    net = OptimNetwork(nn.Identity(), nn.Identity(), engine, None, nn.Identity(), conf=conf.get_config('loss_coarse'))
    frames = _Frames(12)
    loader = FrameLoader(frames, conf.get_int('train.coarse.point_render.batch_size'), RandomSampler(frames, 1, True), num_workers=4)
    _, loader2 = set_hierarchical_config(conf, 'medium', net, loader, STAGE_RESOLUTIONS['medium'][:2])
    assert isinstance(loader2, FrameLoader) and loader2 is not loader and loader2.batch_size == conf.get_int('train.medium.point_render.batch_size') == 2
    assert loader2.dataset is frames and loader2.sampler is loader.sampler and loader.batch_size == 3
    tds = torch.utils.data.TensorDataset(torch.arange(12))
    plain = torch.utils.data.DataLoader(tds, 3, sampler=torch.utils.data.SequentialSampler(tds), num_workers=0)
    _, plain2 = set_hierarchical_config(conf, 'fine', net, plain, STAGE_RESOLUTIONS['fine'][:2])
    assert type(plain2) is torch.utils.data.DataLoader and plain2.batch_size == 1 and plain2.dataset is tds
    assert set_hierarchical_config(conf, 'fine', net, None, STAGE_RESOLUTIONS['fine'][:2])[1] is None


def test_learnable_weights_order_under_the_shipped_configuration(gold):
    from selfreconcode_amd.config import default_config
    conf = default_config()
    torch.manual_seed(0)
    ds, loader = getDatasetAndLoader(FOLDER, CONDS_LENS, 3, conf.get_bool('train.shuffle'), conf.get_int('train.num_workers'),
                                     conf.get_bool('train.opt_pose'), conf.get_bool('train.opt_trans'), conf.get_config('train.opt_camera'), device="cpu")
    names = {id(t): n for n, t in list(zip(ds.cond_ns, ds.conds)) + list(ds.camera_params.items())
             + [("shape", ds.shape), ("poses", ds.poses), ("trans", ds.trans)]}
    got = [names[id(t)] for t in ds.learnable_weights()]
    assert got == gold['learnable_names'].tolist()
    assert got == ['deformer', 'renderer', 'focal_length', 'princeple_points', 'world2cam_coord_trans', 'poses', 'trans']
    assert isinstance(loader, FrameLoader) and loader.dataset is ds and isinstance(loader.sampler, RandomSampler) and loader.sampler.intersect == 1
    assert loader.batch_size == 3 and loader.num_workers == 4 and len(loader) == 4
    ds.opt_camera_params(False)
    assert [names[id(t)] for t in ds.learnable_weights()] == ['deformer', 'renderer', 'poses', 'trans']
    ds.opt_camera_params(True)
    assert len(ds.learnable_weights()) == 8


def test_python_mirrors_of_the_frame_constants():
    import ctypes
    import re
    from selfreconcode_amd import _lib, ops
    txt = open(os.path.join(ROOT, "include", "selfrecon_hip.h")).read()
    assert int(re.search(r"#define\s+SR_FRAMES_MAX_BATCH\s+(\d+)", txt).group(1)) == _lib.SR_FRAMES_MAX_BATCH == ops.FRAMES_MAX_BATCH == 16
    assert ctypes.sizeof(_lib.SrFrameIds) == 4 * _lib.SR_FRAMES_MAX_BATCH            # sr_frame_ids: int32_t id[SR_FRAMES_MAX_BATCH]
    assert [ops.frames_pitch(n) for n in (1, 16, 17, 105, 180, 384)] == [16, 16, 32, 112, 192, 384]
