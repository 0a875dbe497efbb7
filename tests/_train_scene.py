"""The miniature capture folder and training runs the driver tests share (tests/test_train_gpu.py, tests/test_infer_cli_gpu.py): five
frames of 128 x 128 with the 200-vertex synthetic body model, three epochs that visit all three stages.  The folder is written once
per session; every run is made once, by the first test that asks for it, and then only read."""
import copy
import os
import random

import numpy as np
import torch

import _smpl_ref as twin

DEV = "cuda:0"
NV = 200
PYRAMID = [(15, 21, 9), (29, 41, 17), (57, 81, 33)]
RESOLUTIONS = {'coarse': PYRAMID, 'medium': PYRAMID, 'fine': PYRAMID}
SKINNER_GRID = (17, 29, 9)
FRAMES, SIZE = 5, 128
SEED = 0


def write_training_folder(root, frames=FRAMES, S=SIZE):
    """Frames of S x S: the camera SyntheticSequence builds for that size, masks = a centred ellipse around the projected body, noise
    images and normals, small smooth poses (the recipe of tests/test_scene_dataset_gpu.py).  -> the body model's seed."""
    from PIL import Image
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


def train_conf():
    """default_config() cut down to three epochs over the three stages: the shipped pre-fit, batch sizes 2 / 2 / 1, a remesh every
    second iteration, 256 pixels per frame, no DCT term (its windows need 30 frames), one milestone."""
    from selfreconcode_amd.config import default_config
    conf = copy.deepcopy(default_config())
    t = conf['train']
    t['nepoch'], t['sample_pix_num'], t['shuffle'] = 2, 256, True
    t['scheduler']['milestones'] = [1]
    t['medium']['start_epoch'], t['fine']['start_epoch'] = 1, 2
    for stage, bs in (('coarse', 2), ('medium', 2), ('fine', 1)):
        t[stage]['point_render']['batch_size'] = bs
        t[stage]['point_render']['remesh_intersect'] = 2
        conf['loss_' + stage]['dct_weight'] = 0.
    conf['loss_fine']['sample_pix_num'] = 256
    return conf


class Run:
    """What the tests read of one train() call; the network itself is dropped (`net_state` keeps the few numbers asked of it)."""

    def __init__(self, result, text):
        self.rows, self.lines, self.save_root, self.next_epoch, self.stalls, self.text = result.rows, result.lines, result.save_root, result.next_epoch, result.stalls, text
        net = result.optNet
        self.net_state = {'point_radius': net.point_radius, 'remesh_intersect': net.remesh_intersect, 'draw': getattr(net, 'draw', False),
                          'stage_conf': dict(net.conf)}


_SESSION = {}


def folder(tmp_path_factory):
    """The capture folder, after the first run in it (which fits the SDF, builds the skinner and leaves both caches in the folder).
    -> (root, that run)"""
    if 'root' not in _SESSION:
        root = str(tmp_path_factory.mktemp("train_scene") / "subject")
        os.makedirs(root)
        _SESSION['model_seed'] = write_training_folder(root)
        _SESSION['root'] = root
        _SESSION['first'] = run(tmp_path_factory, 'first', smpl=True)
    return _SESSION['root'], _SESSION['first']


def run(tmp_path_factory, name, conf=None, smpl=False, **kwargs):
    """train() into the save folder `name`, seeded with SEED, once per session.  Later calls with the same name return the first result."""
    from selfreconcode_amd.synthetic import LBS_BMAX, LBS_BMIN, synthetic_smpl_model
    from selfreconcode_amd.train import train
    key = ('run', name)
    if key not in _SESSION:
        root = _SESSION['root'] if smpl else folder(tmp_path_factory)[0]
        random.seed(SEED)
        torch.manual_seed(SEED)
        text = []
        result = train(root, conf if conf is not None else train_conf(), kwargs.pop('save_folder', name), device=DEV, resolutions=RESOLUTIONS,
                       smpl_model=synthetic_smpl_model(NV, _SESSION['model_seed']) if smpl else None, skinner_resolution=SKINNER_GRID,
                       bmins=LBS_BMIN, bmaxs=LBS_BMAX, out=lambda *a, **k: text.append(' '.join(str(x) for x in a)), **kwargs)
        _SESSION[key] = Run(result, text)
    return _SESSION[key]


def checkpoint_tensors(path):
    """{dotted name: tensor} of every tensor in a checkpoint written by save_model, plus its epoch."""
    saved = torch.load(path, map_location='cpu', weights_only=False)
    out = {'model_state_dict.' + k: v for k, v in saved['model_state_dict'].items()}
    out.update({k: v for k, v in saved.items() if torch.is_tensor(v)})
    return out, saved['epoch']
