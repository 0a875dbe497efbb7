"""`python -m selfreconcode_amd.infer` on the folder a training run left (tests/_train_scene.py): the files it writes are, byte for byte,
those of a direct infer_export.export_frames call on a network built and loaded by hand; errors.txt parses."""
import os
import re

import pytest
import torch

import _train_scene as ts

pytestmark = pytest.mark.gpu
FRAMES = 2                                 # --frames 2 at batch size 1: batches 0, 1 and 2 (infer.py:133 stops at the first index > frames)
VISITED = (0, 1, 2)


def _tree(root, subs=('meshs', 'def1meshs', 'colors')):
    out = {}
    for name in ('tmp.ply', 'errors.txt'):
        with open(os.path.join(root, name), 'rb') as fh:
            out[name] = fh.read()
    for sub in subs:
        for fn in sorted(os.listdir(os.path.join(root, sub))):
            with open(os.path.join(root, sub, fn), 'rb') as fh:
                out[sub + '/' + fn] = fh.read()
    return out


@pytest.fixture(scope="module")
def direct(tmp_path_factory):
    """export_frames called directly, without and with colours, on a network put together as infer.py does it."""
    from selfreconcode_amd.config import load_config
    from selfreconcode_amd.dataset import getDatasetAndLoader
    from selfreconcode_amd.infer_export import export_frames
    from selfreconcode_amd.model import getOptNet
    from selfreconcode_amd.posed import FULL_RATIO as RATIO
    from selfreconcode_amd.utils.checkpoint import load_model
    root, first = ts.folder(tmp_path_factory)
    conf = load_config(os.path.join(first.save_root, 'config.conf'))
    condlen = {'deformer': conf.get_int('mlp_deformer.condlen'), 'renderer': conf.get_int('render_net.condlen')}
    ds, _ = getDatasetAndLoader(root, condlen, 1, False, 0, False, False, False, device=ts.DEV)
    net, _ = getOptNet(ds, 1, None, None, ts.PYRAMID, ts.DEV, conf)
    net, ds = load_model(os.path.join(first.save_root, 'latest.pth'), net, ds, ts.DEV)
    net.dataset = ds
    net.eval()
    TmpVs, Tmpfs = net.discretizeSDF(RATIO, None, 0.)
    trees = {}
    for color in (False, True):
        out_root = str(tmp_path_factory.mktemp("direct_color" if color else "direct_plain"))
        export_frames(net, TmpVs, Tmpfs, [(torch.tensor([i]), ds.batch([i])) for i in VISITED], out_root, RATIO, color=color)
        trees[color] = _tree(out_root)
    return first.save_root, trees


def test_infer_without_colours_writes_what_export_frames_writes(direct):
    from selfreconcode_amd import infer
    rec_root, trees = direct
    said = []
    assert infer.main(['--gpu-ids', '0', '--rec-root', rec_root, '--frames', str(FRAMES), '--nColor', '--nV'],
                      out=lambda *a, **k: said.append(a), resolutions=ts.PYRAMID) == 0
    got = _tree(rec_root)
    assert set(got) == set(trees[False]) and not [k for k in got if got[k] != trees[False][k]]
    assert sorted(k for k in got if k.startswith('meshs/')) == sorted(f'meshs/{i}.{e}' for i in VISITED for e in ('npy', 'png'))
    assert not any(k.startswith('colors/') for k in got)
    assert sum('not written' in str(a[0]) for a in said) == 1 and [a[0] for a in said if isinstance(a[0], int)] == list(VISITED)
    lines = got['errors.txt'].decode().splitlines()
    assert lines[0] == '      mask' and len(lines) == 2 + len(VISITED)
    for i, line in zip(VISITED, lines[1:]):
        m = re.fullmatch(r' *(\d+): (\d\.\d{4})', line)
        assert m and int(m.group(1)) == i and 0. <= float(m.group(2)) <= 1.
    m = re.fullmatch(r'mask mean: (\d\.\d{4}), max: (\d\.\d{4}), min: (\d\.\d{4}), maxinds:((?:\d+ )+)', lines[-1])
    assert m and float(m.group(3)) <= float(m.group(1)) <= float(m.group(2)) and sorted(int(x) for x in m.group(4).split()) == [0, 1, 2]


def test_infer_with_colours_writes_what_export_frames_writes(direct):
    from selfreconcode_amd import infer
    rec_root, trees = direct
    assert infer.main(['--rec-root', rec_root, '--frames', str(FRAMES)], out=lambda *a, **k: None, resolutions=ts.PYRAMID) == 0
    got = _tree(rec_root)
    assert set(got) == set(trees[True]) and not [k for k in got if got[k] != trees[True][k]]
    assert sorted(k for k in got if k.startswith('colors/')) == [f'colors/{i}.png' for i in VISITED]
