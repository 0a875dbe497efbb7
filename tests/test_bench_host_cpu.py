"""Host logic of bench.py and of the one-launch optimizer that needs no GPU: the frames-per-rank rule of the two scaling modes, the
driver's contract on the command line (defaults that finish within minutes, the flags the driver passes), and FusedAdam's refusals
(it has no CPU path: it must say so, not fall back)."""
import argparse
import importlib
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(**kw):
    base = dict(scaling="weak", frames_per_gpu=0, global_frames=8)
    base.update(kw)
    return argparse.Namespace(**base)


def test_frames_per_rank_rules():
    bench = importlib.import_module("bench")
    # weak scaling: the stage's batch per rank, whatever the world size (configs[1]: 3 frames; the fine stage: 1)
    for world in (1, 2, 8):
        assert bench.frames_per_rank("coarse", _args(), world) == 3
        assert bench.frames_per_rank("fine", _args(), world) == 1
    # --frames-per-gpu 1 at N = 8 is configs[2]
    assert bench.frames_per_rank("coarse", _args(frames_per_gpu=1), 8) == 1
    # strong scaling: a fixed global batch split over the ranks, and a refusal when it does not divide
    assert [bench.frames_per_rank("coarse", _args(scaling="strong"), w) for w in (1, 2, 4, 8)] == [8, 4, 2, 1]
    with pytest.raises(SystemExit):
        bench.frames_per_rank("coarse", _args(scaling="strong"), 3)
    assert set(bench.STAGES) == {"coarse", "fine"} and bench.STAGES["coarse"] == dict(frames=3, rays=2048) and bench.STAGES["fine"] == dict(frames=1, rays=6144)


def test_bench_command_line_contract():
    """`python bench.py --help` works without a GPU and names the flags the driver uses; the defaults are one GPU and a step count that
    finishes within minutes."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--gpus", "--steps", "--warmup", "--scaling", "--frames-per-gpu", "--global-frames", "--no-cpu-baseline", "--simulate-world",
                 "--full", "--dump-outputs"):
        assert flag in r.stdout, flag
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'add_argument("--gpus", type=int, default=1)' in src
    assert 'add_argument("--steps", type=int, default=30)' in src and 'add_argument("--warmup", type=int, default=5)' in src


def test_dump_outputs_names_dtypes_and_sampling(tmp_path):
    """`--dump-outputs`: one .npy per array in float32 / float64, the loss terms of net.info, parameters and gradients by name, and an
    array above the element cap written as the same seeded sample every time."""
    import numpy as np
    bench = importlib.import_module("bench")

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(3, 2)
            self.info = {"rayInfo": (7, torch.tensor(3)), "color_loss": torch.tensor(0.5), "pc_loss": {"mask_loss": torch.tensor(0.25)}, "remesh": None}
            self.TmpVs = torch.arange((bench.DUMP_MAX_ELEMS // 3 + 2) * 3, dtype=torch.float32).view(-1, 3)
            self.Tmpfs = torch.tensor([[0, 1, 2]])

    class Data:
        conds = [torch.ones(4, 2, requires_grad=True)]
        camera_params = {"focal_length": torch.ones(2, dtype=torch.float64, requires_grad=True)}
        poses, trans = torch.zeros(4, 3, requires_grad=True), torch.zeros(4, 3)

        def learnable_weights(self):
            return self.conds + list(self.camera_params.values()) + [self.poses]

    net, ds = Net(), Data()
    net.lin.weight.grad = torch.full((2, 3), 2.0)
    names = bench.dump_outputs(str(tmp_path / "a"), net, ds, torch.tensor(1.5))
    bench.dump_outputs(str(tmp_path / "b"), net, ds, torch.tensor(1.5))
    for n in ("loss", "info.rayInfo", "info.color_loss", "info.pc_loss.mask_loss", "param.lin.weight", "grad.lin.weight", "param.data.conds0",
              "param.data.camera.focal_length", "param.data.poses", "template.TmpVs", "template.Tmpfs"):
        assert n in names and (tmp_path / "a" / (n + ".npy")).is_file(), n
    assert not (tmp_path / "a" / "info.remesh.npy").exists()
    ld = lambda d, n: np.load(str(tmp_path / d / (n + ".npy")))
    assert ld("a", "loss").dtype == np.float32 and float(ld("a", "loss")) == 1.5
    assert ld("a", "info.rayInfo").dtype == np.float64 and ld("a", "info.rayInfo").tolist() == [7.0, 3.0]
    assert ld("a", "param.data.camera.focal_length").dtype == np.float64 and ld("a", "template.Tmpfs").dtype == np.float64
    assert (ld("a", "grad.lin.weight") == 2.0).all() and ld("a", "param.lin.weight").shape == (2, 3)
    v = ld("a", "template.TmpVs")
    assert v.shape == (bench.DUMP_MAX_ELEMS,) and (np.diff(v) > 0).all() and (v == ld("b", "template.TmpVs")).all()
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_MAX_BYTES + 4096 * len(names)


def test_fused_adam_refuses_what_it_does_not_implement():
    from selfreconcode_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(NotImplementedError):
        FusedAdam([p], lr=1e-3, weight_decay=0.1)
    with pytest.raises(NotImplementedError):
        FusedAdam([p], lr=1e-3, amsgrad=True)
    opt = FusedAdam([p], lr=1e-3)
    assert opt.step() is None                                  # no gradient anywhere: nothing to do, no launch
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="GPU"):             # a CPU parameter: no silent fallback to a host loop
        opt.step()
    # the state layout is torch.optim.Adam's: its state_dict loads
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=2e-3)
    opt2 = FusedAdam([torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    opt2.load_state_dict(ref.state_dict())
    assert opt2.param_groups[0]["lr"] == 2e-3
