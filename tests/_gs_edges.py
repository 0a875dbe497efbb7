"""Inputs and float64 expectations of tests/test_ext_ops_edges_gpu.py (the 3-D sampler away from its N == 1, dense, one-pass corridor).
Everything here runs on the CPU; tests/test_ext_ops_edges_cpu.py checks the helpers themselves.

Every case is a dict of float32 CPU tensors -- inp [N,C,D,H,W], grid [N,Do,Ho,Wo,3], go (grad_output), goi (grad_output_input), gog
(grad_output_grid) -- whose values the tests cast to the type under test, so one float64 oracle run serves all of a case's variants."""
import functools
import numpy as np
import torch
from oracle import torch_oracle as orc
from oracle import fixtures as fx

TOL = {torch.float32: 8e-6, torch.float64: 1e-12}      # of the output scale: the reference pin's own numbers (tests/test_gs_reference_pin.py)
LAUNCH_CAP = 2048 * 256                                # sr_stream_grid: items one pass of a capped launch covers
POINT_KEYS = ("out", "gg", "dg", "dgo", "dg0", "dgo0")  # one writer per element: reproducible bit for bit
VOLUME_KEYS = ("gi", "di")                             # accumulated by float atomics in whatever order the waves commit
# case_two_passes in float32 adds about 70 000 terms into each of 240 volume elements: the two summed outputs get four times the error of
# the float32 CPU oracle against the float64 one on the same inputs (2.40e-6 and 2.32e-6; profiles/ext_ops_edges.md)
TWO_PASS_VOLUME_TOL = {"gi": 4 * 2.40e-6, "di": 4 * 2.32e-6}


def unnormalised(g, S):
    """float64 value of GridSamplerMineKernel.cu:210-212 before any clipping."""
    return ((g.double() + 1.) * S - 1.) / 2.


def near_cell_face(points, sizes, eps=1e-4):
    """[..., 3] (x, y, z) points, sizes (D, H, W) -> mask of the points with an unnormalised coordinate within eps of an integer: the
    gradients are piecewise per cell, and a float32 rounding there may pick the neighbouring cell."""
    D, H, W = sizes
    t = torch.stack([unnormalised(points[..., 0], W), unnormalised(points[..., 1], H), unnormalised(points[..., 2], D)], -1)
    return ((t - t.round()).abs() < eps).any(-1)


def safe_points(N, P, seed, span, sizes, max_share=0.01):
    """[N, P, 3] float32 det_tensor points in [-span, span) with those near a cell face left out; asserts the left-out share."""
    cand = fx.det_tensor((N, P + P // 50 + 16, 3), seed, span)
    rows = []
    for n in range(N):
        keep = (~near_cell_face(cand[n], sizes)).nonzero().view(-1)[:P]
        assert len(keep) == P
        used = int(keep[-1]) + 1
        assert (used - P) / used <= max_share, f"{used - P} of {used} points lie within 1e-4 of a cell face"
        rows.append(cand[n, keep])
    return torch.stack(rows)


def _cotangents(inp, grid, seed):
    N, C = inp.shape[:2]
    return dict(inp=inp, grid=grid, go=fx.det_tensor((N, C) + tuple(grid.shape[1:4]), seed + 1, 1.0), goi=fx.det_tensor(tuple(inp.shape), seed + 2, 1.0),
                gog=fx.det_tensor(tuple(grid.shape), seed + 3, 1.0))


def case_batch(general=True):
    """N = 2 with a [2,2,3,37,3] grid (split()'s general branch), or the same 222 points per batch as [2,1,1,222,3]."""
    inp = fx.det_tensor((2, 5, 4, 3, 6), 900, 1.0)
    c = _cotangents(inp, safe_points(2, 222, 901, 1.2, (4, 3, 6)).view(2, 2, 3, 37, 3), 902)
    if not general:
        c["grid"], c["gog"], c["go"] = c["grid"].reshape(2, 1, 1, 222, 3), c["gog"].reshape(2, 1, 1, 222, 3), c["go"].reshape(2, 5, 1, 1, 222)
    return c


def case_strides():
    inp = fx.det_tensor((2, 6, 5, 4, 7), 910, 1.0)
    return _cotangents(inp, safe_points(2, 131, 911, 1.15, (5, 4, 7)).view(2, 1, 1, 131, 3), 912)


def case_two_passes():
    P = LAUNCH_CAP + 4099
    inp = fx.det_tensor((1, 4, 3, 4, 5), 920, 1.0)
    return _cotangents(inp, safe_points(1, P, 921, 1.1, (3, 4, 5)).view(1, 1, 1, P, 3), 922)


def case_channel_last(C, N=1):
    inp = fx.det_tensor((N, C, 5, 4, 7), 930 + C, 1.0)
    return _cotangents(inp, safe_points(N, 300, 931 + C, 1.2, (5, 4, 7)).view(N, 1, 1, 300, 3), 932 + C)


THIN_VOLUMES = [(1, 3, 1, 1, 1), (1, 3, 1, 4, 1), (2, 4, 2, 1, 5)]


def case_thin(shape):
    """Every combination, over the three axes, of -1, 1, +-(1 - 1/S), 0, two values outside [-1, 1] and an interior one."""
    N, C, D, H, W = shape
    per_axis = [torch.tensor([-1., 1., 1. - 1. / S, -(1. - 1. / S), 0., 1.3, -1.7, 0.37]) for S in (W, H, D)]
    pts = torch.cartesian_prod(*per_axis)                                      # [512, 3] float32
    grid = torch.stack([pts.roll(n * 37, 0) for n in range(N)]).view(N, 1, 1, -1, 3).contiguous()
    return _cotangents(fx.det_tensor(shape, 940 + D * H * W, 1.0), grid, 941)


def flat_axes(grid, sizes, dtype):
    """[N,...,3] mask of the grid-gradient components the border rule (:44-60) zeroes: the coordinate, unnormalised in the type under
    test as the kernels do it, is <= 0 or >= S - 1.  Always the case on an axis of size 1."""
    D, H, W = sizes
    g = grid.to(dtype)
    t = torch.stack([((g[..., a] + 1.) * S - 1.) / 2. for a, S in enumerate((W, H, D))], -1)
    lim = torch.tensor([W - 1, H - 1, D - 1], dtype=dtype)
    return (t <= 0) | (t >= lim)


NONFINITE = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]


def case_nonfinite():
    """One axis of each of the first 15 points is NaN, +-Inf or +-1e30, the other axes and 17 more points are interior.  Returns the
    case as the kernels get it and the two finite stand-ins the expectations are built from:
      forward (GridSamplerMineKernel.cu:33-35, CUDA's ::max / ::min drop a NaN operand): NaN, -Inf, -1e30 clip to 0, +Inf, +1e30 to S-1;
      backward (:44-60, :122-129): +-Inf and +-1e30 clip the same way with a zero multiplier; NaN fails both comparisons, keeps
      multiplier 1, and is then downgraded to -100: all 8 corners are out of bounds and the point contributes nothing anywhere.
    (The host build of the reference's kernels is no witness for the NaN forward value: its stand-in for ::max returns S-1 for a NaN.)"""
    sizes = (4, 5, 6)
    inp = fx.det_tensor((1, 3) + sizes, 950, 1.0)
    base = safe_points(1, 32, 951, 0.8, sizes)
    c = _cotangents(inp, base.clone().view(1, 1, 1, 32, 3), 952)
    stand_in = base.clone().view(1, 1, 1, 32, 3)
    dead = torch.zeros(32, dtype=torch.bool)
    for j, (axis, v) in enumerate((a, v) for a in range(3) for v in NONFINITE):
        c["grid"][0, 0, 0, j, axis] = v
        stand_in[0, 0, 0, j, axis] = 5.0 if v > 0 else -5.0                    # NaN > 0 is False: first voxel plane
        dead[j] = v != v
    return c, stand_in, dead


def case_centres():
    """4096 points exactly on the voxel centres of a [1,3,2,4,4] volume, cotangents in {-2,-1,1,2}: every weight is 0 or 1 and every
    partial sum an integer of magnitude <= 256, so the scatter-add is exact in half, float and double in any order."""
    D, H, W, P, C = 2, 4, 4, 4096, 3
    u = fx.det_array((P, 3), 960, 1.0, np.float64) * 0.5 + 0.5
    vox = torch.from_numpy(np.floor(u * np.array([W, H, D])).astype(np.int64))                  # (x, y, z) per point
    grid = ((2 * vox + 1).double() / torch.tensor([W, H, D]) - 1.).float().view(1, 1, 1, P, 3)
    pick = torch.from_numpy(np.floor((fx.det_array((C, P), 961, 1.0, np.float64) * 0.5 + 0.5) * 4).astype(np.int64))
    go = torch.tensor([-2., -1., 1., 2.])[pick].view(1, C, 1, 1, P)
    goi = torch.from_numpy(np.floor(fx.det_array((1, C, D, H, W), 962, 3.999, np.float64))).float()
    lin = (vox[:, 2] * H + vox[:, 1]) * W + vox[:, 0]
    gi = torch.zeros(C, D * H * W, dtype=torch.int64).index_add_(1, lin, go.view(C, P).long()).view(1, C, D, H, W)
    dgo = goi.view(C, -1).long()[:, lin].view(1, C, 1, 1, P)
    return dict(inp=fx.det_tensor((1, C, D, H, W), 963, 1.0), grid=grid, go=go, goi=goi, gog=torch.zeros(1, 1, 1, P, 3)), gi, dgo


def oracle_all(inp, grid, go, goi, gog, dtype=torch.float64):
    """oracle/torch_oracle.py::grid_sample_3d with autograd to second order, on the CPU.  out; gi, gg = backward; di, dg, dgo = double
    backward of <gi, goi> + <gg, gog>; dg0, dgo0 = the same without grad_output_input."""
    i, g, o = [t.detach().to(dtype).clone().requires_grad_(True) for t in (inp, grid, go)]
    out = orc.grid_sample_3d(i, g)
    gi, gg = torch.autograd.grad(out, (i, g), o, create_graph=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    di, dg0, dgo0 = torch.autograd.grad((gg * gog.to(dtype)).sum(), (i, g, o), retain_graph=True, allow_unused=True)
    dga, dgoa = torch.autograd.grad((gi * goi.to(dtype)).sum(), (g, o), allow_unused=True)
    di, dg0, dgo0 = z(di, i), z(dg0, g), z(dgo0, o)
    r = dict(out=out, gi=gi, gg=gg, di=di, dg=dg0 + z(dga, g), dgo=dgo0 + z(dgoa, o), dg0=dg0, dgo0=dgo0)
    return {k: v.detach() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def reference(builder, *args):
    """float64 oracle of a case built by `builder(*args)` on its float32 values upcast; computed once per session, never modified."""
    return oracle_all(**globals()[builder](*args))


@functools.lru_cache(maxsize=None)
def reference_nonfinite():
    c, stand_in, dead = case_nonfinite()
    alive = (~dead).to(c["go"].dtype).view(1, 1, 1, 1, -1)
    r = oracle_all(c["inp"], stand_in, c["go"] * alive, c["goi"], c["gog"])
    r["out"] = oracle_all(c["inp"], stand_in, c["go"], c["goi"], c["gog"])["out"]
    for k in ("dgo", "dgo0"):
        r[k] = r[k] * alive.double()
    return r


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)
