"""The skinning-field builder on the GPU (csrc/lbsw.hip, model/Deformer.py) against the reference's own compute_lbswField / smooth_weights
frozen in tests/golden/lbsw.npz, and against the float64 twin of tests/_lbsw_ref.py.

Bound everywhere a fixture exists: our error against the twin <= 4 x the reference's own recorded float32 error against that twin
(floor 1e-6); voxels whose k-th and (k+1)-th distances are closer than 1e-6 (relative) may be left out, at most 0.1 % of them.
Every test prints the figures before it asserts."""
import os

import numpy as np
import pytest
import torch

import _lbsw_ref as twin
from selfreconcode_amd.synthetic import LBS_BMAX, LBS_BMIN, SMPL_PARENTS, synthetic_body, synthetic_joints

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbsw.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def body():
    v, w = synthetic_body(seed=twin.GOLDEN_BODY_SEED)
    return v.to(DEV), w.to(DEV)


@pytest.fixture(scope="module")
def small_twin(body):
    v, w = body
    pre, gap = twin.field(LBS_BMIN, LBS_BMAX, twin.SMALL_GRID, v.cpu().numpy(), w.cpu().numpy(), twin.K_REF)
    return pre, gap


def _field(body, res, k, times, **kw):
    from selfreconcode_amd.model.Deformer import compute_lbswField
    v, w = body
    out = compute_lbswField(LBS_BMIN, LBS_BMAX, res, v, w, mean_neighbor=k, smooth_times=times, **kw)
    W, H, D = res
    assert tuple(out.shape) == (1, w.shape[1], D, H, W) and out.dtype == torch.float32
    return out


def _check(name, ours, tw, gap, ref_err, ref=None):
    err, dropped = twin.masked_error(ours, tw, gap)
    vs_ref = "" if ref is None else f", vs the reference's float32 field {np.abs(np.asarray(ours, np.float64) - ref).max():.3e}"
    print(f"{name}: error vs float64 twin {err:.3e} (reference's own {float(ref_err):.3e}, bound {twin.bound(ref_err):.3e}), "
          f"{dropped} of {np.asarray(gap).size} voxels excluded{vs_ref}")
    assert dropped <= twin.EXCLUDE_CAP * np.asarray(gap).size
    assert err <= twin.bound(ref_err)


def test_stage1_small_grid_against_reference(gold, body, small_twin):
    ours = _field(body, twin.SMALL_GRID, twin.K_REF, 0)[0].cpu().numpy()
    _check("stage 1 (17,29,9) k=30", ours, small_twin[0], small_twin[1], gold["small_err_pre"], gold["small_pre"])


def test_stage1_k5_against_reference(gold, body):
    v, w = body
    tw, gap = twin.field(LBS_BMIN, LBS_BMAX, twin.SMALL_GRID, v.cpu().numpy(), w.cpu().numpy(), 5)
    ours = _field(body, twin.SMALL_GRID, 5, 0)[0].cpu().numpy()
    _check("stage 1 (17,29,9) k=5", ours, tw, gap, gold["small_k5_err_pre"], gold["small_k5_pre"])


def test_stage1_mid_grid_subsample_against_reference(gold, body):
    v, w = body
    idx = gold["mid_idx"].astype(np.int64)
    assert np.array_equal(idx, twin.mid_subsample())
    tw, gap = twin.knn_blend(twin.centres(LBS_BMIN, LBS_BMAX, twin.MID_GRID, flat_index=idx), v.cpu().numpy(), w.cpu().numpy(), twin.K_REF)
    ours = _field(body, twin.MID_GRID, twin.K_REF, 0)[0].reshape(24, -1)[:, idx].cpu().numpy()
    _check("stage 1 (33,57,17) subsample", ours, tw.T, gap, gold["mid_err_pre"], gold["mid_pre"])


@pytest.mark.parametrize("times", [0, 1, 30])
def test_stage2_alone_against_reference(gold, small_twin, times):
    from selfreconcode_amd.model.Deformer import smooth_weights
    pre = torch.from_numpy(gold["small_pre"]).to(DEV)[None]
    keep = pre.clone()
    out = smooth_weights(pre, times)
    assert torch.equal(pre, keep)                                          # the argument is left as it was
    if times == 0:
        assert torch.equal(out, pre)
        return
    tw = twin.smooth(small_twin[0], times)
    # the recorded error after 30 steps bounds 30 steps; one step is held to the error recorded BEFORE smoothing, which it starts from
    ref_err = gold["small_err_post"] if times == 30 else gold["small_err_pre"]
    ref = gold["small_post"] if times == 30 else None
    _check(f"stage 2 alone, {times} steps", out[0].cpu().numpy(), tw, np.full(tw[0].size, np.inf), ref_err, ref)


def test_stage2_hand_computed_3x3x3():
    from selfreconcode_amd.model.Deformer import smooth_weights
    a = np.arange(27, dtype=np.float64).reshape(3, 3, 3) / 26.0 + 0.5
    f = np.stack([a, 2.0 - a])                                             # channel sums 2 everywhere
    out = smooth_weights(torch.from_numpy(f).float().to(DEV)[None], 1)[0].double().cpu().numpy()
    exp = f.copy()
    for c in range(2):
        m = (f[c, 2, 1, 1] + f[c, 0, 1, 1] + f[c, 1, 2, 1] + f[c, 1, 0, 1] + f[c, 1, 1, 2] + f[c, 1, 1, 0]) / 6.0
        exp[c, 1, 1, 1] = (f[c, 1, 1, 1] - m) * 0.7 + m
    exp = exp / exp.sum(0, keepdims=True)
    err = np.abs(out - exp).max()
    print(f"3x3x3 hand case: {err:.3e}")
    assert err <= 8 * 2.0 ** -24                                            # eight float32 roundings of values <= 1 (6 adds, scale, divide)
    # the centre of a linear ramp is its neighbours' mean: only the normalisation acts
    assert abs(out[0, 1, 1, 1] - f[0, 1, 1, 1] / 2.0) <= 8 * 2.0 ** -24


def test_stage2_grid_without_interior():
    from selfreconcode_amd.model.Deformer import smooth_weights
    from selfreconcode_amd.synthetic import det_tensor
    f = (det_tensor((1, 5, 2, 7, 9), 31, 0.5) + 1.0).to(DEV)               # D = 2: no interior voxel, every step only renormalises
    out = smooth_weights(f, 3)
    exp = f.double() / f.double().sum(1, keepdim=True)
    err = float((out.double() - exp).abs().max())
    print(f"D = 2: {err:.3e}")
    assert err <= 3 * 4 * 2.0 ** -24                                        # three renormalisations: a 5-term sum and a divide each


def test_end_to_end_against_reference(gold, body, small_twin):
    ours = _field(body, twin.SMALL_GRID, twin.K_REF, 30)[0].cpu().numpy()
    tw = twin.smooth(small_twin[0], 30)
    _check("end to end (17,29,9)", ours, tw, small_twin[1] * 0 + np.inf, gold["small_err_post"], gold["small_post"])
    idx = gold["mid_idx"].astype(np.int64)
    mid = _field(body, twin.MID_GRID, twin.K_REF, 30)[0].reshape(24, -1)[:, idx].cpu().numpy()
    err = np.abs(mid.astype(np.float64) - gold["mid_post"]).max()
    # both are float32 results within their own error of the same twin: ours within 4 x, the reference within 1 x
    print(f"end to end (33,57,17) subsample vs the reference's float32 field: {err:.3e} (bound {5 * max(float(gold['mid_err_post']), 2.5e-7):.3e})")
    assert err <= 5 * max(float(gold["mid_err_post"]), 2.5e-7)


def test_axis_order_body_shift_moves_the_field_along_w(body):
    from selfreconcode_amd.model.Deformer import compute_lbswField
    v, w = body
    W, H, D = twin.SMALL_GRID
    step = (LBS_BMAX[0] - LBS_BMIN[0]) / W
    base = compute_lbswField(LBS_BMIN, LBS_BMAX, twin.SMALL_GRID, v, w, mean_neighbor=twin.K_REF, smooth_times=0)
    shift = torch.tensor([3 * step, 0., 0.], device=DEV)
    moved = compute_lbswField(LBS_BMIN, LBS_BMAX, twin.SMALL_GRID, v + shift, w, mean_neighbor=twin.K_REF, smooth_times=0)
    assert tuple(base.shape) == (1, 24, D, H, W)
    err = float((moved[..., 3:] - base[..., :-3]).abs().max())
    other = min(float((moved[..., 3:, :] - base[..., :-3, :]).abs().max()), float((moved[:, :, 3:] - base[:, :, :-3]).abs().max()))
    print(f"axis order: shifted along W {err:.3e}, along H / D {other:.3e}")
    # the same geometry up to the float32 rounding of the shifted coordinates (relative 1e-7 of distances >= 1e-2: as in stage 1)
    assert err <= 1e-4 and other > 1e-2


# ------------------------------------------------------------------------------------------------ full size
FULL = (129, 225, 65)


@pytest.fixture(scope="module")
def full(body):
    v, w = body
    from selfreconcode_amd.model.Deformer import compute_lbswField
    pre = compute_lbswField(LBS_BMIN, LBS_BMAX, FULL, v, w, mean_neighbor=twin.K_REF, smooth_times=0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()                                   # (`pre` is the test's, not the build's)
    post = compute_lbswField(LBS_BMIN, LBS_BMAX, FULL, v, w, mean_neighbor=twin.K_REF, smooth_times=30)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return pre, post, peak


def test_full_size_stage1_against_twin(gold, body, full):
    v, w = body
    n = FULL[0] * FULL[1] * FULL[2]
    idx = np.arange(113, n, 233)                                           # ~8.1k voxels
    tw, gap = twin.knn_blend(twin.centres(LBS_BMIN, LBS_BMAX, FULL, flat_index=idx), v.cpu().numpy(), w.cpu().numpy(), twin.K_REF)
    ours = full[0][0].reshape(24, -1)[:, torch.from_numpy(idx).to(DEV)].cpu().numpy()
    # no reference run exists at this size (50 minutes of CPU): the same body in the same box, so the error recorded on (33,57,17)
    _check("full size stage 1", ours, tw.T, gap, gold["mid_err_pre"])


def test_full_size_smoothing_properties_and_memory(body, full):
    v, w = body
    pre, post, peak = full
    f = pre.clone()
    for _ in range(30):                                                    # the reference's slicing formulation, float32, on the device
        mean = (f[:, :, 2:, 1:-1, 1:-1] + f[:, :, :-2, 1:-1, 1:-1] + f[:, :, 1:-1, 2:, 1:-1] + f[:, :, 1:-1, :-2, 1:-1] + f[:, :, 1:-1, 1:-1, 2:]
                + f[:, :, 1:-1, 1:-1, :-2]) / 6.0
        f[:, :, 1:-1, 1:-1, 1:-1] = (f[:, :, 1:-1, 1:-1, 1:-1] - mean) * 0.7 + mean
        f = f / f.sum(1, keepdim=True)
    err = float((post - f).abs().max())
    sums = float((post.sum(1) - 1).abs().max())
    volume = post.numel() * 4
    print(f"full size: vs sliced torch {err:.3e}, channel sums off by {sums:.3e}, min {float(post.min()):.3e}, peak {peak / volume:.2f} x the volume")
    # two float32 evaluations of the same 30 steps, different summation order: at most 8 roundings of values <= 1 per step
    assert err <= 30 * 8 * 2.0 ** -24
    assert not torch.isnan(post).any() and float(post.min()) >= 0.
    assert sums <= 1e-6
    assert peak < 3 * volume
    from selfreconcode_amd.model.Deformer import compute_lbswField
    again = compute_lbswField(LBS_BMIN, LBS_BMAX, FULL, v, w, mean_neighbor=twin.K_REF, smooth_times=30)
    assert torch.equal(again, post)


# ------------------------------------------------------------------------------------------------ the skinner built from it
def test_initial_lbs_skinner(body):
    from selfreconcode_amd.model.Deformer import LBS_BOX_MARGIN, LBSkinner, initial_lbs_skinner
    from selfreconcode_amd.utils.utils import smpl_tmp_Apose
    v, w = body
    res = (65, 113, 33)
    pose0 = torch.from_numpy(smpl_tmp_Apose(0)).float().view(24, 3)
    Js = synthetic_joints()
    sk = initial_lbs_skinner(v, w, Js, np.array(SMPL_PARENTS), pose0, res)
    assert isinstance(sk, LBSkinner) and tuple(sk.ws.shape) == (1, 24, res[2], res[1], res[0])
    margin = torch.tensor(LBS_BOX_MARGIN, device=DEV)
    assert torch.equal(sk.b_min.view(3), v.min(0)[0] - margin) and torch.equal(sk.b_max.view(3), v.max(0)[0] + margin)
    zero = torch.zeros(1, 3, device=DEV)
    with torch.no_grad():
        rest = sk(v[None], [pose0.view(1, 24, 3).to(DEV), zero])[0]
    e_rest = float((rest - v).abs().max())
    # A = G inv(G) in float32 over chains of <= 9 joints, times weights that sum to 1 within 1e-6, on coordinates <= 1.3
    print(f"initial_lbs_skinner: rest pose moves the body by {e_rest:.3e}")
    assert e_rest <= 1e-5
    pose = pose0.clone()
    pose[16] += torch.tensor([0., 0., 0.5]); pose[4] += torch.tensor([0.4, 0., 0.]); pose[12] += torch.tensor([0., 0.3, 0.])
    pose = pose.view(1, 24, 3).to(DEV)
    with torch.no_grad():
        A = sk.posed_transforms(pose)[0]                                   # [24,4,4]
        T = torch.einsum("vj,jab->vab", w, A)
        direct = (T[:, :3, :3] @ v[:, :, None])[:, :, 0] + T[:, :3, 3]
        posed = sk(v[None], [pose, zero])[0]
    diag = float((((sk.b_max - sk.b_min).view(3) / torch.tensor(res, device=DEV).float()) ** 2).sum().sqrt())
    off = float((posed - direct).norm(dim=1).max())
    print(f"initial_lbs_skinner: posed body within {off / diag:.2f} voxel diagonals of direct LBS (diagonal {diag:.4f})")
    assert off <= 1.5 * diag


def test_ties_lower_index_wins():
    from selfreconcode_amd.model.Deformer import compute_lbswField
    verts = torch.tensor([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [5., 5., 5.]], device=DEV)
    ws = torch.tensor([[1., 0.], [0., 1.], [.5, .5]], device=DEV)
    a = compute_lbswField([-1, -1, -1], [1, 1, 1], (5, 7, 3), verts, ws, mean_neighbor=1, smooth_times=0)
    b = compute_lbswField([-1, -1, -1], [1, 1, 1], (5, 7, 3), verts, ws, mean_neighbor=1, smooth_times=0)
    assert torch.equal(a, b)
    assert torch.equal(a[0, 0], torch.ones_like(a[0, 0])) and torch.equal(a[0, 1], torch.zeros_like(a[0, 1]))
    swapped = compute_lbswField([-1, -1, -1], [1, 1, 1], (5, 7, 3), verts, ws[[1, 0, 2]], mean_neighbor=1, smooth_times=0)
    assert torch.equal(swapped[0, 1], torch.ones_like(a[0, 0]))


def test_neighbour_count_limits(body):
    from selfreconcode_amd.model.Deformer import compute_lbswField
    v, w = body
    with pytest.raises((ValueError, RuntimeError)):
        compute_lbswField(LBS_BMIN, LBS_BMAX, (5, 7, 3), v, w, mean_neighbor=33, smooth_times=0)
    with pytest.raises((ValueError, RuntimeError)):
        compute_lbswField(LBS_BMIN, LBS_BMAX, (5, 7, 3), v[:4], w[:4], mean_neighbor=5, smooth_times=0)
    from selfreconcode_amd import _lib
    out = torch.empty((24, 3, 7, 5), device=DEV)
    import ctypes
    lo, hi = (ctypes.c_float * 3)(*LBS_BMIN), (ctypes.c_float * 3)(*LBS_BMAX)
    for nv, k in ((v.shape[0], 33), (4, 5)):
        assert _lib.raw("sr_lbsw_knn_blend")(v.data_ptr(), w.data_ptr(), nv, 24, k, 5, 7, 3, lo, hi, 0, out.data_ptr(), 0) == -1     # SR_EINVAL
    assert compute_lbswField(LBS_BMIN, LBS_BMAX, (5, 7, 3), v, w, mean_neighbor=32, smooth_times=0).shape == (1, 24, 3, 7, 5)
