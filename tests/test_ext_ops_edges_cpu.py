"""The helpers behind tests/test_ext_ops_edges_gpu.py, checked without a GPU: the vectorised upsampler reference against the loop it
restates, and the hand-built sampler expectations (exact scatter, border mask, non-finite stand-ins) against the float64 oracle."""
import numpy as np
import pytest
import torch
from oracle import fixtures as fx
import _gs_edges as ge
from _interp2x_ref import interp2x_loop, interp2x_vectorised


@pytest.mark.parametrize("shape", [(5, 4, 6), (1, 3, 1)])
def test_vectorised_upsampler_reference_equals_the_loop(shape):
    a = fx.det_array(shape, 77, 1.0)
    lo, lb = interp2x_loop(a, 0.1)
    vo, vb = interp2x_vectorised(a, 0.1)
    assert vo.dtype == np.float32 and np.array_equal(vo, lo) and np.array_equal(vb, lb)
    assert lb.any() and not lb.all()
    stacked = interp2x_vectorised(np.stack([a, -a])[None], 0.1)                 # leading dimensions are independent volumes
    assert np.array_equal(stacked[0][0, 0], lo) and np.array_equal(stacked[0][0, 1], interp2x_loop(-a, 0.1)[0])
    assert np.array_equal(stacked[1][0, 1], interp2x_loop(-a, 0.1)[1])


def test_vectorised_upsampler_reference_in_float64_is_the_interpolation():
    a = fx.det_array((3, 1, 4), 79, 1.0, np.float64)
    vo, _ = interp2x_vectorised(a, 0.0)
    ti = torch.nn.functional.interpolate(torch.from_numpy(a)[None, None], size=vo.shape, mode="trilinear", align_corners=True)[0, 0]
    assert vo.dtype == np.float64 and np.abs(vo - ti.numpy()).max() < 1e-15


def test_safe_points_leave_out_cell_faces_and_few_points():
    sizes = (4, 3, 6)
    p = ge.safe_points(2, 222, 901, 1.2, sizes)
    assert p.shape == (2, 222, 3) and p.dtype == torch.float32 and not ge.near_cell_face(p, sizes).any()
    on_face = torch.tensor([[1. / 6 - 1 + 1e-6, 0.3, 0.2], [0.31, 0.3, 0.2]])     # x unnormalises to 3e-6 / to 3.43
    assert ge.near_cell_face(on_face, sizes).tolist() == [True, False]
    P = ge.LAUNCH_CAP + 4099                                                       # the largest case: about 0.06 % of the candidates are left out
    big = ge.case_two_passes()["grid"]
    assert big.shape == (1, 1, 1, P, 3) and not ge.near_cell_face(big, (3, 4, 5)).any()


def test_exact_scatter_expectation_is_the_oracles_gradient():
    c, gi, dgo = ge.case_centres()
    assert set(c["go"].unique().tolist()) == {-2., -1., 1., 2.} and torch.equal(c["grid"].half().float(), c["grid"])
    assert int(gi.abs().max()) <= 256 and (gi != 0).float().mean() > 0.9
    r = ge.oracle_all(**c)
    assert torch.equal(r["gi"], gi.double()) and torch.equal(r["dgo"], dgo.double()) and not r["di"].any()


@pytest.mark.parametrize("shape", ge.THIN_VOLUMES)
def test_border_mask_matches_the_oracles_zero_gradients(shape):
    c = ge.case_thin(shape)
    flat = ge.flat_axes(c["grid"], shape[2:], torch.float64)
    for a, S in enumerate((shape[4], shape[3], shape[2])):
        assert flat[..., a].all() if S == 1 else (flat[..., a].any() and not flat[..., a].all())
    r = ge.oracle_all(**c)
    assert not r["gg"][flat].any() and r["out"].abs().max() > 0


def test_nonfinite_expectation_is_finite_and_dead_points_are_silent():
    c, stand_in, dead = ge.case_nonfinite()
    assert int(dead.sum()) == 3 and int((~torch.isfinite(c["grid"])).sum()) == 9 and torch.isfinite(stand_in).all()
    r = ge.reference_nonfinite()
    assert all(torch.isfinite(v).all() for v in r.values())
    for k in ("gg", "dg", "dg0"):
        assert not r[k][0, 0, 0, dead].any()
    for k in ("dgo", "dgo0"):
        assert not r[k][0, :, 0, 0, dead].any()
    assert r["out"][0, :, 0, 0, dead].abs().min() > 0                              # the forward value of a NaN point is a real sample
    axis_of = [a for a in range(3) for _ in ge.NONFINITE]
    for j, a in enumerate(axis_of):                                                # the non-finite axis has no gradient, the others do
        assert r["gg"][0, 0, 0, j, a] == 0 and (dead[j] or r["gg"][0, 0, 0, j].abs().sum() > 0)
