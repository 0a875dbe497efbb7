"""The float64 LBS / kinematic-chain references and the seeded cases of tests/_lbs_ref.py, checked on the host: the case generator's
guarantees, the references against finite differences of their own values and against the closed forms of csrc/lbs.hip's header.
tests/test_lbs_paths_gpu.py holds the kernels to what is checked here."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import torch_oracle as orc
import _lbs_ref as R


@pytest.fixture(scope="module")
def K():
    return R.constants()


def _extent():
    return np.asarray(fx.LBS_BMAX, np.float64) - np.asarray(fx.LBS_BMIN, np.float64)


def test_interior_points_stay_clear_of_the_cell_faces_in_float32_and_float64():
    p = R.interior_points(2000, 5)
    assert p.dtype == np.float32
    t32 = R.unnormalised_f32(p)
    t64 = ((2. * (p.astype(np.float64) - np.asarray(fx.LBS_BMIN)) / _extent() - 1. + 1.) * R._sizes() - 1.) / 2.
    f32, f64 = t32 - np.floor(t32), t64 - np.floor(t64)
    assert (f32 >= R.FRAC_LO).all() and (f32 <= R.FRAC_HI).all() and (f64 >= R.FRAC_LO).all() and (f64 <= R.FRAC_HI).all()
    assert (np.floor(t32) == np.floor(t64)).all()                                # kernel and reference agree on the cell
    assert (t32 > 0).all() and (t32 < R._sizes() - 1).all()                      # never on the border rule
    cells = {tuple(c) for c in np.floor(t32).astype(int)}
    assert len(cells) == int(np.prod(R._sizes() - 1))                            # 2000 points visit every one of the 960 cells


def test_outside_points_are_beyond_the_box_on_one_two_and_three_axes():
    p, out = R.outside_points(70, 9)
    lo, hi = np.asarray(fx.LBS_BMIN, np.float64), np.asarray(fx.LBS_BMAX, np.float64)
    dist = np.maximum(lo - p, p - hi) / _extent()                                # > 0: beyond a face, in shares of the extent
    assert (dist[out] >= R.OUT_MARGIN).all() and (dist[~out] < 0).all()
    assert set(out.sum(1).tolist()) == {1, 2, 3}
    assert (p[out] < lo[None].repeat(70, 0)[out]).any() and (p[out] > hi[None].repeat(70, 0)[out]).any()      # both sides
    t = R.unnormalised_f32(p)
    assert ((t[out] <= 0) | (t[out] >= (R._sizes()[None].repeat(70, 0))[out] - 1)).all()                        # the border rule applies there


def test_lattice_points_sit_on_voxel_centres_and_box_faces():
    p = R.lattice_points(60, 4)
    lo, hi = np.asarray(fx.LBS_BMIN, np.float32), np.asarray(fx.LBS_BMAX, np.float32)
    on_face = (p == lo) | (p == hi)
    assert not on_face[0::2].any() and on_face[1::2].any(1).all() and set(on_face[1::2].sum(1).tolist()) == {1, 2, 3}
    t = ((2. * (p.astype(np.float64) - lo) / _extent() - 1. + 1.) * R._sizes() - 1.) / 2.
    assert (np.abs(t - np.round(t))[~on_face] < 1e-5).all()                      # centres up to the float32 rounding of p


@pytest.mark.parametrize("N,P,order", R.case_table())
def test_case_frames_cover_what_the_order_promises(N, P, order):
    c = R.make_case(P, N, order, lattice=True)
    bi = c.bi.numpy()
    assert c.p.shape == (P, 3) and c.p.dtype == torch.float32 and bi.shape == (P,) and bi.min() >= 0 and bi.max() < N
    used = set(bi.tolist())
    if order == "sorted":
        assert (np.diff(bi) >= 0).all() and (used == set(range(N)) if P >= N else len(used) == P)
    elif order == "interleaved":
        assert used == set(range(min(N, P))) and (N == 1 or P == 1 or (np.diff(bi[:min(N, P)]) == 1).all())
    elif order == "last":
        assert used == {N - 1}
    else:
        assert N // 2 not in used and N // 2 in c.empty and (used == set(range(N)) - {N // 2} if P >= N - 1 else True)
    assert c.empty == sorted(set(range(N)) - used)
    assert int((c.cls == 2).sum()) == P // 6 and bool((c.deriv == (c.cls != 2)).all())
    assert int((R.make_case(P, N, order).cls == 2).sum()) == 0                   # backward cases: nothing is left out of a comparison


def test_case_table_reaches_every_value_of_every_axis():
    tab = R.case_table()
    assert 24 <= len(tab) <= 30
    assert {n for n, _, _ in tab} == set(R.NFRAMES) and {p for _, p, _ in tab} == set(R.POINTS) and {o for _, _, o in tab} == set(R.ORDERS)
    assert {(p, o) for _, p, o in tab} == {(p, o) for p in R.POINTS for o in R.ORDERS}
    assert {(n, o) for n, _, o in tab} == {(n, o) for n in R.NFRAMES for o in R.ORDERS} - {(1, "empty")}


def test_given_transforms_is_the_oracle_forward(K):
    c = R.make_case(65, 3, "interleaved", lattice=True)
    y0 = orc.lbs_forward(c.p.double(), c.poses.double(), c.trans.double(), K.ws, K.b_min, K.b_max, K.Js, K.init_pose, batch_inds=c.bi)
    y1 = R.lbs_from_transforms(c.p.double(), R.transforms(c.poses, K), c.trans.double(), K, c.bi)
    assert torch.equal(y0, y1)
    assert orc.lbs_transforms.__module__ == orc.__name__                        # and the oracle is left as it was


def test_reference_jacobian_matches_central_differences_of_its_value(K):
    c = R.make_case(257, 9, "interleaved")
    A = R.transforms(c.poses, K)
    ref = R.lbs_reference(c.p, A, c.trans, c.bi, K)
    h = 1e-6
    fd = torch.zeros(c.P, 3, 3, dtype=torch.float64)
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64); e[k] = h
        yp = R.lbs_from_transforms(c.p.double() + e, A, c.trans.double(), K, c.bi)
        ym = R.lbs_from_transforms(c.p.double() - e, A, c.trans.double(), K, c.bi)
        fd[:, :, k] = (yp - ym) / (2 * h)
    inside = c.cls == 0
    assert int(inside.sum()) > 150 and int((c.cls == 1).sum()) > 50
    torch.testing.assert_close(ref.J, fd, rtol=1e-7, atol=1e-8)                  # interior and outside alike (no point is excluded)


def test_reference_abar_and_transbar_equal_the_closed_forms(K):
    """csrc/lbs.hip: Abar[frame][j] = sum w_j ybar (x) [p;1], transbar[frame] = sum ybar (first order), over the frame's points."""
    c = R.make_case(255, 8, "empty")
    A = R.transforms(c.poses, K)
    ref = R.lbs_reference(c.p, A, c.trans, c.bi, K, c.wy, None)
    nps = 2. * (c.p.double() - K.b_min) / (K.b_max - K.b_min) - 1.
    w = orc.grid_sample_3d(K.ws, nps.view(1, 1, 1, -1, 3)).view(24, -1).t()                          # [P,24]
    ph = torch.cat([c.p.double(), torch.ones(c.P, 1, dtype=torch.float64)], 1)
    per_point = w[:, :, None, None] * c.wy.double()[:, None, :, None] * ph[:, None, None, :]        # [P,24,3,4]
    Abar = torch.zeros(c.N, 24, 3, 4, dtype=torch.float64).index_add_(0, c.bi, per_point)
    tbar = torch.zeros(c.N, 3, dtype=torch.float64).index_add_(0, c.bi, c.wy.double())
    torch.testing.assert_close(ref.Abar, Abar.view(c.N, 24, 12), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(ref.transbar, tbar, rtol=1e-12, atol=1e-13)
    assert c.empty == [4] and float(ref.Abar[4].abs().max()) == 0.0 and float(ref.transbar[4].abs().max()) == 0.0
    # and with a cotangent on J the translations still see ybar alone, an empty frame still nothing
    ref2 = R.lbs_reference(c.p, A, c.trans, c.bi, K, c.wy, c.wJ)
    torch.testing.assert_close(ref2.transbar, tbar, rtol=1e-12, atol=1e-13)
    assert float(ref2.Abar[4].abs().max()) == 0.0 and float((ref2.Abar - ref.Abar).abs().max()) > 1e-3


def test_reference_pbar_matches_central_differences_of_the_scalar(K):
    c = R.make_case(65, 3, "interleaved")
    A = R.transforms(c.poses, K)
    ref = R.lbs_reference(c.p, A, c.trans, c.bi, K, c.wy, c.wJ)

    def scalar_per_point(p):
        r = R.lbs_reference(p, A, c.trans, c.bi, K)
        return (r.y * c.wy.double()).sum(1) + (r.J * c.wJ.double()).sum((1, 2))
    h = 1e-6
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64); e[k] = h
        fd = (scalar_per_point(c.p.double() + e) - scalar_per_point(c.p.double() - e)) / (2 * h)
        torch.testing.assert_close(ref.pbar[:, k], fd, rtol=1e-6, atol=1e-6)


def test_chain_reference_posebar_matches_central_differences(K):
    poses = R.chain_poses(3)
    assert float(poses[0, 3].abs().max()) == 0.0 and float(poses[1].abs().max()) == 0.0                 # an exact-zero joint, a zero pose
    assert 5e-5 < float(poses[0, 7].norm()) < 2e-4 and abs(float(poses[0, 11].norm()) - 3.1) < 1e-6
    wA, wG = fx.det_tensor((3, 24, 4, 4), 62, 1.0), fx.det_tensor((3, 24, 4, 4), 63, 1.0)
    ref = R.chain_reference(poses, K, wA, wG)
    torch.testing.assert_close(ref.G[:, :, :3, 3], ref.newJ, rtol=0, atol=1e-14)
    torch.testing.assert_close(ref.G[:, :, :3, :3] @ ref.G[:, :, :3, :3].transpose(-1, -2), torch.eye(3, dtype=torch.float64).expand(3, 24, 3, 3),
                               rtol=0, atol=1e-12)

    def scalar(po):
        r = R.chain_reference(po, K)
        return (r.A * wA.double()).sum() + (r.G * wG.double()).sum()
    # central differences at the planted joints of pose 0 and at every joint of the zero pose; the step is far below the 1e-4
    # rotations and far above the 1e-8 inside the norm
    h = 1e-6
    for b, joints in ((0, (0, 3, 7, 11, 2, 9)), (1, range(24)), (2, (0, 5))):
        for j in joints:
            for k in range(3):
                d = torch.zeros(3, 24, 3, dtype=torch.float64); d[b, j, k] = h
                fd = (scalar(poses.double() + d) - scalar(poses.double() - d)) / (2 * h)
                assert abs(float(ref.posebar[b, j, k]) - float(fd)) <= 1e-5 * max(1.0, abs(float(fd))), (b, j, k, float(ref.posebar[b, j, k]), float(fd))
