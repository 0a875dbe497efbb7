"""The pose-conditioning kernels (csrc/posecond.hip through posecond_ops.py) against the float64 restatements of tests/_posecond_ref.py:
the pose feature, the fused neighbour search against its witness (bit for bit) and against float64, the code blend and the sigma
calibration.  Every bound is stated before the run; the measured maxima are printed before they are asserted."""
import math

import numpy as np
import pytest
import torch

import _posecond_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2. ** -24
FEATURE_TOL = 64 * U              # about twenty float32 operations on magnitudes <= 1 with 2-ulp sinf / cosf
D2_REL = 210 * U                  # 207 fused terms plus the roundings of a difference, all terms non-negative
BLEND_TOL = 32 * U                # times max|codes|: w_k off by (|a_k| + 4) u relative, w_k |a_k| <= 1 / e, K + 1 roundings of the sum
WEIGHT_SUM_TOL = 8 * U


def _poses(n, seed, scale=0.3):
    return (scale * np.random.default_rng(seed).standard_normal((n, 24, 3))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ features
@pytest.mark.parametrize("N", [1, 65, 300])
def test_pose_features(N):
    from selfreconcode_amd import posecond_ops as po
    rng = np.random.default_rng(N)
    theta = _poses(N, 100 + N, 0.8)
    theta[0] = 0.                                                                    # the zero pose
    if N > 1:
        axis = rng.standard_normal((24, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        theta[1] = (axis * (math.pi - 1e-3 * rng.uniform(-1, 1, (24, 1)))).astype(np.float32)      # angles within 1e-3 of pi
        theta[2] = (axis * 1e-7).astype(np.float32)                                  # angles of 1e-7
        theta[3, 5] = 0.                                                             # one resting joint among moving ones
    weights = rng.uniform(0.2, 2., 23)
    weights[4] = 0.
    for w in (None, weights):
        got = po.pose_features(torch.from_numpy(theta).to(DEV), w)
        assert got.shape[0] == 207 and got.shape[1] >= N and got.shape[1] % po.LD_ALIGN == 0
        assert not bool(got[:, N:].any())
        got = got[:, :N].T.double().cpu().numpy()
        want = ref.features(theta, w)
        err = np.abs(got - want).max()
        print(f"pose_features N={N} weights={'yes' if w is not None else 'no'}: max error {err:.3e} (bound {FEATURE_TOL:.3e})")
        assert err <= FEATURE_TOL
        assert not got[0].any()                                                      # zero pose -> zero feature, exactly
        if w is not None:
            assert not got[:, 4 * 9:5 * 9].any()
    again = po.pose_features(torch.from_numpy(theta).to(DEV), weights)
    assert torch.equal(again, po.pose_features(torch.from_numpy(theta).to(DEV), weights))


def test_pose_features_refuses():
    from selfreconcode_amd import posecond_ops as po
    with pytest.raises(ValueError, match="24,3"):
        po.pose_features(torch.zeros((3, 23, 3), device=DEV))
    with pytest.raises(ValueError, match="joint_weights"):
        po.pose_features(torch.zeros((3, 24, 3), device=DEV), [-1.] * 23)
    with pytest.raises(RuntimeError, match="non-GPU"):
        po.pose_features(torch.zeros((3, 24, 3)))


# ------------------------------------------------------------------------------------------------ search
def _search_case(N, Q):
    """Training poses with a duplicated row (3 = 1) and a NaN row (2) when N >= 5; queries: training pose 0, training pose 1, random."""
    train = _poses(N, 7 * N + 1)
    if N >= 5:
        train[3] = train[1]
        train[2] = np.nan
    queries = _poses(Q, 13 * N + Q)
    queries[0] = train[0]
    if Q > 1 and N > 1:
        queries[1] = train[1]
    frames = (np.arange(Q) * 7) % N
    if N >= 5:
        frames[frames == 2] = 4                                                      # (no query is the NaN row)
    return train, queries, frames.astype(np.int64)


@pytest.mark.parametrize("Q", [1, 3, 70])
@pytest.mark.parametrize("N", [1, 5, 64, 257, 1000])
def test_pose_neighbors(N, Q):
    from selfreconcode_amd import posecond_ops as po
    train, queries, frames = _search_case(N, Q)
    index = po.PoseIndex.build(torch.from_numpy(train).to(DEV))
    feat = index.feat_t[:, :N].T.double().cpu().numpy()
    worst_rel, worst_ratio = 0., 0.
    for mode, exclude in (("poses", -1), ("frames", 0), ("frames", 2)):
        qposes = queries if mode == "poses" else train[frames]
        qf = None if mode == "poses" else frames
        tq = torch.from_numpy(qposes).to(DEV)
        featq = po.pose_features(tq)[:, :Q].T.double().cpu().numpy()
        with np.errstate(invalid='ignore'):
            D64 = ref.distances(featq, feat)
        ok = ref.allowed(Q, N, qf, exclude) & np.isfinite(D64)
        for K in (1, 4, 8):
            tqf = None if qf is None else torch.from_numpy(qf).to(DEV)
            idx, d2 = po.pose_neighbors(tq, index, K, tqf, exclude, "fused")
            idx_m, d2_m = po.pose_neighbors(tq, index, K, tqf, exclude, "matrix")
            assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and tuple(idx.shape) == tuple(d2.shape) == (Q, K)
            # 1. the fused search is its witness, bit for bit
            assert torch.equal(idx, idx_m) and torch.equal(d2.view(torch.int32), d2_m.view(torch.int32)), (mode, exclude, K)
            idx, d2 = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()
            ref_idx, ref_d2 = ref.neighbors(D64, K, qf, exclude)
            for q in range(Q):
                filled = int(min(K, ok[q].sum()))
                # 8. what cannot be filled is -1 / +inf; 9. (ok leaves the NaN row out) it is never returned
                assert (idx[q, filled:] == -1).all() and np.isposinf(d2[q, filled:]).all(), (mode, exclude, K, q)
                got = idx[q, :filled]
                assert (got >= 0).all() and (got < N).all() and ok[q, got].all() and len(set(got.tolist())) == filled      # 4. distinct, allowed
                keys = list(zip(d2[q, :filled].tolist(), got.tolist()))
                assert keys == sorted(keys)                                          # 4. ascending (d2, idx)
                true = D64[q, got]
                # 2. each d2 is the float64 distance of its own idx within the summation bound
                assert (np.abs(d2[q, :filled].astype(np.float64) - true) <= D2_REL * true).all(), (mode, exclude, K, q)
                # 3. and that distance is the k-th smallest up to a swap of near-equal neighbours
                assert (true <= (1. + 2. * D2_REL) * ref_d2[q, :filled]).all(), (mode, exclude, K, q)
                pos = true > 0
                if pos.any():
                    worst_rel = max(worst_rel, float((np.abs(d2[q, :filled][pos] - true[pos]) / true[pos]).max()))
                    worst_ratio = max(worst_ratio, float((true[pos] / ref_d2[q, :filled][pos]).max()))
                if qf is not None:
                    assert (np.abs(got - qf[q]) > exclude).all()                     # 7. never itself (nor its window)
            if mode == "poses":
                # 6. a query that is a training pose finds it first at d2 = 0
                assert idx[0, 0] == 0 and d2[0, 0] == 0.
                if Q > 1 and N >= 5 and K > 1:
                    # 5. the duplicated rows come back lower index first with equal bits
                    assert idx[1, 0] == 1 and idx[1, 1] == 3 and d2[1, 0] == 0. and d2[1, 1] == 0.
            if N >= 5:
                assert not (idx == 2).any()                                          # 9. the NaN row
    print(f"pose_neighbors N={N} Q={Q}: max |d2 - d2_64| / d2_64 = {worst_rel:.3e} (bound {D2_REL:.3e}), "
          f"max d2_64(idx_k) / k-th smallest = {worst_ratio:.9f}")


def test_pose_neighbors_refuses():
    from selfreconcode_amd import posecond_ops as po
    index = po.PoseIndex.build(torch.from_numpy(_poses(6, 1)).to(DEV))
    q = torch.from_numpy(_poses(2, 2)).to(DEV)
    for K in (0, po.MAX_K + 1):
        with pytest.raises(ValueError, match="K in"):
            po.pose_neighbors(q, index, K)
    with pytest.raises(ValueError, match="method"):
        po.pose_neighbors(q, index, 2, method="tree")
    with pytest.raises(ValueError, match="query_frames"):
        po.pose_neighbors(q, index, 2, torch.arange(3, device=DEV), 0)


# ------------------------------------------------------------------------------------------------ blend
@pytest.mark.parametrize("L", [1, 128, 130])
def test_blend_codes(L):
    from selfreconcode_amd import posecond_ops as po
    N, Q = 257, 70
    rng = np.random.default_rng(L)
    index = po.PoseIndex.build(torch.from_numpy(_poses(N, 3)).to(DEV))
    q = torch.from_numpy(_poses(Q, 4)).to(DEV)
    codes_h = rng.standard_normal((N, L)).astype(np.float32)
    codes = torch.from_numpy(codes_h).to(DEV)
    cmax = float(np.abs(codes_h).max())
    for K in (1, 4, 8):
        idx, d2 = po.pose_neighbors(q, index, K)
        idx_h, d2_h = idx.cpu().numpy().astype(np.int64), d2.double().cpu().numpy()
        sigma2 = float(np.median(d2_h[:, 0])) * 0.25
        out, w = po.blend_codes(idx, d2, codes, sigma2)
        assert tuple(out.shape) == (Q, L) and tuple(w.shape) == (Q, K)
        want, want_w = ref.blend(idx_h, d2_h, codes_h, sigma2)
        err = float(np.abs(out.double().cpu().numpy() - want).max())
        sum_err = float((w.double().sum(1) - 1.).abs().max())
        print(f"blend_codes L={L} K={K}: max error {err:.3e} (bound {BLEND_TOL * cmax:.3e}), max |sum w - 1| {sum_err:.3e} (bound {WEIGHT_SUM_TOL:.3e})")
        assert err <= BLEND_TOL * cmax
        assert sum_err <= WEIGHT_SUM_TOL
        assert float(np.abs(w.double().cpu().numpy() - want_w).max()) <= BLEND_TOL
        if K == 1:
            assert torch.equal(out, codes[idx[:, 0].long()]) and bool((w == 1.).all())
        # a tiny sigma2 returns the nearest frame's code
        near, wn = po.blend_codes(idx, d2, codes, 1e-30)
        assert torch.equal(near, codes[idx[:, 0].long()]) and bool((wn[:, 0] == 1.).all()) and not bool(wn[:, 1:].any())
        assert torch.equal(po.blend_codes(idx, d2, codes, sigma2)[0], out)
    # rows without a neighbour give zeros; a row that is part filled uses what it has
    idx = torch.tensor([[-1, -1, -1], [5, -1, -1], [7, 9, -1]], dtype=torch.int32, device=DEV)
    d2 = torch.tensor([[math.inf] * 3, [0.5, math.inf, math.inf], [0.25, 0.25, math.inf]], device=DEV)
    out, w = po.blend_codes(idx, d2, codes, 1.)
    assert not bool(out[0].any()) and not bool(w[0].any())
    assert torch.equal(out[1], codes[5]) and w[1].tolist() == [1., 0., 0.]
    assert w[2].tolist() == [0.5, 0.5, 0.] and torch.equal(out[2], torch.addcmul(0.5 * codes[7], codes[9], torch.tensor(0.5, device=DEV)))


def test_blend_codes_refuses():
    from selfreconcode_amd import posecond_ops as po
    idx = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    d2 = torch.zeros((2, 2), device=DEV)
    codes = torch.zeros((4, 3), device=DEV)
    for sigma2 in (0., -1., math.nan, 1e-46):
        with pytest.raises(ValueError, match="sigma2"):
            po.blend_codes(idx, d2, codes, sigma2)
    with pytest.raises(ValueError, match="idx / d2"):
        po.blend_codes(idx, d2[:, :1], codes, 1.)


# ------------------------------------------------------------------------------------------------ calibration
def test_calibrate_sigma2():
    from selfreconcode_amd import posecond_ops as po
    N = 300
    train = torch.from_numpy(_poses(N, 9)).to(DEV)
    index = po.PoseIndex.build(train)
    for exclude in (0, 15, N - 2):
        _, d2 = po.pose_neighbors(train, index, 1, torch.arange(N, device=DEV), exclude)
        want = ref.calibrate(d2[:, 0].cpu().numpy())
        assert po.calibrate_sigma2(index, exclude) == want and want > 0.
    with pytest.raises(ValueError, match="explicit sigma"):
        po.calibrate_sigma2(index, N - 1)
    small = po.PoseIndex.build(train[:5])
    with pytest.raises(ValueError, match="explicit sigma"):
        po.calibrate_sigma2(small, 15)
