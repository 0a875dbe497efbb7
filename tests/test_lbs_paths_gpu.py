"""csrc/lbs.hip on every launch path, against the float64 references of tests/_lbs_ref.py (which tests/test_lbs_ref_cpu.py checks on
the host): the forward with frames staged in LDS (<= 8) and read from global memory, the two backward kernels with 256-thread
blocks (<= 14 frames) and 64-thread blocks (15 .. 32), wave and workgroup tails, several workgroups, frames in any order, frames
without points, the capped grid, every nullable argument, and the kinematic chain from one pose to several workgroups.

Tolerances are the project's own for these quantities (test_lbs_jacobian_backward_against_float64_autograd,
test_kinematic_chain_kernel_vs_oracle).  The Python wrappers allocate their outputs with torch.empty; `_poison` hands the allocator
NaN-filled blocks of the same sizes just before (best effort), and every output is checked to be finite in full."""
import functools
import hashlib

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
import _lbs_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Y_TOL = dict(rtol=1e-5, atol=2e-6)
J_TOL = dict(rtol=1e-4, atol=1e-5)
CHAIN_TOL = dict(rtol=2e-5, atol=2e-6)
POSEBAR_TOL = dict(rtol=2e-4, atol=2e-5)


@functools.lru_cache(maxsize=None)
def _skin():
    from selfreconcode_amd.model.Deformer import LBSkinner
    from selfreconcode_amd.utils import smpl_tmp_Apose
    return LBSkinner(fx.synthetic_lbs_volume(R.VOL_DHW), fx.LBS_BMIN, fx.LBS_BMAX, fx.synthetic_joints(), np.array(fx.SMPL_PARENTS),
                     init_pose=torch.from_numpy(smpl_tmp_Apose(1)), align_corners=False).to(DEV)


@functools.lru_cache(maxsize=None)
def _K():
    return R.constants(_skin().init_pose.cpu())


@functools.lru_cache(maxsize=None)
def _case(P, N, order, lattice=False, seed=1):
    """The seeded case, its posed transforms (the oracle's chain in double, rounded to the float32 both sides then read) and
    everything the kernels take, on the GPU."""
    c = R.make_case(P, N, order, seed=seed, lattice=lattice)
    c.A = R.transforms(c.poses, _K()).float()
    c.g = {k: getattr(c, k).to(DEV) for k in ("p", "bi", "A", "trans", "wy", "wJ")}
    return c


@functools.lru_cache(maxsize=None)
def _ref(P, N, order, kind):
    """The float64 reference of a case, computed once: 'fwd' (y, J; on-lattice points included), 'bwd' (first order), 'jac'."""
    c = _case(P, N, order, kind == "fwd")
    wy, wJ = (None, None) if kind == "fwd" else (c.wy, None) if kind == "bwd" else (c.wy, c.wJ)
    return R.lbs_reference(c.p, c.A, c.trans, c.bi, _K(), wy, wJ)


def _poison(*numels):
    junk = [torch.full((max(n, 1),), float("nan"), device=DEV) for n in numels]
    del junk                                                         # freed together: the next torch.empty of each size gets one of them


def _finite(*ts):
    for t in ts:
        assert t is not None and bool(torch.isfinite(t).all())


def _close(a, b, what, rtol, atol):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = float((a - b).abs().max()) if a.numel() else 0.0
    print(f"{what}: max|kernel - float64| = {err:.3e}, max|float64| = {float(b.abs().max()) if b.numel() else 0.0:.3e}")
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol, msg=lambda m: what + ": " + m)


def _grad_close(a, b, what):
    """rtol 1e-3, atol 1e-3 max|reference|"""
    _close(a, b, what, 1e-3, 1e-3 * float(b.abs().max()))


def _forward(c, with_jac, g=None):
    g = g or c.g
    _poison(c.P * 3, c.P * 9)
    y, J = _skin().fused(g["p"], g["A"], g["trans"], g["bi"], with_jac=with_jac)
    _finite(y, *([J] if with_jac else []))
    assert (J is None) == (not with_jac)
    return y, J


def _bwd(c, need=(True, True, True), g=None, bi="given", ppf=0):
    """sr_lbs_bwd through LBSkinner.fused_backward -> (pbar, Abar [N,24,12], transbar)"""
    g = g or c.g
    N = g["A"].shape[0]
    _poison(c.P * 3, N * 288, N * 3)
    out = _skin().fused_backward(g["p"], g["A"], g["bi"] if bi == "given" else None, ppf, g["wy"], *need)
    for o, n in zip(out, need):
        assert (o is not None) == n
        if n:
            _finite(o)
    return out


def _jac_bwd(c, need=(True, True, True), g=None, bi="given", ppf=0, ybar="given"):
    """sr_lbs_jac_bwd through _LBSValueJacobian -> (y, J, pbar, Abar [N,24,12], transbar); ybar 'given' | 'zero' | None"""
    from selfreconcode_amd.model.Deformer import _LBSValueJacobian
    g = g or c.g
    N = g["A"].shape[0]
    q, A, t = (x.clone().requires_grad_(n) for x, n in zip((g["p"], g["A"], g["trans"]), need))
    y, J = _LBSValueJacobian.apply(_skin(), q, A, t, g["bi"] if bi == "given" else None, ppf)
    ins = [x for x, n in zip((q, A, t), need) if n]
    _poison(c.P * 3, N * 288, N * 3)
    if ybar is None:
        got = list(torch.autograd.grad([J], ins, [g["wJ"]], allow_unused=True))
    else:
        got = list(torch.autograd.grad([y, J], ins, [g["wy"] if ybar == "given" else torch.zeros_like(g["wy"]), g["wJ"]], allow_unused=True))
    pbar, Abar, tbar = (got.pop(0) if n else None for n in need)
    if Abar is not None:
        assert Abar.shape == (N, 24, 4, 4) and float(Abar[:, :, 3].abs().max()) == 0.0           # the bottom row of a transform has no cotangent
        Abar = Abar[:, :, :3, :].reshape(N, 24, 12)
    _finite(y, J, *[o for o in (pbar, Abar, tbar) if o is not None])
    return y.detach(), J.detach(), pbar, Abar, tbar


def _empty_frames_are_zero(c, Abar, tbar):
    for f in c.empty:
        assert int(torch.count_nonzero(Abar[f])) == 0 and int(torch.count_nonzero(tbar[f])) == 0, f


# ------------------------------------------------------------------------------------------------ a. against float64
CASES = R.case_table()


@pytest.mark.parametrize("N,P,order", CASES)
def test_forward_against_float64(N, P, order):
    c, ref = _case(P, N, order, True), _ref(P, N, order, "fwd")
    y, _ = _forward(c, False)
    _close(y, ref.y, "y", **Y_TOL)


@pytest.mark.parametrize("N,P,order", CASES)
def test_forward_with_jacobian_against_float64(N, P, order):
    c, ref = _case(P, N, order, True), _ref(P, N, order, "fwd")
    y, J = _forward(c, True)
    _close(y, ref.y, "y", **Y_TOL)
    d = c.deriv
    assert int((~d).sum()) == P // 6                                 # only the on-lattice class is value-only
    _close(J.cpu()[d], ref.J[d], "J", **J_TOL)


@pytest.mark.parametrize("N,P,order", CASES)
def test_lbs_bwd_against_float64(N, P, order):
    c, ref = _case(P, N, order), _ref(P, N, order, "bwd")
    pbar, Abar, tbar = _bwd(c)
    _grad_close(pbar, ref.pbar, "pbar"); _grad_close(Abar, ref.Abar, "Abar"); _grad_close(tbar, ref.transbar, "transbar")
    _empty_frames_are_zero(c, Abar, tbar)


@pytest.mark.parametrize("N,P,order", CASES)
def test_lbs_jac_bwd_against_float64(N, P, order):
    c, ref = _case(P, N, order), _ref(P, N, order, "jac")
    y, J, pbar, Abar, tbar = _jac_bwd(c)
    _close(y, ref.y, "y", **Y_TOL); _close(J, ref.J, "J", **J_TOL)
    _grad_close(pbar, ref.pbar, "pbar"); _grad_close(Abar, ref.Abar, "Abar"); _grad_close(tbar, ref.transbar, "transbar")
    _empty_frames_are_zero(c, Abar, tbar)


def test_pose_gradients_through_the_chain_and_the_skinning_at_nine_frames():
    """LBSkinner.forward under autograd (chain kernel -> sr_lbs_fwd, sr_lbs_bwd -> chain backward) against the oracle from the poses."""
    c = _case(257, 9, "interleaved")
    ref = R.lbs_pose_reference(c.p, c.poses, c.trans, c.bi, _K(), c.wy)
    p, po, t = c.g["p"].clone().requires_grad_(True), c.poses.to(DEV).requires_grad_(True), c.g["trans"].clone().requires_grad_(True)
    y = _skin()(p, [po, t], c.g["bi"])
    got = torch.autograd.grad((y * c.g["wy"]).sum(), [p, po, t])
    for name, a, b in zip(("pbar", "posebar", "transbar"), got, ref):
        _finite(a); _grad_close(a, b, name)


# ------------------------------------------------------------------------------------------------ b. the capped grid
def _workspace_rows(P, N):
    from selfreconcode_amd import _lib
    return int(_lib.raw("sr_lbs_bwd_workspace_floats")(P, N)) // (N * 291)


# 64- and 256-thread blocks.  The grid is sized for 256-thread blocks and capped at 512 workgroups whatever the block shape: at three
# frames the cap binds (512 workgroups, two passes of the grid-stride loop), at fifteen the 129 workgroups of 64 threads take four.
GRID_CASES = [(15, 32768 + 65, "interleaved", 32768, 129), (3, 131072 + 257, "sorted", 131072, 512)]


@pytest.mark.parametrize("N,P,order,chunk,rows", GRID_CASES)
def test_grid_capped_lbs_bwd_against_float64(N, P, order, chunk, rows):
    c = _case(P, N, order)
    assert _workspace_rows(P, N) == rows and _workspace_rows(chunk, N) == chunk // 256 and P > rows * (64 if N > 14 else 256)
    ref = R.lbs_reference(c.p, c.A, c.trans, c.bi, _K(), c.wy, None)
    pbar, Abar, tbar = _bwd(c)
    _grad_close(pbar, ref.pbar, "pbar"); _grad_close(Abar, ref.Abar, "Abar"); _grad_close(tbar, ref.transbar, "transbar")


def _chunk_of(c, lo, hi):
    g = dict(c.g)
    for k in ("p", "bi", "wy", "wJ"):
        g[k] = c.g[k][lo:hi].contiguous()
    return type(c)(P=hi - lo), g


@pytest.mark.parametrize("N,P,order,chunk,rows", GRID_CASES)
def test_grid_capped_jac_bwd_equals_its_chunks(N, P, order, chunk, rows):
    """pbar is per point: bit-equal to the same points launched in chunks at or below the cap (one pass of the grid-stride loop at
    256 threads); Abar and transbar against the double-precision sum of the chunks' outputs."""
    c = _case(P, N, order)
    y, J, pbar, Abar, tbar = _jac_bwd(c)
    As, ts = torch.zeros(N, 24, 12, dtype=torch.float64), torch.zeros(N, 3, dtype=torch.float64)
    for lo in range(0, P, chunk):
        hi = min(P, lo + chunk)
        cc, g = _chunk_of(c, lo, hi)
        yc, Jc, pc, Ac, tc = _jac_bwd(cc, g=g)
        assert torch.equal(yc, y[lo:hi]) and torch.equal(Jc, J[lo:hi]) and torch.equal(pc, pbar[lo:hi]), (lo, hi)
        As += Ac.cpu().double(); ts += tc.cpu().double()
    _grad_close(Abar, As, "Abar"); _grad_close(tbar, ts, "transbar")


def test_forward_grid_stride_equals_its_chunks():
    """sr_lbs_fwd caps its grid at 2048 workgroups of 256: beyond 524288 points a thread takes a second point."""
    N, P, chunk = 9, 2048 * 256 + 257, 2048 * 256
    p = torch.from_numpy(R.interior_points(P, 77)).to(DEV)
    bi = torch.from_numpy(R.frame_ids(P, N, "interleaved")).to(DEV)
    c = _case(257, N, "interleaved")
    skin, A, t = _skin(), c.g["A"], c.g["trans"]
    y, J = skin.fused(p, A, t, bi, with_jac=True)
    y0, _ = skin.fused(p, A, t, bi, with_jac=False)
    _finite(y, J, y0)
    for lo, hi in ((0, chunk), (chunk, P)):
        yc, Jc = skin.fused(p[lo:hi].contiguous(), A, t, bi[lo:hi].contiguous(), with_jac=True)
        yc0, _ = skin.fused(p[lo:hi].contiguous(), A, t, bi[lo:hi].contiguous(), with_jac=False)
        assert torch.equal(yc, y[lo:hi]) and torch.equal(Jc, J[lo:hi]) and torch.equal(yc0, y0[lo:hi])
    tail = slice(P - 300, P)
    ref = R.lbs_reference(p[tail].cpu(), c.A, c.trans, bi[tail].cpu(), _K())
    _close(y[tail], ref.y, "y", **Y_TOL); _close(y0[tail], ref.y, "y", **Y_TOL); _close(J[tail], ref.J, "J", **J_TOL)


# ------------------------------------------------------------------------------------------------ c. equivalences, bit for bit
def test_three_frames_among_twelve_equal_the_three_alone():
    """Same points and transforms as frames (1, 5, 10) of 12 -- transforms read from global memory -- and as 3 frames staged in LDS.
    Both counts use 256-thread backward blocks."""
    c = _case(1000, 3, "interleaved")
    used = torch.tensor([1, 5, 10])
    big = _case(257, 12, "sorted", seed=2)                          # the nine other frames: some other transforms
    g = dict(c.g)
    A12, t12 = big.A.clone(), big.trans.clone()
    A12[used], t12[used] = c.A, c.trans
    g["A"], g["trans"], g["bi"] = A12.to(DEV), t12.to(DEV), used.to(DEV)[c.g["bi"]]
    for jac in (False, True):
        a, b = _forward(c, jac), _forward(c, jac, g)
        assert torch.equal(a[0], b[0]) and (not jac or torch.equal(a[1], b[1]))
    unused = torch.tensor([f for f in range(12) if f not in used.tolist()])
    for run in (_bwd, lambda c, g=None: _jac_bwd(c, g=g)[2:]):
        (p3, A3, t3), (p12, A12b, t12b) = run(c), run(c, g=g)
        assert torch.equal(p3, p12)
        assert torch.equal(A3.cpu(), A12b.cpu()[used]) and torch.equal(t3.cpu(), t12b.cpu()[used])
        assert int(torch.count_nonzero(A12b.cpu()[unused])) == 0 and int(torch.count_nonzero(t12b.cpu()[unused])) == 0


@pytest.mark.parametrize("N,V", [(3, 85), (9, 29), (15, 70)])
def test_points_per_frame_equals_explicit_batch_indices(N, V):
    """batch_inds == NULL with points_per_frame (the [N,V,3] call form) against the same frames spelled out"""
    P = N * V
    c = _case(P, N, "sorted")
    assert torch.equal(c.bi, torch.arange(P) // V)
    skin, g = _skin(), c.g
    for jac in (False, True):
        a = _forward(c, jac)
        _poison(P * 3, P * 9)
        y, J = skin.fused(g["p"].view(N, V, 3), g["A"], g["trans"], None, with_jac=jac)
        assert y.shape == (N, V, 3) and torch.equal(y.view(-1, 3), a[0]) and (not jac or torch.equal(J, a[1]))
    for run in (_bwd, lambda c, **k: _jac_bwd(c, **k)[2:]):
        for a, b in zip(run(c), run(c, bi=None, ppf=V)):
            assert torch.equal(a, b)
    ref = _ref(P, N, "sorted", "jac")
    y, J, pbar, Abar, tbar = _jac_bwd(c, bi=None, ppf=V)             # and the path itself against float64
    _close(y, ref.y, "y", **Y_TOL); _close(J, ref.J, "J", **J_TOL)
    _grad_close(pbar, ref.pbar, "pbar"); _grad_close(Abar, ref.Abar, "Abar"); _grad_close(tbar, ref.transbar, "transbar")


@pytest.mark.parametrize("N,P", [(3, 1000), (15, 257)])
def test_permuting_the_points_permutes_the_per_point_outputs(N, P):
    c = _case(P, N, "interleaved")
    perm = torch.from_numpy(np.argsort(fx.det_array((P,), 91, 1.0, np.float64), kind="stable")).to(DEV)
    g = dict(c.g)
    for k in ("p", "bi", "wy", "wJ"):
        g[k] = c.g[k][perm].contiguous()
    y, J = _forward(c, True)
    yp, Jp = _forward(c, True, g)
    assert torch.equal(yp, y[perm]) and torch.equal(Jp, J[perm])
    assert torch.equal(_bwd(c, g=g)[0], _bwd(c)[0][perm])
    assert torch.equal(_jac_bwd(c, g=g)[2], _jac_bwd(c)[2][perm])


@pytest.mark.parametrize("N,P", [(3, 1000), (14, 1000), (15, 1000), (32, 257)])
def test_backward_is_reproducible_on_interleaved_frames(N, P):
    """csrc/lbs.hip's claim for the per-frame sums: bit-reproducible run to run, whatever the schedule"""
    c = _case(P, N, "interleaved")
    for a, b in zip(_bwd(c), _bwd(c)):
        assert torch.equal(a, b)
    for a, b in zip(_jac_bwd(c), _jac_bwd(c)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ d. nullable arguments
@pytest.mark.parametrize("N,P,order", [(3, 257, "interleaved"), (15, 255, "empty")])
def test_each_output_absent_in_turn(N, P, order):
    c = _case(P, N, order)
    full, full_jac = _bwd(c), _jac_bwd(c)[2:]
    for absent in range(3):
        need = tuple(k != absent for k in range(3))
        for got, want in ((_bwd(c, need), full), (_jac_bwd(c, need)[2:], full_jac)):
            for k in range(3):
                assert (got[k] is None) if k == absent else torch.equal(got[k], want[k]), (absent, k)


@pytest.mark.parametrize("N,P,order", [(3, 257, "interleaved"), (15, 255, "empty")])
def test_jac_bwd_without_ybar_equals_a_zero_ybar(N, P, order):
    c = _case(P, N, order)
    _, _, p0, A0, t0 = _jac_bwd(c, ybar="zero")
    _, _, p1, A1, t1 = _jac_bwd(c, ybar=None)
    assert torch.equal(p0, p1) and torch.equal(A0, A1)
    assert t1 is None and int(torch.count_nonzero(t0)) == 0         # no ybar: the translations get no gradient at all
    ref = R.lbs_reference(c.p, c.A, c.trans, c.bi, _K(), None, c.wJ)
    _grad_close(p1, ref.pbar, "pbar"); _grad_close(A1, ref.Abar, "Abar")
    _empty_frames_are_zero(c, A1, t0)


def test_forward_with_lookup_points_against_float64():
    """tp != NULL: weights looked up at tps (all three point classes), transforms applied to ps; 300 points over 9 frames"""
    c = _case(300, 9, "interleaved", True)
    ps = fx.det_tensor((300, 3), 95, 0.8)
    ref = R.lbs_reference(ps, c.A, c.trans, c.bi, _K(), tps=c.p)
    _poison(900)
    y, J = _skin().fused(ps.to(DEV), c.g["A"], c.g["trans"], c.g["bi"], tps=c.g["p"])
    assert J is None
    _finite(y); _close(y, ref.y, "y", **Y_TOL)
    assert float((ref.y - R.lbs_reference(ps, c.A, c.trans, c.bi, _K()).y).abs().max()) > 1e-3      # (and the lookup point matters)
    from selfreconcode_amd import _lib
    with pytest.raises(_lib.SrError, match="SR_EINVAL"):            # the analytic Jacobian is for weights looked up at p itself
        _skin().fused(ps.to(DEV), c.g["A"], c.g["trans"], c.g["bi"], with_jac=True, tps=c.g["p"])


@pytest.mark.parametrize("N", [3, 15])
def test_no_points_zero_fill_the_frame_sums(N):
    c = _case(64, N, "sorted")
    cc = type(c)(P=0)
    g = dict(c.g)
    g["p"], g["bi"], g["wy"], g["wJ"] = (torch.zeros(s, device=DEV, dtype=d) for s, d in
                                          (((0, 3), torch.float32), ((0,), torch.int64), ((0, 3), torch.float32), ((0, 3, 3), torch.float32)))
    pbar, Abar, tbar = _bwd(cc, g=g)
    assert pbar.shape == (0, 3) and Abar.shape == (N, 24, 12) and int(torch.count_nonzero(Abar)) == 0 and int(torch.count_nonzero(tbar)) == 0
    y, J, pbar, Abar, tbar = _jac_bwd(cc, g=g)
    assert y.shape == (0, 3) and J.shape == (0, 3, 3) and pbar.shape == (0, 3)
    assert Abar.shape == (N, 24, 12) and int(torch.count_nonzero(Abar)) == 0 and int(torch.count_nonzero(tbar)) == 0


def test_thirty_three_frames_forward_runs_backward_is_refused():
    """The forward has no frame limit (beyond 8 it reads the transforms from global memory); the backward kernels hold one LDS row
    per frame and both entry points refuse more than 32 frames before they launch anything."""
    from selfreconcode_amd import _lib
    c = _case(300, 33, "interleaved", True)
    ref = R.lbs_reference(c.p, c.A, c.trans, c.bi, _K())
    y, J = _forward(c, True)
    _close(y, ref.y, "y", **Y_TOL); _close(J.cpu()[c.deriv], ref.J[c.deriv], "J", **J_TOL)
    with pytest.raises(_lib.SrError, match="sr_lbs_bwd failed: SR_EINVAL"):
        _bwd(c)
    with pytest.raises(RuntimeError, match="sr_lbs_jac_bwd failed: SR_EINVAL"):
        _jac_bwd(c)
    torch.cuda.synchronize()
    y2, _ = _forward(c, False)                                       # nothing was launched, nothing is broken afterwards
    _close(y2, ref.y, "y", **Y_TOL)


# ------------------------------------------------------------------------------------------------ e. the kinematic chain
@functools.lru_cache(maxsize=None)
def _chain_ref(B, cot):
    wA = fx.det_tensor((B, 24, 4, 4), 62, 1.0) if cot in ("A", "both") else None
    wG = fx.det_tensor((B, 24, 4, 4), 63, 1.0) if cot in ("G", "both") else None
    return wA, wG, R.chain_reference(R.chain_poses(B), _K(), wA, wG)


@pytest.mark.parametrize("cot", ["A", "G", "both"])
@pytest.mark.parametrize("B", [1, 31, 32, 33, 64, 100])
def test_kinematic_chain_against_float64(B, cot):
    """One workgroup covers 32 poses: a lone pose, a full workgroup less one, exactly one, one more, two, and a ragged fourth; poses with
    exact-zero joints, a whole zero pose, rotations of 1e-4 and rotations near pi (R.chain_poses)."""
    wA, wG, ref = _chain_ref(B, cot)
    poses = R.chain_poses(B).to(DEV).requires_grad_(True)
    _poison(B * 384, B * 384)
    G, A = _skin().posed_chain(poses)
    _finite(G, A)
    _close(G, ref.G, "G", **CHAIN_TOL); _close(A, ref.A, "A", **CHAIN_TOL)
    bottom = torch.tensor([0., 0., 0., 1.], device=DEV).expand(B, 24, 4)
    assert torch.equal(G[:, :, 3], bottom) and torch.equal(A[:, :, 3], bottom)
    outs, cots = zip(*[(o, w.to(DEV)) for o, w in ((A, wA), (G, wG)) if w is not None])
    _poison(B * 72)
    posebar, = torch.autograd.grad(outs, poses, cots)
    _finite(posebar)
    assert posebar.shape == (B, 24, 3)
    _close(posebar, ref.posebar, "posebar", **POSEBAR_TOL)
    if B > 2:                                                        # posedSkeleton takes a whole sequence: the joints are G's translations
        J = _skin().posedSkeleton([poses.detach(), torch.zeros(B, 3, device=DEV)])
        _close(J, ref.newJ, "posed joints", **CHAIN_TOL)


# ------------------------------------------------------------------------------------------------ f. the recorded bits
# The smallest cases that reach each launch path: frames staged in LDS, 256-thread backward blocks, a workgroup of one point and
# several frame passes per wave (3 frames); transforms read from global memory in the forward (9); 64-thread backward blocks, a
# ragged last wave and frames without points (15).
PIN_CASES = [(3, 257, "interleaved"), (9, 257, "interleaved"), (15, 255, "empty")]
PIN_CHAIN_B = 33


def lbs_path_digests():
    """name -> SHA-256 (as 32 uint8), in a fixed order, of the bytes of every output of the LBS kernels on PIN_CASES and of the kinematic chain, forward and
    backward with both cotangents, at PIN_CHAIN_B poses.  oracle/gen_lbs_paths_golden.py records what this returns."""
    out = {}

    def put(name, t):
        out[name] = torch.from_numpy(np.frombuffer(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).digest(), np.uint8).copy())

    for N, P, order in PIN_CASES:
        c, tag = _case(P, N, order), f"n{N}_"
        for name, t in zip(("fwd_jac_y", "fwd_jac_J"), _forward(c, True)):
            put(tag + name, t)
        put(tag + "fwd_y", _forward(c, False)[0])
        for name, t in zip(("bwd_pbar", "bwd_Abar", "bwd_transbar"), _bwd(c)):
            put(tag + name, t)
        for name, t in zip(("jac_y", "jac_J", "jac_pbar", "jac_Abar", "jac_transbar"), _jac_bwd(c)):
            put(tag + name, t)
    B = PIN_CHAIN_B
    poses = R.chain_poses(B).to(DEV).requires_grad_(True)
    G, A = _skin().posed_chain(poses)
    posebar, = torch.autograd.grad([A, G], poses, [fx.det_tensor((B, 24, 4, 4), 62, 1.0).to(DEV), fx.det_tensor((B, 24, 4, 4), 63, 1.0).to(DEV)])
    put("chain_G", G); put("chain_A", A); put("chain_posebar", posebar)
    return out


def test_every_launch_path_gives_the_recorded_bits(golden):
    """Pins the kernels bit for bit on the paths that the float64 tests above hold to a tolerance.  tests/golden/lbs_paths.npz holds the
    digests that oracle/gen_lbs_paths_golden.py recorded with the kernels as they were before csrc/rot_device.h existed; a change that
    means to keep the bits does not record it again."""
    g, out = golden("lbs_paths")["digests"], lbs_path_digests()
    assert g.shape == (len(out), 32) and len(out) == 11 * len(PIN_CASES) + 3
    for want, (k, v) in zip(g, out.items()):
        assert torch.equal(v, want), k
