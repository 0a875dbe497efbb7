"""Every launch of the device-driven refiner (csrc/refiner.hip) and of the per-ray newton kernels (csrc/tracer.hip) alone, on synthetic
buffers, against the float64 restatement and the error budgets of tests/_refiner_ref.py (proved on the host by
tests/test_refiner_ref_cpu.py).  The kernels take a plain struct of raw pointers, so sdf_out, def_out, the cotangent rows and t
are just buffers here: no network, no chain, no iteration.

Every buffer carries guard rows and starts as a sentinel (a NaN with a payload no arithmetic produces, -1, 0xAB); a launch may
change exactly what its contract says it writes -- everything else is compared bit for bit with its state before the launch.
A queue is compared as a set (ordered by original index): the contract leaves the slot order across waves free.
Each test prints `ratio <launch> <quantity> <max error / bound>`; profiles/refiner_kernels.md holds the measured values."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import torch_oracle as orc
import _lbs_ref as R
import _refiner_ref as F
import test_lbs_paths_gpu as LP           # the LBS tests' skinner and constants: the volume, box and init pose both sides read

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 3
SENT_BITS = 0x7FC0ABCD
f32 = np.float32
NS = F.SimpleNamespace

MS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
NFRAMES = (1, 8, 9, 32)
P_ENQ = 2048 * 16 + 17                   # CHECK / finish take 16 rays per workgroup on a grid capped at 2048: two passes + a tail
P_RAY = 2048 * 256 + 1                   # STEP / FINAL and the newton kernels take 256


def _geom(i):
    N, order = NFRAMES[i % 4], R.ORDERS[(i // 4 + i) % 4]
    return N, ("last" if N == 1 and order == "empty" else order)


# ------------------------------------------------------------------------------------------------ buffers
def _full(shape, kind):
    if kind == "f":
        return torch.full(shape, SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full(shape, -1 if kind == "i" else 0xAB, dtype=torch.int32 if kind == "i" else torch.uint8, device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _pitch(n, how):
    return n if how == "exact" else n + (-n) % 4 if n % 4 else n + 4


@functools.lru_cache(maxsize=None)
def _frames(N):
    c = R.make_case(1, N, "sorted")
    return R.transforms(c.poses, LP._K()).float(), c.trans


class Rig:
    """The buffers of one sr_refine_args on the GPU, every one with GUARD rows beyond the capacity P."""

    def __init__(self, P, times=2, N=1, L_sdf=6, L_def=6, E=128, pitch="exact", rows=True, bars=False, bar_pitch="exact", n_skip=None,
                 ld_sdf=1, ld_def=3, A=None, trans=None):
        self.P, self.times, self.N, self.L_sdf, self.L_def, self.E, self.rows, self.n_skip = P, times, N, L_sdf, L_def, E, rows, n_skip
        self.ld_a0, self.ld_a0d = _pitch(3 + 6 * L_sdf, pitch), _pitch(3 + 6 * L_def + E, pitch)
        self.ld_a0bar, self.ld_a0dbar = _pitch(3 + 6 * L_sdf, bar_pitch), _pitch(3 + 6 * L_def + E, bar_pitch)
        self.ld_skipbar = 0 if n_skip is None else _pitch(n_skip, bar_pitch)
        self.ld_sdf, self.ld_def = ld_sdf, ld_def
        self.w_sdf = np.asarray(orc.resolve_pe_weights(L_sdf, 0.8), f32) if L_sdf else np.zeros(0, f32)
        self.w_def = np.asarray(orc.resolve_pe_weights(L_def, 0.62), f32) if L_def else np.zeros(0, f32)
        self.conds = fx.det_array((N, max(E, 1)), 12, 0.1, f32)
        if A is None:
            A, trans = _frames(N)
        assert A.shape[0] == N
        R_ = P + GUARD
        T = dict(live=_full((times + 3 + GUARD,), "i"), unit=_full((R_, 4), "f"), conv=_full((R_,), "b"), t=_full((R_, 4), "f"), s=_full((R_,), "f"),
                 sdf_out=_full((R_, ld_sdf), "f"), def_out=_full((R_, ld_def), "f"), p_out=_full((R_, 3), "f"), conv_out=_full((R_,), "b"),
                 p0=_full((R_, 3), "f"), rays=_full((R_, 3), "f"), batch_inds=torch.zeros(R_, dtype=torch.int64, device=DEV))
        for i in range(2):
            T[f"x{i}"], T[f"v{i}"], T[f"frame{i}"], T[f"orig{i}"] = _full((R_, 3), "f"), _full((R_, 3), "f"), _full((R_,), "i"), _full((R_,), "i")
        if rows:
            T["a0"], T["a0d"] = _full((R_, self.ld_a0), "f"), _full((R_, self.ld_a0d), "f")
        if bars:
            T["a0bar"], T["a0dbar"] = _full((R_, self.ld_a0bar), "f"), _full((R_, self.ld_a0dbar), "f")
            if n_skip is not None:
                T["skipbar"] = _full((R_, self.ld_skipbar), "f")
        self.T = T
        self.C = dict(cam=_dev(F.CAM), w_sdf=_dev(np.append(self.w_sdf, f32(0))), w_def=_dev(np.append(self.w_def, f32(0))), conds=_dev(self.conds),
                      A=A.to(DEV), trans=trans.float().to(DEV))

    def put(self, name, a, col=None):
        a = _dev(a)
        if col is None:
            self.T[name][:a.shape[0]] = a
        else:
            self.T[name][:a.shape[0], col] = a

    def put_queue(self, cur, x, v, frame, orig):
        self.put(f"x{cur}", x); self.put(f"v{cur}", v); self.put(f"frame{cur}", frame.astype(np.int32)); self.put(f"orig{cur}", orig.astype(np.int32))

    def put_live(self, phase, M):
        live = np.zeros(self.times + 3, np.int32)
        live[phase] = M
        self.put("live", live)

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in self.T.items()}

    def args(self):
        from selfreconcode_amd import _lib
        T, C, p = self.T, self.C, _lib.ptr
        a = _lib.SrRefineArgs()
        a.P, a.times = self.P, self.times
        a.p0, a.rays, a.batch_inds, a.cam = p(T["p0"]), p(T["rays"]), p(T["batch_inds"]), p(C["cam"])
        a.L_sdf, a.w_sdf, a.L_def, a.w_def = self.L_sdf, p(C["w_sdf"]), self.L_def, p(C["w_def"])
        a.conds, a.ld_conds, a.E = p(C["conds"]), self.conds.shape[1], self.E
        self.keep = LP._skin().fill_lbs_fields(a, C["A"], C["trans"])
        a.dthreshold, a.athreshold, a.w1, a.w2 = float(F.DTHR), float(F.ATHR), float(F.W1), float(F.W2)
        a.live = p(T["live"])
        for i in range(2):
            a.x[i], a.v[i], a.frame[i], a.orig[i] = p(T[f"x{i}"]), p(T[f"v{i}"]), p(T[f"frame{i}"]), p(T[f"orig{i}"])
        a.unit, a.conv, a.t, a.s = p(T["unit"]), p(T["conv"]), p(T["t"]), p(T["s"])
        a.a0, a.ld_a0, a.a0d, a.ld_a0d = p(T.get("a0")), self.ld_a0, p(T.get("a0d")), self.ld_a0d
        a.sdf_out, a.ld_sdf, a.def_out, a.ld_def = p(T["sdf_out"]), self.ld_sdf, p(T["def_out"]), self.ld_def
        a.a0bar, a.ld_a0bar, a.a0dbar, a.ld_a0dbar = p(T.get("a0bar")), self.ld_a0bar, p(T.get("a0dbar")), self.ld_a0dbar
        a.skipbar, a.ld_skipbar, a.n_skip = p(T.get("skipbar")), self.ld_skipbar, self.n_skip or 0
        a.p_out, a.conv_out = p(T["p_out"]), p(T["conv_out"])
        return a

    def launch(self, name, *ints):
        """-> (state before, state after) on the host"""
        from selfreconcode_amd import _lib
        before = self.snapshot()
        a = self.args()
        with torch.cuda.device(0):
            _lib.call(name, ctypes.byref(a), *ints, _lib.stream_of(self.T["live"]))
        return before, self.snapshot()


def _only_changed(before, after, allowed):
    """Bit for bit, nothing but `allowed` (name -> boolean mask of the elements the contract writes) differs from before."""
    assert set(allowed) <= set(before)
    for k in before:
        changed = _bits(before[k]) != _bits(after[k])
        mask = allowed.get(k)
        if mask is not None:
            changed &= ~np.broadcast_to(mask.reshape(mask.shape + (1,) * (changed.ndim - mask.ndim)), changed.shape)
        assert not changed.any(), (k, np.argwhere(changed)[:5].tolist())


def _head(arr, n):
    m = np.zeros(arr.shape[0], bool)
    m[:n] = True
    return m


def _at(arr, idx):
    m = np.zeros(arr.shape[0], bool)
    m[idx] = True
    assert m.sum() == len(idx)                                              # no index twice
    return m


RATIOS = {}


def _within(launch, what, got, ref, tol):
    """|got - ref| <= tol elementwise (tol 0: equal; tol inf: unconstrained but finite); prints the largest error / bound."""
    got, ref, tol = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(tol, np.float64), np.shape(ref))
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), (launch, what, "non-finite output")
    pos = np.isfinite(tol) & (tol > 0)
    ratio = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    RATIOS[(launch, what)] = max(RATIOS.get((launch, what), 0.0), ratio)
    print(f"ratio {launch} | {what} | {ratio:.3f}")
    bad = ~(err <= tol)
    assert not bad.any(), (launch, what, ratio, np.argwhere(bad)[:5].tolist())


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b))), what


def _check_rows(launch, rig, a0, a0d, x, frame):
    """First-layer input rows of both networks for the rays (x, frame), against float64: coordinates, codes and pad columns exact."""
    for got, L, w, conds, E, ld, what in ((a0, rig.L_sdf, rig.w_sdf, None, 0, rig.ld_a0, "a0"), (a0d, rig.L_def, rig.w_def, rig.conds, rig.E, rig.ld_a0d, "a0d")):
        ref, tol = F.embed_rows(x, frame, L, w, conds, E, ld)
        assert got.shape == ref.shape
        _within(launch, what + " sin/cos", got, ref, tol)


def _queue_of(state, i):
    return state[f"x{i}"], state[f"v{i}"], state[f"frame{i}"], state[f"orig{i}"]


# ------------------------------------------------------------------------------------------------ sr_refine_init
INIT = [(1000, 2, 6, 6, 128, "exact", True), (1000, 2, 6, 6, 128, "pad", True), (257, 2, 0, 0, 0, "exact", True), (257, 2, 0, 6, 128, "pad", True),
        (65, 2, 10, 10, 0, "pad", True), (1000, 2, 10, 6, 128, "exact", True), (1000, 2, 6, 6, 128, "exact", False), (1, 30, 6, 6, 128, "pad", True),
        (0, 2, 6, 6, 128, "exact", True), (P_ENQ, 1, 6, 0, 0, "exact", True)]


@pytest.mark.parametrize("P,times,L_sdf,L_def,E,pitch,rows", INIT)
def test_init(P, times, L_sdf, L_def, E, pitch, rows):
    N = 5
    rig = Rig(P, times, N, L_sdf, L_def, E, pitch, rows)
    p0, rays, bi = fx.det_array((P, 3), 41, 1.2, f32), fx.det_array((P, 3), 42, 1.0, f32), (np.arange(P) * 3) % N
    rig.put("p0", p0); rig.put("rays", rays); rig.put("batch_inds", bi.astype(np.int64))
    before, after = rig.launch("sr_refine_init")
    _same_bits(after["x0"][:P], p0, "x"); _same_bits(after["v0"][:P], rays, "v")
    assert np.array_equal(after["frame0"][:P], bi) and np.array_equal(after["orig0"][:P], np.arange(P))
    assert np.array_equal(after["unit"][:P], np.tile(np.array([1, 0, 0, 0], f32), (P, 1)))
    assert after["live"][:times + 3].tolist() == [P] + [0] * (times + 2)
    allowed = {k: _head(after[k], P) for k in ("x0", "v0", "frame0", "orig0", "unit")}
    allowed["live"] = _head(after["live"], times + 3)
    if rows:
        allowed["a0"] = allowed["a0d"] = _head(after["a0"], P)
        _check_rows("init", rig, after["a0"][:P], after["a0d"][:P], p0, bi)
    _only_changed(before, after, allowed)


# ------------------------------------------------------------------------------------------------ sr_refine_embed
@pytest.mark.parametrize("phase,M,L_sdf,L_def,E,pitch", [(2, 257, 6, 6, 128, "exact"), (3, 257, 6, 6, 128, "pad"), (3, 1000, 10, 0, 0, "exact"), (2, 1, 0, 10, 128, "pad")])
def test_embed(phase, M, L_sdf, L_def, E, pitch):
    N, P = 9, M + 21
    rig = Rig(P, 2, N, L_sdf, L_def, E, pitch)
    x, frame = fx.det_array((M, 3), 43, 1.2, f32), (np.arange(M) * 5) % N
    rig.put_queue(phase & 1, x, fx.det_array((M, 3), 44, 1.0, f32), frame, np.arange(M)[::-1])
    rig.put_live(phase, M)
    before, after = rig.launch("sr_refine_embed", phase)
    _check_rows("embed", rig, after["a0"][:M], after["a0d"][:M], x, frame)
    _only_changed(before, after, dict(a0=_head(after["a0"], M), a0d=_head(after["a0"], M)))


# ------------------------------------------------------------------------------------------------ sr_refine_mid
@functools.lru_cache(maxsize=None)
def _mid_case(M, N, order, mix, jac, seed=1):
    return F.make_mid_case(M, N, order, mix, LP._K(), seed=seed, jac=jac)


@functools.lru_cache(maxsize=None)
def _mid_ref(mode, M, N, order, mix, jac, seed=1):
    c = _mid_case(M, N, order, mix, jac, seed)
    return F.mid(mode, NS(x=c.x, v=c.v, frame=c.frame, orig=np.arange(c.M)), c.f, c.off, c.lbs)


def _mid_rig(M, c, idx, phase, times=2, rows=False, pitch="exact", ld_sdf=1, ld_def=3):
    P = M + 37
    rig = Rig(P, times, c.N, rows=rows, pitch=pitch, ld_sdf=ld_sdf, ld_def=ld_def, A=c.A, trans=c.trans)
    orig = (P - 1 - np.arange(M)).astype(np.int32)
    rig.put_queue(phase & 1, c.x[idx], c.v[idx], c.frame[idx], orig)
    rig.put("sdf_out", c.f[idx], col=0)
    for k in range(3):
        rig.put("def_out", c.off[idx, k], col=k)
    rig.put_live(phase, M)
    return rig, orig


def _canonical(after, nxt, n, orig_retired):
    q = F.queue_sorted(*_queue_of(after, nxt), n)
    return [_bits(np.ascontiguousarray(a)) for a in (q.x, q.v, q.frame, q.orig, after["p_out"][orig_retired], after["conv_out"][orig_retired])]


def _run_check(M, N, order, mix, rows, pitch="exact", phase=0):
    c = _mid_case(min(M, 1000), N, order, mix, False)
    idx = np.arange(M) % c.M
    ok = _mid_ref(F.CHECK, c.M, N, order, mix, False).ok[idx]
    runs = []
    for rep in range(2):                                                    # two launches of the same case: same retired values, same queue as a set
        rig, orig = _mid_rig(M, c, idx, phase, rows=rows, pitch=pitch, ld_sdf=2, ld_def=4)
        before, after = rig.launch("sr_refine_mid", phase, F.CHECK)
        nxt, n = (phase & 1) ^ 1, int(after["live"][phase + 1])
        assert n == int((~ok).sum())
        runs.append(_canonical(after, nxt, n, orig[ok]))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    q = F.queue_sorted(*_queue_of(after, nxt), n)
    kept = np.nonzero(~ok)[0]
    kept = kept[np.argsort(orig[kept], kind="stable")]
    _same_bits(q.x, c.x[idx][kept], "x"); _same_bits(q.v, c.v[idx][kept], "v")
    assert np.array_equal(q.frame, c.frame[idx][kept]) and np.array_equal(q.orig, orig[kept])
    _same_bits(after["p_out"][orig[ok]], c.x[idx][ok], "retired position")                        # a copy: bit-exact
    assert (after["conv_out"][orig[ok]] == 1).all()
    allowed = {k: _head(after[k], n) for k in (f"x{nxt}", f"v{nxt}", f"frame{nxt}", f"orig{nxt}")}
    allowed["live"] = _at(after["live"], [phase + 1])
    allowed["p_out"] = allowed["conv_out"] = _at(after["p_out"], orig[ok])
    if rows:
        allowed["a0"] = allowed["a0d"] = _head(after["a0"], n)
        _check_rows("mid CHECK", rig, after["a0"][:n][q.perm], after["a0d"][:n][q.perm], q.x, q.frame)
    _only_changed(before, after, allowed)
    print(f"CHECK M={M} N={N} {order} {mix}: {int(ok.sum())} retired, {n} kept")


@pytest.mark.parametrize("i,M", list(enumerate(MS)))
def test_mid_check(i, M):
    _run_check(M, *_geom(i), "half", rows=(i % 2 == 0), pitch=("pad" if i % 4 == 0 else "exact"))


@pytest.mark.parametrize("M,mix", [(257, "all"), (257, "none"), (257, "one"), (1, "all"), (1, "none"), (17, "one")])
def test_mid_check_mixtures(M, mix):
    _run_check(M, 8, "interleaved", mix, rows=True)


def test_mid_check_grid_stride():
    _run_check(P_ENQ, 9, "interleaved", "half", rows=True)


def _run_step(M, N, order, phase, big=False):
    c = _mid_case(min(M, 1000), N, order, "half", True)
    idx = np.arange(M) % c.M
    ref = _mid_ref(F.STEP, c.M, N, order, "half", True)
    rig, orig = _mid_rig(M, c, idx, phase, ld_sdf=1 if big else 3, ld_def=3 if big else 5)
    before, after = rig.launch("sr_refine_mid", phase, F.STEP)
    assert np.array_equal(after["conv"][:M], ref.conv[idx].astype(np.uint8))
    if M >= 16:
        assert (after["s"][:M][idx == 5] == 0).all() and (after["t"][:M][idx == 5] == 0).all()         # v = 0: |u| = 0, e = 0 exactly
    assert (after["t"][:M, 3] == 0).all()
    _within("mid STEP", "s", after["s"][:M], ref.s[idx], ref.ds[idx])
    _within("mid STEP", "t", after["t"][:M], ref.t[idx], ref.dt[idx])
    s = ref.s[ref.s > 0]
    assert M < 255 or (s.min() < 1e-5 and s.max() > 0.2)                                         # the kappa scaling of the bound is exercised
    _only_changed(before, after, dict(conv=_head(after["conv"], M), t=_head(after["t"], M), s=_head(after["s"], M)))


@pytest.mark.parametrize("i,M", list(enumerate(MS)))
def test_mid_step(i, M):
    _run_step(M, *_geom(i + 1), phase=1 + i % 2)


def test_mid_step_grid_stride():
    _run_step(P_RAY, 8, "sorted", 2, big=True)


def _run_final(M, N, order, times, big=False):
    phase = times + 1
    c = _mid_case(min(M, 1000), N, order, "half", False)
    idx = np.arange(M) % c.M
    ok = _mid_ref(F.FINAL, c.M, N, order, "half", False).ok[idx]
    rig, orig = _mid_rig(M, c, idx, phase, times=times, ld_sdf=1 if big else 2, ld_def=3)
    before, after = rig.launch("sr_refine_mid", phase, F.FINAL)
    _same_bits(after["p_out"][orig], c.x[idx], "retired position")
    assert np.array_equal(after["conv_out"][orig], ok.astype(np.uint8))
    _only_changed(before, after, dict(p_out=_at(after["p_out"], orig), conv_out=_at(after["p_out"], orig)))       # live and both queues stay


@pytest.mark.parametrize("i,M", list(enumerate(MS)))
def test_mid_final(i, M):
    _run_final(M, *_geom(i + 2), times=1 + i % 2)


def test_mid_final_grid_stride():
    _run_final(P_RAY, 32, "interleaved", 2, big=True)


# ------------------------------------------------------------------------------------------------ sr_refine_finish
def _finish_inputs(M, rig, mix, seed=1):
    n_s, n_d = 3 + 6 * rig.L_sdf, 3 + 6 * rig.L_def
    d = NS(x=fx.det_array((M, 3), seed * 10 + 1, 1.0, f32), v=fx.det_array((M, 3), seed * 10 + 2, 1.0, f32), frame=((np.arange(M) * 7) % rig.N).astype(np.int32),
           f=fx.det_array((M,), seed * 10 + 3, 2e-4, f32), t=np.concatenate([fx.det_array((M, 3), seed * 10 + 4, 1.0, f32), np.zeros((M, 1), f32)], 1),
           s=(10 ** (-6 + 5.5 * F._unit01((M,), seed * 10 + 5))).astype(f32), a0bar=fx.det_array((M, rig.ld_a0bar), seed * 10 + 6, 1.0, f32),
           a0dbar=fx.det_array((M, rig.ld_a0dbar), seed * 10 + 7, 0.3, f32),
           skipbar=None if rig.n_skip is None else fx.det_array((M, rig.ld_skipbar), seed * 10 + 8, 1.0, f32))
    d.conv = F.want_of(M, mix, seed)
    if M >= 16 and mix != "all":
        d.conv[:4] = False
        d.f[1], d.f[2] = 0.0, -0.0                                          # f == 0 with w2 s > 0: sign(0) = 0, the step follows the ray term alone
        d.a0bar[3], d.a0dbar[3], d.t[3], d.f[3] = 0.0, 0.0, 0.0, 1e-4       # every cotangent zero: |g|^2 = 0
        if d.skipbar is not None:
            d.skipbar[3] = 0.0
    return d


def _run_finish(M, phase, mix, L_sdf=6, L_def=6, E=128, n_skip=None, bar_pitch="exact", rows=True, pitch="exact", tile=1000):
    base_M = min(M, tile)
    idx = np.arange(M) % base_M
    P = M + 29
    orig = (P - 1 - np.arange(M)).astype(np.int32)
    runs = []
    for rep in range(2):
        rig = Rig(P, 2, 9, L_sdf, L_def, E, pitch, rows, True, bar_pitch, n_skip, ld_sdf=2)
        d = _finish_inputs(base_M, rig, mix)
        cur, nxt = phase & 1, (phase & 1) ^ 1
        rig.put_queue(cur, d.x[idx], d.v[idx], d.frame[idx], orig)
        rig.put("sdf_out", d.f[idx], col=0)
        for name in ("t", "s", "a0bar", "a0dbar"):
            rig.put(name, getattr(d, name)[idx])
        rig.put("conv", d.conv[idx].astype(np.uint8))
        if n_skip is not None:
            rig.put("skipbar", d.skipbar[idx])
        rig.put_live(phase, M)
        before, after = rig.launch("sr_refine_finish", phase)
        conv = d.conv[idx]
        n = int(after["live"][phase + 1])
        assert n == int((~conv).sum())
        runs.append(_canonical(after, nxt, n, orig[conv]))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    ref = F.finish(d.x, d.conv, d.f, d.t, d.s, d.a0bar, d.skipbar, n_skip or 0, d.a0dbar, L_sdf, rig.w_sdf, L_def, rig.w_def)
    q = F.queue_sorted(*_queue_of(after, nxt), n)
    kept = np.nonzero(~conv)[0]
    kept = kept[np.argsort(orig[kept], kind="stable")]
    want, tol = ref.x[idx][kept], ref.dx[idx][kept]
    fin = np.isfinite(want).all(1)
    assert (~fin).sum() == (0 if (base_M < 16 or mix == "all") else int((idx[kept] == 3).sum()))   # only the |g|^2 = 0 ray, as -loss / 0 gives
    assert not np.isfinite(q.x[~fin]).any()
    _within("finish", "x", q.x[fin], want[fin], tol[fin])
    _same_bits(q.v, d.v[idx][kept], "v")
    assert np.array_equal(q.frame, d.frame[idx][kept]) and np.array_equal(q.orig, orig[kept])
    _same_bits(after["p_out"][orig[conv]], d.x[idx][conv], "retired position")
    assert (after["conv_out"][orig[conv]] == 1).all()
    allowed = {k: _head(after[k], n) for k in (f"x{nxt}", f"v{nxt}", f"frame{nxt}", f"orig{nxt}")}
    allowed["live"] = _at(after["live"], [phase + 1])
    allowed["p_out"] = allowed["conv_out"] = _at(after["p_out"], orig[conv])
    if rows:
        allowed["a0"] = allowed["a0d"] = _head(after["a0"], n)
        r0, r0d = after["a0"][:n][q.perm], after["a0d"][:n][q.perm]
        _check_rows("finish", rig, r0[fin], r0d[fin], q.x[fin], q.frame[fin])                    # the rows of x[nxt][k], frame[nxt][k]
        assert not np.isfinite(r0[~fin][:, :3]).any() and not np.isfinite(r0d[~fin][:, :3]).any()
    _only_changed(before, after, allowed)
    gb = ref.dx[idx][kept][fin]
    print(f"finish M={M} {mix}: {int(conv.sum())} retired, {n} kept, median bound {np.median(gb) if gb.size else 0:.2e}")


@pytest.mark.parametrize("i,M", list(enumerate(MS)))
def test_finish(i, M):
    L_sdf, L_def = ((6, 6), (10, 6), (0, 10))[i % 3]
    n_skip = (None, 3 + 6 * L_sdf, 20)[(i // 3 + i) % 3]
    _run_finish(M, 1 + i % 2, "half", L_sdf, L_def, 128 if i % 2 else 0, n_skip, "pad" if i % 2 else "exact", rows=(i % 4 != 3), pitch="pad" if i % 3 == 0 else "exact")


@pytest.mark.parametrize("mix,n_skip", [("all", None), ("none", 39), ("none", 20), ("one", None), ("half", 20), ("half", 39)])
def test_finish_mixtures_and_skip(mix, n_skip):
    _run_finish(257, 2, mix, n_skip=n_skip, bar_pitch="pad")


def test_finish_grid_stride():
    _run_finish(P_ENQ, 1, "half", n_skip=39)


# ------------------------------------------------------------------------------------------------ csrc/tracer.hip
CAMD = np.array([0.125, 0.25, 2.5], f32)          # dyadic: y = c + 2 v is then exactly parallel to v in float32, every product exact


@functools.lru_cache(maxsize=None)
def _newton_case(seed=4):
    B = 1000
    y = R.interior_points(B, seed)
    f, v = F.draw_rays(y.astype(np.float64), F.want_of(B, "half", seed), seed * 10 + 2, special=True, cam=CAMD)
    v[8] = [0.25, -0.5, -1.0]
    y[8] = CAMD + 2 * v[8]
    f[8] = 1e-5
    jl = (np.eye(3, dtype=f32)[None] + fx.det_array((B, 3, 3), seed * 10 + 3, 0.5, f32)).astype(f32)
    return NS(B=B, y=y, f=f, v=v, jl=jl, gf=fx.det_array((B, 3), seed * 10 + 4, 1.0, f32), oj=fx.det_array((B, 3, 3), seed * 10 + 5, 0.3, f32),
              goff=fx.det_array((B, 3), seed * 10 + 6, 0.5, f32), p=fx.det_array((B, 3), seed * 10 + 7, 1.0, f32), off=fx.det_array((B, 3), seed * 10 + 8, 0.05, f32))


def _newton_common(a, bufs):
    a.dthreshold, a.athreshold, a.w1, a.w2 = float(F.DTHR), float(F.ATHR), float(F.W1), float(F.W2)
    bufs["cam"] = _dev(CAMD)
    a.cam = bufs["cam"].data_ptr()


def _call(name, a, on):
    from selfreconcode_amd import _lib
    with torch.cuda.device(0):
        _lib.call(name, ctypes.byref(a), _lib.stream_of(on))
    torch.cuda.synchronize()


def _guarded(t, M, what):
    """the guard rows of an output stayed the sentinel"""
    tail = t[M:].cpu().numpy()
    if tail.dtype == np.float32:
        assert (tail.view(np.int32) == SENT_BITS).all(), what
    else:
        assert (tail == 0xAB).all(), what


@pytest.mark.parametrize("M", [1, 255, 257, P_RAY])
@pytest.mark.parametrize("group,with_p", [(1, False), (1, True), (4, False), (4, True)])
def test_newton_update(M, group, with_p):
    from selfreconcode_amd import _lib
    c = _newton_case()
    idx = np.arange(M) % c.B
    ld_sdf, ld_off = (1, 3) if M == P_RAY else (2, 4)
    sdf4 = np.zeros((M, group, ld_sdf), f32)
    off4 = np.zeros((M, group, ld_off), f32)
    sdf4[:, 0, 0] = c.f[idx]
    off4[:, 0, :3] = c.off[idx]
    if group == 4:
        sdf4[:, 1:, 0] = c.gf[idx]
        off4[:, 1:, :3] = c.oj[idx].transpose(0, 2, 1)                     # tangent row 1 + c holds d off / d p_c
    b = dict(sdf4=_dev(sdf4), off4=_dev(off4), y=_dev(c.y[idx]), jl=_dev(c.jl[idx]), rays=_dev(c.v[idx]), p=_dev(c.p[idx]),
             p_out=_full((M + GUARD, 3), "f"), conv=_full((M + GUARD,), "b"))
    a = _lib.SrNewtonArgs()
    a.M, a.group, a.sdf4, a.ld_sdf, a.off4, a.ld_off = M, group, b["sdf4"].data_ptr(), ld_sdf, b["off4"].data_ptr(), ld_off
    a.y, a.jlbs, a.rays, a.p = b["y"].data_ptr(), b["jl"].data_ptr(), b["rays"].data_ptr(), b["p"].data_ptr()
    a.p_out, a.converged = (b["p_out"].data_ptr() if with_p else None), b["conv"].data_ptr()
    _newton_common(a, b)
    _call("sr_newton_update", a, b["y"])
    ref = F.newton_update(group, c.f, c.gf, c.oj, c.y, c.jl, c.v, c.p, cam=CAMD)
    assert np.array_equal(b["conv"][:M].cpu().numpy(), ref.conv[idx].astype(np.uint8))
    _guarded(b["conv"], M, "conv"); _guarded(b["p_out"], M if with_p else 0, "p_out")
    if with_p:
        got = b["p_out"][:M].cpu().numpy()
        still = ref.conv[idx] | (group == 1)
        _same_bits(got[still], c.p[idx][still], "converged rays are copied")
        _within(f"newton_update g{group}", "p_out", got[~still], ref.x[idx][~still], ref.dx[idx][~still])


@pytest.mark.parametrize("M", [1, 255, 257, P_RAY])
@pytest.mark.parametrize("ld_t", [0, 3, 4, 7])
def test_newton_prepare_and_apply(M, ld_t):
    """ld_t 0: the t_out == NULL form (convergence test only).  Otherwise prepare, then apply on prepare's own t / s / flags: the
    pair lands within the update bound of the float64 point, as group 4 of sr_newton_update does."""
    from selfreconcode_amd import _lib
    c = _newton_case()
    idx = np.arange(M) % c.B
    ld_sdf = 1 if M == P_RAY else 3
    sdf = np.zeros((M, ld_sdf), f32)
    sdf[:, 0] = c.f[idx]
    b = dict(sdf=_dev(sdf), y=_dev(c.y[idx]), jl=_dev(c.jl[idx]), rays=_dev(c.v[idx]), p=_dev(c.p[idx]), gf=_dev(c.gf[idx]), goff=_dev(c.goff[idx]),
             conv=_full((M + GUARD,), "b"), t=_full((M + GUARD, max(ld_t, 1)), "f"), s=_full((M + GUARD,), "f"), p_out=_full((M + GUARD, 3), "f"))
    a = _lib.SrNewton2Args()
    a.M, a.sdf, a.ld_sdf, a.y, a.jlbs, a.rays, a.converged = M, b["sdf"].data_ptr(), ld_sdf, b["y"].data_ptr(), b["jl"].data_ptr(), b["rays"].data_ptr(), b["conv"].data_ptr()
    if ld_t:
        a.t_out, a.ld_t, a.s_out = b["t"].data_ptr(), ld_t, b["s"].data_ptr()
    _newton_common(a, b)
    _call("sr_newton_prepare", a, b["y"])
    ref = F.newton_prepare(c.f, c.y, c.jl, c.v, cam=CAMD)
    conv = b["conv"][:M].cpu().numpy()
    assert np.array_equal(conv, ref.conv[idx].astype(np.uint8))
    _guarded(b["conv"], M, "conv"); _guarded(b["t"], M if ld_t else 0, "t"); _guarded(b["s"], M if ld_t else 0, "s"); _guarded(b["p_out"], 0, "p_out")
    if not ld_t:
        return
    t, s = b["t"][:M].cpu().numpy(), b["s"][:M].cpu().numpy()
    assert (t[:, 3:] == 0).all() and (s[idx == 8] == 0).all() and (t[idx == 8] == 0).all() and (s[idx == 5] == 0).all() and (t[idx == 5] == 0).all()
    _within("newton_prepare", "s", s, ref.s[idx], ref.ds[idx])
    _within("newton_prepare", "t", t[:, :3], ref.t[idx], ref.dt[idx])
    a.grad_f, a.grad_off, a.p, a.p_out = b["gf"].data_ptr(), b["goff"].data_ptr(), b["p"].data_ptr(), b["p_out"].data_ptr()
    _call("sr_newton_apply", a, b["y"])
    got = b["p_out"][:M].cpu().numpy()
    _guarded(b["p_out"], M, "p_out")
    still = ref.conv[idx]
    _same_bits(got[still], c.p[idx][still], "converged rays are copied")
    # apply alone, on the t and s it was given (tight: they are inputs) ...
    alone = F.newton_apply(conv.astype(bool), c.f[idx], t[:, :3], s, c.gf[idx], c.goff[idx], c.p[idx])
    _within("newton_apply", "p_out", got[~still], alone.x[~still], alone.dx[~still])
    # ... and the pair against the float64 point: t and s carry prepare's budgets into the update bound
    pair = F._update(c.p, c.f, c.gf, 0.0, ref.t, np.where(np.isfinite(ref.dt), ref.dt, np.inf), c.goff, 0.0, ref.s, ref.ds)
    _within("newton prepare+apply", "p_out", got[~still], pair.x[idx][~still], pair.dx[idx][~still])


# ------------------------------------------------------------------------------------------------ composed
def test_composed_launch_sequence_retires_every_ray_once():
    """init -> CHECK -> [STEP -> finish] x 2 -> FINAL at P = 1000 with sdf_out / def_out / cotangent buffers refilled per phase from a
    seeded function of the original index; the host reads the queue back after each launch and holds the launch to the reference
    on THAT queue.  Every ray's result lands at its original index exactly once."""
    P, times, N = 1000, 2, 9
    K = LP._K()
    tgt = R.make_case(P, N, "interleaved", seed=3)                           # ray o's LBS point (the kernel's q = x + offset) and frame
    A = R.transforms(tgt.poses, K).float()
    qt, bi = tgt.p.numpy(), tgt.bi.numpy()
    y = R.lbs_reference(tgt.p.double(), A, tgt.trans, tgt.bi, K).y.numpy()
    dy = F.Y_TOL["atol"] + F.Y_TOL["rtol"] * np.abs(y)
    rig = Rig(P, times, N, bars=True, n_skip=39, A=A, trans=tgt.trans)
    lbs = (A, tgt.trans, K)
    off0 = (np.round(fx.det_array((P, 3), 71, 1.0, np.float64) * 127) / 4096).astype(f32)
    rig.put("p0", (qt - off0).astype(f32)); rig.put("rays", np.zeros((P, 3), f32)); rig.put("batch_inds", bi.astype(np.int64))
    rig.launch("sr_refine_init")
    done = np.zeros(P, bool)

    def refill(phase, state):
        """this phase's f, offsets and rays for the rays in the queue, from their original index -> the queue as the host sees it"""
        cur, M = phase & 1, int(state["live"][phase])
        x, _, frame, orig = (a[:M] for a in _queue_of(state, cur))
        assert len(np.unique(orig)) == M and not done[orig].any() and np.array_equal(frame, bi[orig]) and np.abs(x).max() < 8
        f, v = F.draw_rays(y, F.want_of(P, "half", 100 + phase), 200 + phase, dy=dy)
        off = (qt[orig] - x).astype(f32)
        rig.put(f"v{cur}", v[orig]); rig.put("sdf_out", f[orig], col=0)
        for k in range(3):
            rig.put("def_out", off[:, k], col=k)
        return NS(x=x, v=v[orig], frame=frame, orig=orig, f=f[orig], off=off, M=M)

    def retire(before, after, orig, x, flag):
        assert (_bits(before["p_out"][orig]) == SENT_BITS).all() and (before["conv_out"][orig] == 0xAB).all()        # not written before
        _same_bits(after["p_out"][orig], x, "retired position")
        assert np.array_equal(after["conv_out"][orig], flag.astype(np.uint8))
        done[orig] = True

    def enqueued(after, phase, want_orig):
        n = int(after["live"][phase])
        q = F.queue_sorted(*_queue_of(after, phase & 1), n)
        assert np.array_equal(q.orig, np.sort(want_orig))
        _check_rows("composed", rig, after["a0"][:n][q.perm], after["a0d"][:n][q.perm], q.x, q.frame)
        return q

    q = refill(0, rig.snapshot())
    before, after = rig.launch("sr_refine_mid", 0, F.CHECK)
    ref = F.mid(F.CHECK, q, q.f, q.off, lbs)
    retire(before, after, ref.retired.orig, ref.retired.x, ref.retired.flag)
    enqueued(after, 1, q.orig[ref.kept])
    for phase in (1, 2):
        q = refill(phase, after)
        before, after = rig.launch("sr_refine_mid", phase, F.STEP)
        ref = F.mid(F.STEP, q, q.f, q.off, lbs)
        assert np.array_equal(after["conv"][:q.M], ref.conv.astype(np.uint8))
        _within("composed STEP", "t", after["t"][:q.M], ref.t, ref.dt); _within("composed STEP", "s", after["s"][:q.M], ref.s, ref.ds)
        bars = NS(a0bar=F.cotangent_rows(P, rig.ld_a0bar, 300 + phase)[q.orig], a0dbar=F.cotangent_rows(P, rig.ld_a0dbar, 310 + phase, 0.3)[q.orig],
                  skipbar=F.cotangent_rows(P, rig.ld_skipbar, 320 + phase)[q.orig])
        for k, vv in vars(bars).items():
            rig.put(k, vv)
        conv, t, s = after["conv"][:q.M].astype(bool), after["t"][:q.M], after["s"][:q.M]
        before, after = rig.launch("sr_refine_finish", phase)
        fin = F.finish(q.x, conv, q.f, t, s, bars.a0bar, bars.skipbar, 39, bars.a0dbar, rig.L_sdf, rig.w_sdf, rig.L_def, rig.w_def)
        retire(before, after, q.orig[conv], q.x[conv], np.ones(int(conv.sum()), bool))
        nq = enqueued(after, phase + 1, q.orig[~conv])
        kept = np.nonzero(~conv)[0]
        kept = kept[np.argsort(q.orig[kept], kind="stable")]
        _within("composed finish", "x", nq.x, fin.x[kept], fin.dx[kept])
    q = refill(times + 1, after)
    before, after = rig.launch("sr_refine_mid", times + 1, F.FINAL)
    ref = F.mid(F.FINAL, q, q.f, q.off, lbs)
    retire(before, after, ref.retired.orig, ref.retired.x, ref.retired.flag)
    assert done.all() and (_bits(after["p_out"][:P]) != SENT_BITS).all() and (after["conv_out"][:P] != 0xAB).all()
    live = after["live"][:times + 3].tolist()
    assert live[0] == P and all(a > b > 0 for a, b in zip(live, live[1:times + 2])) and live[times + 2] == 0
    assert 0.2 * P < after["conv_out"][:P].sum() < P


def test_ratios_were_recorded():
    """(last in the file) the table of profiles/refiner_kernels.md: the largest error / bound of every launch and quantity in this run"""
    for (launch, what), r in sorted(RATIOS.items()):
        print(f"max ratio {launch} | {what} | {r:.3f}")
        assert r <= 1.0
