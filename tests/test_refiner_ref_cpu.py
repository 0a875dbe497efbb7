"""tests/_refiner_ref.py proved on the host: its residual, cotangent and update against float64 autograd of the reference's own
formulation (loss = w1 |f| + w2 |d x v| / |d|, utils/FindSurfacePs.py:135-151), its embedding against the oracle's Embedder, its
pull-back against autograd of the embedding, its budgets against a numpy float32 evaluation of the same expressions (the bounds
can be met before a GPU sees them; the ratios printed here stand beside the measured ones in profiles/refiner_kernels.md), its
generator against the band around athr -- and the argument refusals of the refiner entry points, which are plain host code that
returns before any launch.  Nothing here reaches a launch."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import torch_oracle as orc
import _lbs_ref as R
import _refiner_ref as F

EPS = F.EPS
f32 = np.float32


def _toy(seed, M):
    """Toy differentiable f(p), offset(p) and deformer d = B sin(C q) + q, q = p + offset(p), in torch float64."""
    g = lambda shape, k, s: torch.from_numpy(fx.det_array(shape, seed * 10 + k, s, np.float64))
    Wf, Co, Cd, Bd = g((3,), 1, 1.0), g((3, 3), 2, 1.5), g((3, 3), 3, 1.0), g((3, 3), 4, 0.3)
    sdf = lambda p: torch.sin(p @ Wf) * 2e-4 + (p * p).sum(1) * 1e-4 - 5e-5
    off = lambda p: 0.05 * torch.sin(p @ Co.t())
    lbs = lambda q: torch.sin(q @ Cd.t()) @ Bd.t() + q
    p = g((M, 3), 5, 0.6)
    return sdf, off, lbs, p


def _jac(fn, p):
    p = p.clone().requires_grad_(True)
    return orc.compute_jacobian(p, fn(p), False, False).numpy()


def test_residual_cotangent_and_update_equal_autograd_of_the_reference_formulation():
    M = 64
    sdf, off, lbs, p = _toy(3, M)
    cam = torch.from_numpy(F.CAM.astype(np.float64))
    with torch.no_grad():
        y0 = lbs(p + off(p))
    dh = torch.nn.functional.normalize(y0 - cam, dim=1)
    theta = torch.from_numpy(10 ** (-6 + 5.4 * (0.5 + 0.5 * fx.det_array((M,), 77, 1.0, np.float64))))
    n = torch.nn.functional.normalize(torch.linalg.cross(dh, torch.from_numpy(fx.det_array((M, 3), 78, 1.0, np.float64)), dim=1), dim=1)
    v = torch.cos(theta)[:, None] * dh + torch.sin(theta)[:, None] * n
    w1, w2 = float(F.W1), float(F.W2)
    # the reference: FindSurfacePs.py:135-151
    cur = p.clone().requires_grad_(True)
    loss1 = sdf(cur).abs()
    direct = lbs(cur + off(cur)) - cam
    loss2 = torch.linalg.cross(direct, v, dim=1).norm(dim=1) / direct.norm(dim=1)
    loss = w1 * loss1 + w2 * loss2
    grad = torch.autograd.grad(loss.sum(), cur)[0]
    new = (cur + (-loss / (grad * grad).sum(1)).view(-1, 1) * grad).detach().numpy()
    # e = ds/dy by autograd
    yy = y0.clone().requires_grad_(True)
    dd = yy - cam
    ss = torch.linalg.cross(dd, v, dim=1).norm(dim=1) / dd.norm(dim=1)
    e_auto = torch.autograd.grad(ss.sum(), yy)[0].numpy()
    # the restatement
    with torch.no_grad():
        q = p + off(p)
        f = sdf(p).numpy()
    jl, jo = _jac(lbs, q), _jac(off, p)
    pg = p.clone().requires_grad_(True)
    gf = torch.autograd.grad(sdf(pg).sum(), pg)[0].numpy()
    r = F.residual(f.astype(f32), y0.numpy(), v.numpy(), F.CAM, dy=None)
    np.testing.assert_allclose(r.s, ss.detach().numpy(), rtol=1e-9, atol=0)           # |u| ~ 1e-6 |d|: the cross product cancels ten digits
    np.testing.assert_allclose(r.e, e_auto, rtol=1e-7, atol=1e-12)          # |u| ~ 1e-6 |d|: autograd's own division loses digits
    t, _ = F.cotangent(jl, r.e, r.de)
    goff, _ = F.cotangent(jo, t, 0 * r.de)
    f64 = f.astype(f32).astype(np.float64)                                  # the kernels see f in float32; sign and |f| follow it
    up = F._update(p.numpy(), f64, gf, 0.0, t, 0.0, goff, 0.0, r.s, 0.0)
    np.testing.assert_allclose(up.g, grad.numpy(), rtol=1e-7, atol=1e-12)     # f's float32 rounding does not change its sign
    lr = w1 * np.abs(f) + w2 * r.s
    np.testing.assert_allclose(p.numpy() - (lr / (up.g * up.g).sum(1))[:, None] * up.g, new, rtol=1e-7, atol=1e-10)
    # ... and through newton_update(group 4), whose step is the same formula on (f, grad f, tangent rows, y, J_lbs)
    nu = F.newton_update(4, f64, gf, jo, y0.numpy(), jl, v.numpy(), p.numpy(), dthr=0.0)      # dthr 0: nothing converges
    assert not nu.conv.any()
    np.testing.assert_allclose(nu.x, new, rtol=0, atol=1e-9 + 1e-6 * np.abs(new - p.numpy()).max())
    # J instead of J^T would not pass
    assert np.abs(np.einsum("prc,pc->pr", jl, r.e) - t).max() > 1e-3 * np.abs(t).max()


def test_degenerate_rays():
    """|u| = 0 (v parallel to y - c, v = 0): s = 0 and the u^ term of e vanishes; sign(0) = 0; |g|^2 = 0 is non-finite."""
    y = np.array([[0.5, 0.25, 0.125], [0.5, 0.25, 0.125]])
    cam = np.zeros(3, f32)
    v = np.array([[1.0, 0.5, 0.25], [0.0, 0.0, 0.0]])
    r = F.residual(np.zeros(2, f32), y, v, cam)
    assert (r.s == 0).all() and (r.e == 0).all() and r.ok.all() and r.de[1] == 0 and np.isinf(r.de[0])
    z = np.zeros((1, 3))
    up = F._update(np.ones((1, 3)), np.zeros(1, f32), np.ones((1, 3)), 0.0, 0.5 * np.ones((1, 3)), 0.0, z, 0.0, np.array([0.25]), 0.0, 3.0, 2.0)
    np.testing.assert_allclose(up.g, 1.0)                                   # sign(0) = 0: only w2 t is left
    np.testing.assert_allclose(up.x, 1.0 - 0.5 / 3.0)
    up = F._update(np.ones((1, 3)), np.ones(1, f32), z, 0.0, z, 0.0, z, 0.0, np.array([0.25]), 0.0)
    assert not np.isfinite(up.x).any()


@pytest.mark.parametrize("L,E,pad", [(0, 0, 0), (6, 0, 1), (6, 128, 0), (10, 128, 1), (0, 128, 3)])
def test_embed_rows_equal_the_oracle_embedder(L, E, pad):
    P, N = 37, 5
    x = fx.det_array((P, 3), 11, 1.2, f32)
    frame = np.arange(P) % N
    w = np.asarray(orc.resolve_pe_weights(L, 0.62), np.float64) if L else np.zeros(0)
    conds = fx.det_array((N, max(E, 1)), 12, 0.1, f32)
    ld = 3 + 6 * L + E + pad
    rows, tol = F.embed_rows(x, frame, L, w, conds, E, ld)
    want = orc.pe_embed(torch.from_numpy(x).double(), L, list(w)).numpy()
    np.testing.assert_allclose(rows[:, :3 + 6 * L], want, rtol=0, atol=1e-15)
    assert np.array_equal(rows[:, 3 + 6 * L:3 + 6 * L + E], conds[frame, :E].astype(np.float64)) and (rows[:, 3 + 6 * L + E:] == 0).all()
    assert (tol[:, :3] == 0).all() and (tol[:, 3 + 6 * L:] == 0).all()
    got = _embed_f32(x, L, w.astype(f32))
    ratio = np.abs(got - rows[:, :3 + 6 * L])[:, 3:] / np.maximum(tol[:, 3:3 + 6 * L], 1e-300) if L else np.zeros(1)
    print(f"embed L={L}: numpy float32 error / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("L,n2", [(0, 0), (6, 39), (6, 20), (10, 3), (10, 63)])
def test_pe_pullback_equals_autograd_of_the_embedding(L, n2):
    P = 41
    x = fx.det_array((P, 3), 21, 1.2, f32)
    w = np.asarray(orc.resolve_pe_weights(L, 0.7), np.float64) if L else np.zeros(0)
    n = 3 + 6 * L
    g0, g2 = fx.det_array((P, n + 5), 22, 1.0, f32), fx.det_array((P, max(n2, 1) + 2), 23, 1.0, f32)
    val, tot = F.pe_pullback(x, L, w, g0, g2 if n2 else None, n2)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    cot = torch.from_numpy(g0[:, :n]).double().clone()
    m = min(n2, n)
    cot[:, :m] += torch.from_numpy(g2[:, :m]).double()
    want = torch.autograd.grad((orc.pe_embed(xt, L, list(w)) * cot).sum(), xt)[0].numpy()
    np.testing.assert_allclose(val, want, rtol=1e-12, atol=1e-12)
    assert (tot >= np.abs(val) - 1e-12).all()
    got = _pullback_f32(x, L, w.astype(f32), g0, g2 if n2 else None, n2)
    ratio = np.abs(got - val) / F.pe_bound(L, tot)
    print(f"pull-back L={L} n2={n2}: numpy float32 error / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0


# ------------------------------------------------------------------------------------------------ float32 evaluations (numpy, no FMA)
def _embed_f32(x, L, w):
    out = [x]
    for k in range(L):
        a = x * f32(2.0 ** k)
        out += [w[2 * k] * np.sin(a), w[2 * k + 1] * np.cos(a)]
    return np.concatenate(out, 1).astype(np.float64)


def _pullback_f32(x, L, w, g0, g2, n2):
    n = 3 + 6 * L
    at = g0[:, :n].copy()
    if g2 is not None:
        at[:, :min(n2, n)] += g2[:, :min(n2, n)]
    acc = at[:, :3].copy()
    for k in range(L):
        a, fk = x * f32(2.0 ** k), f32(2.0 ** k)
        acc = acc + fk * (w[2 * k] * np.cos(a) * at[:, 3 + 6 * k:6 + 6 * k] - w[2 * k + 1] * np.sin(a) * at[:, 6 + 6 * k:9 + 6 * k])
    assert acc.dtype == f32
    return acc.astype(np.float64)


def _residual_f32(y, v, cam):
    d = y - cam
    u = np.stack([d[:, 1] * v[:, 2] - d[:, 2] * v[:, 1], d[:, 2] * v[:, 0] - d[:, 0] * v[:, 2], d[:, 0] * v[:, 1] - d[:, 1] * v[:, 0]], 1)
    un, dn = np.sqrt((u * u).sum(1, dtype=f32)), np.sqrt((d * d).sum(1, dtype=f32))
    s = un / dn
    with np.errstate(divide="ignore"):
        iu = np.where(un > 0, f32(1) / un, f32(0))
    h = u * iu[:, None]
    c = np.stack([v[:, 1] * h[:, 2] - v[:, 2] * h[:, 1], v[:, 2] * h[:, 0] - v[:, 0] * h[:, 2], v[:, 0] * h[:, 1] - v[:, 1] * h[:, 0]], 1)
    e = c / dn[:, None] - (un[:, None] * d) / (dn * dn * dn)[:, None]
    ang = np.arcsin(s) * f32(180.0) / f32(np.pi)
    assert s.dtype == f32 and e.dtype == f32 and ang.dtype == f32
    return s, e, ang


def _exact_y_rays(M, seed, mix="half"):
    y = R.interior_points(M, seed)
    f, v = F.draw_rays(y.astype(np.float64), F.want_of(M, mix, seed), seed * 10 + 2, special=(mix == "half"))
    return y, f, v


def test_float32_residual_and_cotangent_stay_within_the_budgets():
    M = 20000
    y, f, v = _exact_y_rays(M, 3)
    r = F.residual(f, y, v, F.CAM)
    assert 0.2 < r.ok.mean() < 0.8 and r.s[r.s > 0].min() < 3e-6 and r.s.max() > 0.25            # the kappa scaling is exercised
    s, e, ang = _residual_f32(y, v, F.CAM)
    rs = np.abs(s - r.s) / np.where(r.ds > 0, r.ds, 1.0)                                       # (ds = 0 only for v = 0, where s = 0 exactly)
    with np.errstate(invalid="ignore", divide="ignore"):
        re = np.nan_to_num(np.abs(e - r.e).max(1) / r.de, nan=0.0)
    print(f"residual: numpy float32 error / bound: s {rs.max():.3f}, e {re.max():.3f}")
    assert rs.max() <= 1.0 and re.max() <= 1.0
    assert np.array_equal((np.abs(f) < F.DTHR) & (ang < F.ATHR), r.ok)                          # no flag flips outside the band
    assert (s[5] == 0) and (e[5] == 0).all()
    J = np.eye(3, dtype=f32)[None] + fx.det_array((M, 3, 3), 9, 0.5, f32)
    t, dt = F.cotangent(J, r.e, r.de)
    t32 = np.stack([J[:, 0, c] * e[:, 0] + J[:, 1, c] * e[:, 1] + J[:, 2, c] * e[:, 2] for c in range(3)], 1)
    rt = np.abs(t32 - t) / np.where(dt > 0, dt, 1.0)
    print(f"cotangent: numpy float32 error / bound: {rt.max():.3f}")
    assert rt.max() <= 1.0


@pytest.mark.parametrize("L", [0, 6, 10])
def test_float32_update_stays_within_the_budget(L):
    M, E = 4000, 7
    x = fx.det_array((M, 3), 31, 1.0, f32)
    w = np.asarray(orc.resolve_pe_weights(L, 0.62), f32) if L else np.zeros(0, f32)
    n = 3 + 6 * L
    a0bar, skip, a0dbar = fx.det_array((M, n + 1), 32, 1.0, f32), fx.det_array((M, n), 33, 1.0, f32), fx.det_array((M, n + E), 34, 0.3, f32)
    f = fx.det_array((M,), 35, 2e-4, f32)
    f[:3] = [0.0, -0.0, 5e-5]
    t = np.concatenate([fx.det_array((M, 3), 36, 1.0, f32), np.zeros((M, 1), f32)], 1)
    s = (10 ** (-6 + 5.5 * F._unit01((M,), 37))).astype(f32)
    conv = np.zeros(M, bool)
    up = F.finish(x, conv, f, t, s, a0bar, skip, n, a0dbar, L, w, L, w)
    gf, goff = _pullback_f32(x, L, w, a0bar, skip, n).astype(f32), _pullback_f32(x, L, w, a0dbar, None, 0).astype(f32)
    sg = np.sign(f)[:, None]
    g = F.W1 * sg * gf + F.W2 * (t[:, :3] + goff)
    Lr = F.W1 * np.abs(f) + F.W2 * s
    st = -Lr / (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    xn = x + st[:, None] * g
    assert xn.dtype == f32
    ratio = np.abs(xn - up.x) / up.dx
    print(f"update L={L}: numpy float32 error / bound = {ratio.max():.3f}, median bound {np.median(up.dx):.2e}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("mix", F.MIXES)
def test_generator_leaves_no_ray_in_the_band_and_plants_the_edges(mix):
    M = 1000
    y, f, v = _exact_y_rays(M, 5, mix)
    r = F.residual(f, y, v, F.CAM)
    assert (np.abs(r.ang - float(F.ATHR)) >= F.BAND * r.da).all()
    want = F.want_of(M, mix, 5)
    if mix != "half":
        assert np.array_equal(r.ok, want)
        return
    assert list(r.ok[:8]) == [False, False, True, True, True, True, True, False]
    assert f[0] == F.DTHR and f[1] == -F.DTHR and 0 < f[2] < F.DTHR and f[3] == 0 and f[4] == 0 and np.signbit(f[4]) and (v[5] == 0).all()
    gap = np.abs(r.ang[6:8] - float(F.ATHR)) / r.da[6:8]
    assert (gap >= F.BAND).all() and (gap < F.BAND + 0.5).all() and r.ang[6] < float(F.ATHR) < r.ang[7]
    assert np.array_equal(r.ok[8:], want[8:])


def test_mid_case_generator_keeps_the_lbs_points_and_the_band():
    K = R.constants()
    c = F.make_mid_case(257, 9, "interleaved", "half", K, seed=2, jac=True)
    assert ((c.x + c.off).astype(f32) == R.make_case(257, 9, "interleaved", seed=2).p.numpy()).all() and (c.off != 0).mean() > 0.5
    q = F.SimpleNamespace(x=c.x, v=c.v, frame=c.frame, orig=np.arange(c.M))
    m = F.mid(F.STEP, q, c.f, c.off, c.lbs)
    assert (np.abs(m.r.ang - float(F.ATHR)) >= F.BAND * m.r.da).all()
    assert 0.2 < m.conv.mean() < 0.8 and (m.t[:, 3] == 0).all() and np.isfinite(m.dt[np.arange(c.M) != 5]).all()
    assert m.r.s[m.r.s > 0].min() < 1e-5 and m.r.s.max() > 0.2
    chk = F.mid(F.CHECK, q, c.f, c.off, c.lbs)
    assert len(chk.kept) + len(chk.retired.orig) == c.M and np.array_equal(chk.retired.x, c.x[m.conv]) and chk.retired.flag.all()
    fin = F.mid(F.FINAL, q, c.f, c.off, c.lbs)
    assert len(fin.kept) == 0 and np.array_equal(fin.retired.flag, m.conv)


# ------------------------------------------------------------------------------------------------ refusals (no launch)
EINVAL = -1
FAKE = 0x1000        # stands for "some pointer": every argument set below is refused before anything would look at it


def _refine_args(P=8, times=2):
    from selfreconcode_amd import _lib
    a = _lib.SrRefineArgs()
    a.P, a.times, a.nframes, a.L_sdf, a.L_def, a.E = P, times, 1, 6, 6, 128
    for name, typ in a._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, FAKE)
    for i in range(2):
        a.x[i] = a.v[i] = a.frame[i] = a.orig[i] = FAKE
    a.ld_a0 = a.ld_a0bar = a.ld_skipbar = a.n_skip = 39
    a.ld_a0d, a.ld_a0dbar, a.ld_conds, a.ld_sdf, a.ld_def = 167, 167, 128, 1, 3
    a.D, a.H, a.W = 2, 2, 2
    return a


def _rc(name, a, *more):
    from selfreconcode_amd import _lib
    return _lib.raw(name)(None if a is None else ctypes.byref(a), *more, None)


ENTRY = [("sr_refine_init", ()), ("sr_refine_embed", (0,)), ("sr_refine_mid", (0, 0)), ("sr_refine_finish", (1,))]


@pytest.mark.parametrize("name,more", ENTRY)
def test_refiner_entry_points_refuse_bad_common_arguments(name, more):
    assert _rc(name, None, *more) == EINVAL
    for field, bad in (("P", -1), ("times", -1), ("L_sdf", 17), ("L_def", 17), ("L_sdf", -1), ("E", -1), ("nframes", 0)):
        a = _refine_args()
        setattr(a, field, bad)
        assert _rc(name, a, *more) == EINVAL, (name, field)
    for field in ("live", "p_out", "conv_out", "cam", "A", "trans", "vol"):
        a = _refine_args()
        setattr(a, field, None)
        assert _rc(name, a, *more) == EINVAL, (name, field)
    a = _refine_args()
    a.orig[1] = None
    assert _rc(name, a, *more) == EINVAL
    a = _refine_args()
    a.ld_a0 = 3 + 6 * 6 - 1
    assert _rc(name, a, *more) == EINVAL
    a = _refine_args()
    a.ld_a0d = 3 + 6 * 6 + 128 - 1
    assert _rc(name, a, *more) == EINVAL


def test_refine_init_refuses_a_null_live_whatever_the_ray_count():
    for P in (0, 1, 8):
        a = _refine_args(P=P)
        a.live = None
        assert _rc("sr_refine_init", a) == EINVAL, P


def test_refine_entry_points_refuse_their_own_bad_arguments():
    def bad(name, more, **kw):
        a = _refine_args()
        for k, v in kw.items():
            setattr(a, k, v)
        return _rc(name, a, *more) == EINVAL
    for k in ("p0", "rays", "batch_inds", "unit", "a0", "a0d", "w_sdf", "w_def", "conds"):
        assert bad("sr_refine_init", (), **{k: None}), k
    for ph in (-1, 4):                                                       # times = 2: phases 0 .. 3
        assert bad("sr_refine_embed", (ph,)) and bad("sr_refine_mid", (ph, 0)) and bad("sr_refine_mid", (ph, 2))
    for ph in (0, 3, -1):                                                    # update phases are 1 .. times
        assert bad("sr_refine_finish", (ph,))
    for mode in (-1, 3):
        assert bad("sr_refine_mid", (0, mode))
    for k in ("a0", "a0d", "w_sdf", "conds"):
        assert bad("sr_refine_embed", (0,), **{k: None}), k
    for k in ("sdf_out", "def_out"):
        assert bad("sr_refine_mid", (0, 0), **{k: None}) and bad("sr_refine_mid", (1, 1), **{k: None})
    for k in ("conv", "t", "s"):
        assert bad("sr_refine_mid", (1, 1), **{k: None}), k
    for k in ("a0", "a0d"):                                                  # one of the pair without the other
        assert bad("sr_refine_mid", (0, 0), **{k: None}) and bad("sr_refine_finish", (1,), **{k: None})
    for k in ("conv", "t", "s", "a0bar", "a0dbar", "sdf_out", "w_sdf", "w_def"):
        assert bad("sr_refine_finish", (1,), **{k: None}), k
    assert bad("sr_refine_finish", (1,), ld_a0bar=38) and bad("sr_refine_finish", (1,), ld_a0dbar=38)
    assert bad("sr_refine_finish", (1,), n_skip=40, ld_skipbar=39)


def _newton_rc(name, cls, **kw):
    from selfreconcode_amd import _lib
    a = getattr(_lib, cls)()
    for fname, typ in a._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, fname, FAKE)
    a.M, a.ld_sdf = 8, 1
    if cls == "SrNewtonArgs":
        a.group, a.ld_off = 4, 4
    else:
        a.ld_t = 4
    for k, v in kw.items():
        setattr(a, k, v)
    return _lib.raw(name)(ctypes.byref(a), None)


def test_tracer_entry_points_refuse_bad_arguments():
    from selfreconcode_amd import _lib
    for name in ("sr_newton_update", "sr_newton_prepare", "sr_newton_apply"):
        assert _lib.raw(name)(None, None) == EINVAL
    for g in (0, 2, 3, 5, -1):
        assert _newton_rc("sr_newton_update", "SrNewtonArgs", group=g) == EINVAL
    assert _newton_rc("sr_newton_update", "SrNewtonArgs", M=-1) == EINVAL
    for k in ("sdf4", "y", "rays", "cam", "converged", "p", "off4", "jlbs"):
        assert _newton_rc("sr_newton_update", "SrNewtonArgs", **{k: None}) == EINVAL, k
    assert _newton_rc("sr_newton_prepare", "SrNewton2Args", M=-1) == EINVAL and _newton_rc("sr_newton_apply", "SrNewton2Args", M=-1) == EINVAL
    for k in ("sdf", "y", "rays", "cam", "converged", "jlbs", "s_out"):
        assert _newton_rc("sr_newton_prepare", "SrNewton2Args", **{k: None}) == EINVAL, k
    for ld in (2, 0, -1):
        assert _newton_rc("sr_newton_prepare", "SrNewton2Args", ld_t=ld) == EINVAL
    for k in ("sdf", "converged", "t_out", "s_out", "grad_f", "grad_off", "p", "p_out"):
        assert _newton_rc("sr_newton_apply", "SrNewton2Args", **{k: None}) == EINVAL, k
