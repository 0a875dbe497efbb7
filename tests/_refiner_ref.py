"""Float64 restatement of the refiner's per-ray launches (csrc/refiner.hip, the newton kernels of csrc/tracer.hip), their error budgets
and the seeded rays of tests/test_refiner_kernels_gpu.py.  tests/test_refiner_ref_cpu.py proves this file against float64 autograd.
Host only: numpy, and torch on the CPU for the LBS reference of tests/_lbs_ref.py.

Written from the contract in include/selfrecon_hip.h (sr_refine_args, sr_newton_args, sr_newton2_args) and the iteration it
replaces (utils/FindSurfacePs.py:114-163), with d = y - c and u = d x v:

    s = |u| / |d|                      e = ds/dy = (v x u^) / |d| - |u| d / |d|^3        (u^ = u / |u|, 0 when |u| = 0)
    flag = |f| < dthr  and  degrees(asin s) < athr                                      (float32 thresholds)
    t = J^T e                          g = w1 sign(f) grad f + w2 (t + J_off^T t)         (sign(0) = 0)
    p <- p - (w1 |f| + w2 s) g / |g|^2

Error budgets (eps = 2^-24; derived, not fitted to any device):
  * a perturbation delta of d moves u by at most |delta||v| and 1/|d| by |delta|/|d| relative, so s by at most
    (|delta|/|d|) (|v| + s) = (|delta|/|d|) kappa s with kappa = 1 + |d||v|/|u|.  In e the unit vector u^ turns by |delta||v|/|u|;
    summing the four first-order terms gives (|delta|/|d|) (kappa |v| + |v| + 3 s) / |d| <= 3 (|delta|/|d|) kappa |v| / |d| (s <= |v|,
    kappa >= 2).  Float32 rounding alone acts like |delta|/|d| = eps per operation; the margin 8 covers the dozen operations, FMA
    contraction and the ulps of sqrtf / asinf:   ds = kappa s (8 eps + rd),  de = kappa |v|/|d| (8 eps + 3 rd),
    rd = 0 for a y that is given, (|dy| + 4 eps |d|) / |d| for a y that comes from the LBS kernel with its own tolerance dy;
  * dt_c = sum_r dJ_rc |e_r| + |J_rc| de + 4 eps |J_rc e_r|;
  * pull-back of the positional encoding: (2L + 8) eps sum |terms|;
  * update: first-order propagation, see `_update`.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import fixtures as fx
import _lbs_ref as R
from test_lbs_paths_gpu import Y_TOL, J_TOL          # the LBS kernels' own tolerances: the budget of a y / J that comes from them

EPS = 2.0 ** -24
CHECK, STEP, FINAL = 0, 1, 2
CAM = np.array([0.1, 0.15, 2.4], np.float32)
DTHR, ATHR = np.float32(5e-5), np.float32(0.3)
W1, W2 = np.float32(3.05), np.float32(1.0)
BAND = 4.0                                           # no generated ray lies within BAND x its own angle budget of athr


def _f64(a):
    return np.asarray(a, np.float64)


def _norm(a):
    return np.sqrt((a * a).sum(-1))


# ------------------------------------------------------------------------------------------------ first-layer input rows
def embed_rows(x, frame, L, w, conds, E, ld):
    """[x | w[2k] sin(2^k x), w[2k+1] cos(2^k x) per band | conds[frame] | zeros up to ld] (column order of model/Embedder.py) ->
    (rows [P, ld] float64, tolerance [P, ld]).  2^k x is exact in float32, so the argument is formed from the float32 x."""
    x32 = np.asarray(x, np.float32).reshape(-1, 3)
    P = x32.shape[0]
    assert ld >= 3 + 6 * L + E
    rows, tol = np.zeros((P, ld)), np.zeros((P, ld))
    rows[:, :3] = x32
    w = _f64(w)
    for k in range(L):
        a = (x32 * np.float32(2.0 ** k)).astype(np.float64)
        rows[:, 3 + 6 * k:6 + 6 * k] = w[2 * k] * np.sin(a)
        rows[:, 6 + 6 * k:9 + 6 * k] = w[2 * k + 1] * np.cos(a)
        tol[:, 3 + 6 * k:6 + 6 * k] = 4 * EPS * abs(w[2 * k])
        tol[:, 6 + 6 * k:9 + 6 * k] = 4 * EPS * abs(w[2 * k + 1])
    if E:
        rows[:, 3 + 6 * L:3 + 6 * L + E] = _f64(conds)[np.asarray(frame, np.int64), :E]
    return rows, tol


# ------------------------------------------------------------------------------------------------ residual
def residual(f, y, v, cam, dthr=DTHR, athr=ATHR, dy=None):
    """s, e = ds/dy, the flag and the budgets ds, de, da (degrees) of one convergence test.  f [M] float32; y, v [M,3]; dy: the
    per-component tolerance of a y that a kernel computed ([M,3]), None for a y that is given."""
    f = np.asarray(f, np.float32)
    y, v, cam = _f64(y), _f64(v), _f64(cam)
    d = y - cam
    u = np.cross(d, v)
    un, dn, vn = _norm(u), _norm(d), _norm(v)
    s = un / dn
    with np.errstate(divide="ignore", invalid="ignore"):
        uh = np.where(un[:, None] > 0, u / un[:, None], 0.0)
        kappa = np.where(un > 0, 1.0 + dn * vn / un, np.inf)
    e = np.cross(v, uh) / dn[:, None] - (un / dn ** 3)[:, None] * d
    ang = np.degrees(np.arcsin(np.minimum(s, 1.0)))
    near = np.abs(f) < np.float32(dthr)                                   # float32 against float32: exact
    ok = near & (ang < np.float64(np.float32(athr)))
    rd = 0.0 if dy is None else (_norm(_f64(dy)) + 4 * EPS * dn) / dn
    ds = (s + vn) * (8 * EPS + rd)                                        # kappa s = s + |v|
    with np.errstate(invalid="ignore"):
        de = np.where(vn == 0, 0.0, kappa * vn / dn * (8 * EPS + 3 * rd))
    da = np.degrees(ds / np.sqrt(np.maximum(1.0 - s * s, 1e-300)))
    return SimpleNamespace(s=s, e=e, ok=ok, near=near, ang=ang, ds=ds, de=de, da=da, kappa=kappa, d=d)


def _jt(J, e):
    """t = J^T e and sum |J|^T |e| per component; J [M,3,3] rows = output coordinate."""
    return np.einsum("prc,pr->pc", J, e)


def cotangent(J, e, de, dJ=None):
    """t = J^T e [M,3] and its budget."""
    J, e = _f64(J), _f64(e)
    t = _jt(J, e)
    aJ = np.abs(J)
    with np.errstate(invalid="ignore"):
        dt = aJ.sum(1) * de[:, None] + 4 * EPS * _jt(aJ, np.abs(e))
    if dJ is not None:
        dt = dt + _jt(_f64(dJ), np.abs(e))
    return t, np.where(np.isnan(dt), np.inf, dt)


# ------------------------------------------------------------------------------------------------ sr_refine_mid
def mid(mode, q, sdf_out, def_out, lbs, cam=CAM, dthr=DTHR, athr=ATHR):
    """One sr_refine_mid launch on the live rows q = (x, v, frame, orig) with f = sdf_out [M] and the offsets def_out [M,3].
    lbs = (A [N,24,4,4], trans [N,3], K).  CHECK / FINAL: `retired` (orig, position, flag) and `kept` (row indices);
    STEP: conv, t [M,4] (4th column 0), s with their budgets."""
    A, trans, K = lbs
    x = _f64(q.x)
    pos = x + _f64(def_out)[:, :3]
    ref = R.lbs_reference(torch.from_numpy(pos), A, trans, torch.from_numpy(np.asarray(q.frame, np.int64)), K)
    y, J = ref.y.numpy(), ref.J.numpy()
    r = residual(sdf_out, y, q.v, cam, dthr, athr, dy=Y_TOL["atol"] + Y_TOL["rtol"] * np.abs(y))
    out = SimpleNamespace(y=y, J=J, r=r, ok=r.ok)
    if mode == STEP:
        t, dt = cotangent(J, r.e, r.de, J_TOL["atol"] + J_TOL["rtol"] * np.abs(J))
        out.conv, out.s, out.ds = r.ok, r.s, r.ds
        out.t, out.dt = np.concatenate([t, np.zeros((len(t), 1))], 1), np.concatenate([dt, np.zeros((len(t), 1))], 1)
        return out
    retire = r.ok | (mode == FINAL)
    out.retired = SimpleNamespace(orig=np.asarray(q.orig)[retire], x=np.asarray(q.x)[retire], flag=r.ok[retire])
    out.kept = np.nonzero(~retire)[0]
    return out


# ------------------------------------------------------------------------------------------------ sr_refine_finish
def pe_pullback(x, L, w, g0, g2=None, n2=0):
    """d/dx of <g, row(x)> for the cotangent row g = g0 (+ g2 on the first n2 columns) of a first-layer input row -> (value [M,3],
    sum of the absolute values of its terms [M,3])."""
    x32 = np.asarray(x, np.float32).reshape(-1, 3)
    w = _f64(w)
    n = 3 + 6 * L
    at, ab = _f64(g0)[:, :n].copy(), np.abs(_f64(g0)[:, :n])
    if g2 is not None and n2 > 0:
        m = min(n2, n)
        at[:, :m] += _f64(g2)[:, :m]
        ab[:, :m] += np.abs(_f64(g2)[:, :m])
    val, tot = at[:, :3].copy(), ab[:, :3].copy()
    for k in range(L):
        a = (x32 * np.float32(2.0 ** k)).astype(np.float64)
        fk = 2.0 ** k
        val += fk * (w[2 * k] * np.cos(a) * at[:, 3 + 6 * k:6 + 6 * k] - w[2 * k + 1] * np.sin(a) * at[:, 6 + 6 * k:9 + 6 * k])
        tot += fk * (abs(w[2 * k]) * np.abs(np.cos(a)) * ab[:, 3 + 6 * k:6 + 6 * k] + abs(w[2 * k + 1]) * np.abs(np.sin(a)) * ab[:, 6 + 6 * k:9 + 6 * k])
    return val, tot


def pe_bound(L, tot):
    return (2 * L + 8) * EPS * tot


def _update(x, f, gf, dgf, t, dt, goff, dgoff, s, ds, w1=W1, w2=W2):
    """p - (w1 |f| + w2 s) g / |g|^2 with g = w1 sign(f) gf + w2 (t + goff), and its first-order budget:
         dg_c   = w1 dgf_c + w2 (dt_c + dgoff_c) + 4 eps (|w1 gf_c| + |w2 t_c| + |w2 goff_c|)
         d|g|^2 = 2 sum |g_c| dg_c + 4 eps |g|^2
         dst    = |st| (d|g|^2 / |g|^2 + 4 eps) + w2 ds / |g|^2
         dx_c   = |st| dg_c + |g_c| dst + 2 eps (|x_c| + |st g_c|)
    (dt, ds: zero where t and s are inputs of the launch).  |g|^2 = 0 gives a non-finite point, as the reference's -loss / 0 does."""
    w1, w2 = float(np.float32(w1)), float(np.float32(w2))
    x, f, gf, t, goff, s = _f64(x), _f64(np.asarray(f, np.float32)), _f64(gf), _f64(t)[:, :3], _f64(goff), _f64(s)
    sg = np.sign(f)[:, None]
    g = w1 * sg * gf + w2 * (t + goff)
    dg = w1 * np.abs(sg) * dgf + w2 * (dt + dgoff) + 4 * EPS * (np.abs(w1 * sg * gf) + np.abs(w2 * t) + np.abs(w2 * goff))
    g2 = (g * g).sum(1)
    dg2 = 2 * (np.abs(g) * dg).sum(1) + 4 * EPS * g2
    Lr = w1 * np.abs(f) + w2 * s
    with np.errstate(divide="ignore", invalid="ignore"):
        st = -Lr / g2
        dst = np.abs(st) * (dg2 / g2 + 4 * EPS) + w2 * ds / g2
        xn = x + st[:, None] * g
        dx = np.abs(st)[:, None] * dg + np.abs(g) * dst[:, None] + 2 * EPS * (np.abs(x) + np.abs(st[:, None] * g))
    return SimpleNamespace(x=xn, dx=dx, g=g, g2=g2, st=st, loss=Lr)


def finish(x, conv, f, t, s, a0bar, skipbar, n_skip, a0dbar, L_sdf, w_sdf, L_def, w_def, w1=W1, w2=W2):
    """One sr_refine_finish launch on the live rows: converged rays are retired at their current position, the others step and
    stay.  -> keep [M] bool, x / dx [M,3] (new position of the kept rays and its budget), gf, goff."""
    gf, af = pe_pullback(x, L_sdf, w_sdf, a0bar, skipbar, n_skip)
    goff, aoff = pe_pullback(x, L_def, w_def, a0dbar)
    up = _update(x, f, gf, pe_bound(L_sdf, af), t, 0.0, goff, pe_bound(L_def, aoff), s, 0.0, w1, w2)
    up.keep, up.gf, up.goff = ~np.asarray(conv, bool), gf, goff
    return up


# ------------------------------------------------------------------------------------------------ csrc/tracer.hip forms
def newton_prepare(f, y, jlbs, v, cam=CAM, dthr=DTHR, athr=ATHR):
    """sr_newton_prepare: conv, t = J_lbs^T e, s for a given y (tight budgets)."""
    r = residual(f, y, v, cam, dthr, athr)
    t, dt = cotangent(jlbs, r.e, r.de)
    return SimpleNamespace(conv=r.ok, t=t, dt=dt, s=r.s, ds=r.ds, r=r)


def newton_apply(conv, f, t, s, grad_f, grad_off, p, w1=W1, w2=W2):
    """sr_newton_apply: converged rays are copied, the others step (t, s, the two gradients are inputs)."""
    up = _update(p, f, grad_f, 0.0, t, 0.0, grad_off, 0.0, s, 0.0, w1, w2)
    c = np.asarray(conv, bool)[:, None]
    up.x, up.dx = np.where(c, _f64(p), up.x), np.where(c, 0.0, up.dx)
    return up


def newton_update(group, f, grad_f, off_jac, y, jlbs, v, p, cam=CAM, dthr=DTHR, athr=ATHR, w1=W1, w2=W2):
    """sr_newton_update.  group 1: the test only (p_out, if asked for, is a copy).  group 4: d(p) = LBS(p + off(p)), so
    dd/dp = J_lbs J_q with J_q = I + d off / d p (off_jac[i][r][c] = d off_r / d p_c, the tangent rows), and the step of the
    unconverged rays uses g = w1 sign(f) grad f + w2 J_q^T J_lbs^T e."""
    pr = newton_prepare(f, y, jlbs, v, cam, dthr, athr)
    out = SimpleNamespace(conv=pr.conv, x=_f64(p).copy(), dx=np.zeros_like(_f64(p)), r=pr.r)
    if group == 4:
        goff, dgoff = cotangent(off_jac, pr.t, 0.0 * pr.ds)               # the part of J_q^T t beyond t itself
        dgoff = dgoff + _jt(np.abs(_f64(off_jac)), np.where(np.isfinite(pr.dt), pr.dt, 1e300))
        up = _update(p, f, grad_f, 0.0, pr.t, np.where(np.isfinite(pr.dt), pr.dt, np.inf), goff, dgoff, pr.s, pr.ds, w1, w2)
        c = pr.conv[:, None]
        out.x, out.dx, out.up = np.where(c, out.x, up.x), np.where(c, 0.0, up.dx), up
    return out


# ------------------------------------------------------------------------------------------------ queues are sets
def queue_sorted(x, v, frame, orig, n):
    """The first n rows of a queue ordered by original index (slot order across waves is free)."""
    orig = np.asarray(orig)[:n]
    assert len(np.unique(orig)) == n, "an original index occurs twice in the queue"
    o = np.argsort(orig, kind="stable")
    return SimpleNamespace(x=np.asarray(x)[:n][o], v=np.asarray(v)[:n][o], frame=np.asarray(frame)[:n][o], orig=orig[o], perm=o)


# ------------------------------------------------------------------------------------------------ seeded rays
def _unit01(shape, seed):
    return 0.5 + 0.5 * fx.det_array(shape, seed, 1.0, np.float64)


def _ray_at(dh, nh, theta):
    return (np.cos(theta)[:, None] * dh + np.sin(theta)[:, None] * nh).astype(np.float32)


def draw_rays(y, want, seed, dy=None, special=False, cam=CAM, dthr=DTHR, athr=ATHR):
    """f [M] float32 and unit rays v [M,3] float32 for surface points y (float64; the reference's), such that ray i passes the test
    exactly when want[i]: passing rays lie at 1e-6 rad .. 0.8 athr with |f| < 0.9 dthr; failing rays alternate between |f| in
    1.5 .. 100 dthr (angle anywhere in 1e-6 .. 0.3 rad) and an angle of 1.25 athr .. 0.3 rad (small |f|).  A ray whose angle lies
    within BAND x its budget of athr is redrawn.  special (M >= 16): rows 0..7 become f = +dthr, -dthr (not converged),
    nextafter(dthr, 0), +0, -0 (converged), v = 0 (|u| = 0), and the two rays at 4.25 x the band below / above athr."""
    y, want = _f64(y), np.asarray(want, bool)
    M = len(y)
    d = y - _f64(cam)
    dh = d / _norm(d)[:, None]
    rr = fx.det_array((M, 3), seed, 1.0, np.float64)
    nh = rr - (rr * dh).sum(1, keepdims=True) * dh
    nh /= _norm(nh)[:, None]
    arad = np.radians(float(athr))
    coin = np.arange(M) % 2 == 0
    lo = np.where(want | coin, 1e-6, 1.25 * arad)
    hi = np.where(want, 0.8 * arad, 0.3)
    small = want | ~coin
    uf = _unit01((M,), seed + 1)
    sgn = np.where(fx.det_array((M,), seed + 2, 1.0, np.float64) < 0, -1.0, 1.0)
    f = (sgn * float(dthr) * np.where(small, 0.9 * uf, 1.5 + 98.5 * uf)).astype(np.float32)
    theta = lo * (hi / lo) ** _unit01((M,), seed + 3)
    v = _ray_at(dh, nh, theta)
    for it in range(1, 20):
        r = residual(f, y, v, cam, dthr, athr, dy)
        bad = np.abs(r.ang - float(athr)) < BAND * r.da
        if not bad.any():
            break
        theta = np.where(bad, lo * (hi / lo) ** _unit01((M,), seed + 3 + 31 * it), theta)
        v = _ray_at(dh, nh, theta)
    else:
        raise AssertionError("could not move every ray out of the band")
    if special and M >= 16:
        th = theta.copy()
        th[:5] = 0.25 * arad
        f[:5] = [dthr, -dthr, np.nextafter(np.float32(dthr), np.float32(0)), 0.0, -0.0]
        f[6:8] = np.float32(0.5) * dthr
        da = residual(f[6:8], y[6:8], _ray_at(dh[6:8], nh[6:8], np.full(2, arad)), cam, dthr, athr, None if dy is None else dy[6:8]).da
        th[6:8] = np.radians(float(athr) + np.array([-1.0, 1.0]) * (BAND + 0.25) * da)
        v[:8] = _ray_at(dh[:8], nh[:8], th[:8])
        v[5] = 0.0
    r = residual(f, y, v, cam, dthr, athr, dy)
    assert not (np.abs(r.ang - float(athr)) < BAND * r.da).any()
    return f, v


MIXES = ("all", "none", "one", "half")


def want_of(M, mix, seed):
    if mix == "all":
        return np.ones(M, bool)
    w = np.zeros(M, bool)
    if mix == "one":
        w[(7 * seed + M // 2) % M] = True
    elif mix == "half":
        w = fx.det_array((M,), seed + 5, 1.0, np.float64) < 0
    return w


def make_mid_case(M, N, order, mix, K, seed=1, jac=False, f_scale=1.0):
    """Rays for one sr_refine_mid launch.  The points the LBS sees, q = x + offset, are tests/_lbs_ref's (interior, outside the
    box and -- value-only launches -- on the lattice), so that the LBS part stays within Y_TOL / J_TOL by that file's construction;
    offsets are multiples of 2^-12 below 1/32 and x = q - offset is kept only where x + offset == q exactly (else offset 0), so the
    float32 sum the kernel forms is the reference's q."""
    c = R.make_case(M, N, order, seed=seed, lattice=not jac)
    q = c.p.numpy()
    off = (np.round(fx.det_array((M, 3), seed * 10 + 1, 1.0, np.float64) * 127) / 4096).astype(np.float32)
    x = (q - off).astype(np.float32)
    exact = (x.astype(np.float64) + off.astype(np.float64) == q.astype(np.float64)) & ((x + off).astype(np.float32) == q)
    off, x = np.where(exact, off, np.float32(0)), np.where(exact, x, q)
    assert (M < 64 or exact.mean() > 0.5) and ((x + off) == q).all()
    A = R.transforms(c.poses, K).float()
    frame = c.bi.numpy().astype(np.int32)
    y = R.lbs_reference(torch.from_numpy(q.astype(np.float64)), A, c.trans, c.bi, K).y.numpy()
    f, v = draw_rays(y, want_of(M, mix, seed), seed * 10 + 2, dy=Y_TOL["atol"] + Y_TOL["rtol"] * np.abs(y), special=(mix == "half"))
    return SimpleNamespace(M=M, N=N, x=x, v=v, frame=frame, f=f, off=off, A=A, trans=c.trans, lbs=(A, c.trans, K), cls=c.cls.numpy())


def cotangent_rows(M, ld, seed, scale=1.0):
    return fx.det_array((M, ld), seed, scale, np.float32)
