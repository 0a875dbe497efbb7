"""Float64 references, a float32 twin and the error budgets of the per-row 3x3 kernels of the optimisation step (sr_svd3x3,
sr_svd3x3_bwd, sr_def_regu_loss_*, the inv3 users) and of the loss reductions around them (csrc/step_ops.hip::reduce_rows).
Plain numpy and CPU torch; nothing here touches a GPU.  tests/test_step3x3_ref_cpu.py calibrates the constants below against
float64 with the twin, tests/test_step3x3_gpu.py holds the kernels to them.

The contract under test (include/selfrecon_hip.h, header of csrc/small_ops.hip): A = U diag(S) V^T from cyclic Jacobi on
A^T A in float32 -- pairs (0,1), (0,2), (1,2), 6 sweeps -- S descending, u_k = A v_k / s_k.  Working on A^T A squares the
condition number: an eigenvalue s_k^2 carries an absolute error of about eps s_max^2, so s_k carries eps s_max^2 / s_k, a null
singular value comes back as about sqrt(eps) s_max, u_k loses orthogonality like eps cond^2, and the gradient of the
deformation regulariser is accurate to eps cond^2.  These are design properties; the budgets below state them per row.
"""
import numpy as np
import torch

EPS = float(np.finfo(np.float32).eps)
SQRT_EPS = float(np.sqrt(EPS))
DET_THRESHOLD = 1e-4                     # inv3's singularity rule: |det| < 1e-4 -> zeros, ok = False

# Budget constants: 4 x the worst ratio of the float32 twin (or the twin-derived gradient) against float64 over all families,
# rounded up to a power of two (the 4 allows for fma contraction and the device's sqrt / division rounding, which numpy does
# not have).  tests/test_step3x3_ref_cpu.py::test_constants_cover_the_twin asserts that each is at least the twin's worst ratio;
# profiles/step_tails_accuracy.md records the ratios.
C_S = 8.0        # |s_k - s64_k|                / (eps s_max^2 / max(s64_k, sqrt(eps) s_max))
C_V = 32.0       # |V^T V - I|                  / eps
C_D = 16.0       # |offdiag V^T (A^T A) V|      / (eps s_max^2)
C_U = 64.0       # |U^T U - I|                  / (eps cond^2),  rows with s_min > sqrt(eps) s_max
C_0 = 4.0        # null singular values         / (sqrt(eps) s_max)
C_G = 1.0        # def-regu gradient per row    / first_order_bounds()["grad"] (which already carries C_S and C_U)
C_B = 32.0       # singular-value gradient per row / svals_grad_bound()
C_R = 32.0       # reductions: |loss - loss64| <= C_R eps sum|terms| (fixed-order float32 tree over <= 2.4M terms: log2(n) eps)


# ------------------------------------------------------------------------------------------------ float64 references
def svd64(A):
    """Singular values (descending) of the float32 inputs promoted to float64: [n,3]."""
    return np.linalg.svd(np.asarray(A, dtype=np.float32).astype(np.float64), compute_uv=False)


def _gm(x, c):
    y = x / (c * c)
    return 2. * y / (y + 4.)


def def_regu64(J, c):
    """Per-row value GM(sum_k log(s_k)^2, c) [n] and its d/dJ [n,3,3] (model/network.py:576-579, utils/utils.py:48-52) in float64,
    through torch.linalg.svdvals autograd.  The loss is the mean of the values; its gradient is d/dJ / n."""
    Jd = torch.as_tensor(np.asarray(J, dtype=np.float32)).double().requires_grad_(True)
    s = torch.log(torch.linalg.svdvals(Jd))
    val = _gm((s * s).sum(1), float(c))
    g, = torch.autograd.grad(val.sum(), Jd)
    return val.detach().numpy(), g.numpy()


def svals_grad64(J, gS):
    """d <gS, svdvals(J)> / dJ in float64: [n,3,3]."""
    Jd = torch.as_tensor(np.asarray(J, dtype=np.float32)).double().requires_grad_(True)
    s = torch.linalg.svdvals(Jd)
    g, = torch.autograd.grad((s * torch.as_tensor(np.asarray(gS)).double()).sum(), Jd)
    return g.numpy()


# ------------------------------------------------------------------------------------------------ the float32 twin
def _rotate32(S, V, p, q):
    """One Jacobi rotation of the symmetric S [n,3,3] in the (p,q) plane, accumulated into V; float32 throughout.  Rows whose
    S_pq is below 1e-30 in magnitude are left alone (the contract's skip)."""
    f = np.float32
    r = 3 - p - q
    spq = S[:, p, q]
    live = np.abs(spq) >= f(1e-30)
    safe = np.where(live, spq, f(1))
    theta = (S[:, q, q] - S[:, p, p]) / (f(2) * safe)
    t = np.where(theta >= 0, f(1), f(-1)) / (np.abs(theta) + np.sqrt(theta * theta + f(1)))
    t = np.where(live, t, f(0)).astype(f)
    c = (f(1) / np.sqrt(t * t + f(1))).astype(f)
    s = (t * c).astype(f)
    spp, sqq, srp, srq = S[:, p, p].copy(), S[:, q, q].copy(), S[:, r, p].copy(), S[:, r, q].copy()
    S[:, p, p] = spp - t * spq
    S[:, q, q] = sqq + t * spq
    S[:, p, q] = S[:, q, p] = np.where(live, f(0), spq)
    S[:, r, p] = S[:, p, r] = c * srp - s * srq
    S[:, r, q] = S[:, q, r] = s * srp + c * srq
    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
    V[:, :, p] = c[:, None] * vp - s[:, None] * vq
    V[:, :, q] = s[:, None] * vp + c[:, None] * vq


def svd_twin32(A):
    """(U, S, V) of A [n,3,3] by the contract's algorithm in float32 numpy (no fma, numpy's sqrt and division)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    n = A.shape[0]
    S = np.einsum('nkr,nkc->nrc', A, A).astype(np.float32)
    V = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    with np.errstate(all='ignore'):
        for _ in range(6):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                _rotate32(S, V, p, q)
        ev = np.stack([S[:, 0, 0], S[:, 1, 1], S[:, 2, 2]], axis=1)
        order = np.argsort(-ev, axis=1, kind='stable')
        ev = np.take_along_axis(ev, order, axis=1)
        V = np.take_along_axis(V, order[:, None, :], axis=2)
        sv = np.sqrt(np.maximum(ev, np.float32(0))).astype(np.float32)
        inv = np.where(sv > np.float32(1e-20), np.float32(1) / np.where(sv > 0, sv, np.float32(1)), np.float32(0)).astype(np.float32)
        U = (np.einsum('nrc,nck->nrk', A, V).astype(np.float32) * inv[:, None, :]).astype(np.float32)
    return U, sv, V


def def_regu_grad_from_usv(U, S, V, c, g0=1.0):
    """The kernels' gradient formula, U diag(gS) V^T with gS_k = g0 GM'(x) 2 log(s_k) / s_k, evaluated in float32 from a float32
    (U, S, V): what the twin predicts for sr_def_regu_loss_bwd."""
    f = np.float32
    with np.errstate(all='ignore'):
        l = np.log(S.astype(f))
        x = (l * l).sum(1, dtype=f)
        y = x / f(c * c)
        dgm = f(8) / ((y + f(4)) * (y + f(4))) / f(c * c)
        gs = (f(g0) * dgm)[:, None] * f(2) * l / S
        return np.einsum('nak,nk,nbk->nab', U.astype(f), gs.astype(f), V.astype(f)).astype(f)


def svals_grad_from_uv(U, V, gS):
    return np.einsum('nak,nk,nbk->nab', U.astype(np.float32), np.asarray(gS, dtype=np.float32), V.astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ budgets
def first_order_bounds(J64, c=None, g0=1.0):
    """Per-row error budgets of the A^T A route for the float64 matrices J64 [n,3,3], WITHOUT the constants except where stated:
      s     [n,3]  eps s_max^2 / max(s_k, sqrt(eps) s_max)          (times C_S)
      v     [n]    eps                                               (times C_V)
      d     [n]    eps s_max^2                                       (times C_D)
      u     [n]    eps cond^2, NaN where s_min <= sqrt(eps) s_max    (times C_U)
      null  [n]    sqrt(eps) s_max                                   (times C_0)
      cond  [n]    s_max / s_min (inf for singular rows)
    and, when c is given, the budget of the deformation-regulariser gradient per row (times C_G), constants C_S and C_U included:
      grad  [n]    max_k sum_j |d gs_k / d s_j| C_S ds_j  +  C_U eps cond^2 max|gJ64|
      val   [n]    sum_k |gs_k| C_S ds_k + 4 (C_S eps)^2 g0 / c^2: the row's value g0 GM(x), with its second-order floor at s = 1
    with ds_j = eps s_max^2 / s_j and gs_k = g0 GM'(x) 2 log(s_k) / s_k, x = sum_k log(s_k)^2:
      d gs_k / d s_j = g0 [ GM''(x) (2 log s_j / s_j)(2 log s_k / s_k) + GM'(x) delta_kj 2 (1 - log s_k) / s_k^2 ]."""
    J64 = np.asarray(J64, dtype=np.float64)
    s = np.linalg.svd(J64, compute_uv=False)
    smax, smin = s[:, 0], s[:, 2]
    with np.errstate(all='ignore'):
        out = {
            's': EPS * (smax * smax)[:, None] / np.maximum(s, SQRT_EPS * smax[:, None]),
            'v': np.full(len(s), EPS),
            'd': EPS * smax * smax,
            'null': SQRT_EPS * smax,
            'cond': np.where(smin > 0, smax / np.where(smin > 0, smin, 1.), np.inf),
            's64': s,
        }
        out['u'] = np.where(smin > SQRT_EPS * smax, EPS * out['cond'] ** 2, np.nan)
        if c is not None:
            c2 = float(c) ** 2
            l = np.log(s)
            x = (l * l).sum(1)
            y = x / c2
            d1 = 8. / (y + 4.) ** 2 / c2                            # GM'(x)
            d2 = -16. / (y + 4.) ** 3 / (c2 * c2)                    # GM''(x)
            a = 2. * l / s                                           # d x / d s_k
            ds = C_S * EPS * (smax * smax)[:, None] / s
            jac = d2[:, None, None] * a[:, :, None] * a[:, None, :]
            jac = jac + d1[:, None, None] * np.eye(3)[None] * (2. * (1. - l) / (s * s))[:, :, None]
            dgs = abs(g0) * (np.abs(jac) * ds[:, None, :]).sum(2)    # [n,k]
            gs = g0 * d1[:, None] * a
            U, _, Vt = np.linalg.svd(J64)
            gJ = np.einsum('nak,nk,nkb->nab', U, gs, Vt)
            out['gJ64'] = gJ
            out['grad'] = dgs.max(1) + C_U * EPS * out['cond'] ** 2 * np.abs(gJ).reshape(len(s), -1).max(1)
            # the row's value GM(x): first order in ds, plus the second-order floor where gs vanishes (s = 1: x ~ 3 ds^2, GM ~ x / 2c^2)
            out['val'] = abs(g0) * ((np.abs(d1[:, None] * a) * ds).sum(1) + 4. * (C_S * EPS) ** 2 / c2)
    return out


def svals_grad_bound(J64, gS):
    """Per-row budget (times C_B) of U diag(gS) V^T against float64.  The Jacobi eigenvectors of A^T A are accurate to
    eps s_max^2 / |s_i^2 - s_j^2| within the plane of a close pair, which matters exactly as far as the pair's cotangents differ;
    u_k = A v_k / s_k adds eps cond^2:
        eps [ cond^2 max|gS| + sum_{i<j} |gS_i - gS_j| s_max^2 / |s_i^2 - s_j^2| ]."""
    s = np.linalg.svd(np.asarray(J64, dtype=np.float64), compute_uv=False)
    gS = np.asarray(gS, dtype=np.float64)
    smax = s[:, 0]
    with np.errstate(all='ignore'):
        b = (smax / s[:, 2]) ** 2 * np.abs(gS).max(1)
        for i, j in ((0, 1), (0, 2), (1, 2)):
            dg = np.abs(gS[:, i] - gS[:, j])
            gap = np.abs(s[:, i] ** 2 - s[:, j] ** 2)
            b = b + np.where(dg > 0, dg * smax * smax / gap, 0.)
    return EPS * b


def det_terms64(J64):
    """(det, sum of the magnitudes of the six products of the cofactor expansion) per row, float64: the float32 determinant of
    inv3 is within a few eps of the second of the first."""
    m = np.asarray(J64, dtype=np.float64).reshape(-1, 9).T
    prods = [m[0] * m[4] * m[8], -m[0] * m[5] * m[7], -m[1] * m[3] * m[8], m[1] * m[5] * m[6], m[2] * m[3] * m[7], -m[2] * m[4] * m[6]]
    return sum(prods), sum(np.abs(p) for p in prods)


def inv3_rule64(J64):
    """(ok, clear) of the |det| >= 1e-4 rule in float64; `clear` is False on rows whose |det| is within 8 eps sum|terms| of the
    threshold, where a float32 determinant may fall on either side."""
    det, mag = det_terms64(J64)
    return np.abs(det) >= DET_THRESHOLD, np.abs(np.abs(det) - DET_THRESHOLD) > 8. * EPS * mag


# ------------------------------------------------------------------------------------------------ inputs
def orth(rng, n, det=+1):
    """n random orthogonal 3x3 matrices (QR of a Gaussian, Haar) with the given determinant."""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.einsum('nii->ni', r))[:, None, :]
    flip = np.sign(np.linalg.det(q)) * det
    q[:, :, 2] *= flip[:, None]
    return q


def _conj(rng, s):
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    return np.einsum('nak,nk,nbk->nab', orth(rng, n), s, orth(rng, n))


def cases(seed=0, n=2000):
    """name -> float32 [rows,3,3], deterministic in (seed, n)."""
    rng = np.random.default_rng(seed)
    out = {}
    mild = np.eye(3)[None] + 0.25 * rng.standard_normal((n, 3, 3))
    out['mild'] = mild
    out['cond1e2'] = _conj(rng, 10. ** rng.uniform(-1., 1., (n, 3)))
    out['cond1e3'] = _conj(rng, 10. ** rng.uniform(-1.5, 1.5, (n, 3)))
    out['rotation'] = orth(rng, n)
    refl = orth(rng, n)
    refl[:, :, 1] *= -1.
    out['reflection'] = refl
    h = n // 2
    out['repeat2'] = np.concatenate([_conj(rng, np.tile([2., 1., 1.], (h, 1))), _conj(rng, np.tile([.7, .7, .3], (n - h, 1)))])
    out['repeat3'] = np.repeat(np.array([.5, 1., 2.]), [n // 3, n // 3, n - 2 * (n // 3)])[:, None, None] * orth(rng, n)
    out['identity'] = np.tile(np.eye(3), (64, 1, 1))
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    diag = []
    for base, flip in (((.5, 1., 2.), None), ((.5, 1., 2.), 0), ((.5, 1., 2.), 1), ((.5, 1., 2.), 2), ((1., 1., 2.), None)):
        for p in perms:
            d = np.array([base[i] for i in p])
            if flip is not None:
                d[flip] *= -1.
            diag.append(np.diag(d))
    out['diagonal'] = np.stack(diag)
    m = 256
    # half of each singular family by conjugation (rank up to float32 rounding of the entries), half exactly singular in float32
    r0, r1 = rng.standard_normal((m // 2, 3)), rng.standard_normal((m // 2, 3))
    out['rank2'] = np.concatenate([_conj(rng, np.stack([rng.uniform(.5, 2., m // 2), rng.uniform(.1, .5, m // 2), np.zeros(m // 2)], 1)),
                                   np.stack([r0, r1, 2. * r0.astype(np.float32)], axis=1)])
    out['rank1'] = np.concatenate([_conj(rng, np.stack([rng.uniform(.5, 2., m // 2), np.zeros(m // 2), np.zeros(m // 2)], 1)),
                                   np.stack([r0, 2. * r0.astype(np.float32), -.5 * r0.astype(np.float32)], axis=1)])
    out['zero'] = np.zeros((m, 3, 3))
    out['tiny'] = mild * 1e-3
    out['huge'] = mild * 1e3
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def cotangents(name, J, seed=1):
    """Random gS [n,3] for a family; equal within each group of repeated singular values (the gradient is only defined there)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((J.shape[0], 3))
    if name == 'repeat3':
        g[:, 1] = g[:, 0]; g[:, 2] = g[:, 0]
    elif name == 'repeat2':
        s = svd64(J)
        tie12 = (s[:, 0] - s[:, 1]) > (s[:, 1] - s[:, 2])
        g[tie12, 2] = g[tie12, 1]
        g[~tie12, 1] = g[~tie12, 0]
    return g.astype(np.float32)


def det_threshold_cases(seed=0, rows=64):
    """Jacobians Q diag(1, 1, d) with |d| on both sides of inv3's threshold: (J float32 [24 rows,3,3], d float64)."""
    rng = np.random.default_rng(seed)
    mags = [0., 5e-5, 9.9e-5, 1.01e-4, 2e-4, 1e-2]
    d = np.concatenate([np.full(rows, sgn * mag) for mag in mags for sgn in (1., -1.)])
    J = orth(rng, len(d)) * np.stack([np.ones_like(d), np.ones_like(d), d], axis=1)[:, None, :]
    return np.ascontiguousarray(J, dtype=np.float32), d


# ------------------------------------------------------------------------------------------------ reductions
def reduce64(mode, num, den, frame, N):
    """The three loss modes of reduce_rows in float64 from per-row (num, den) and the row's frame (-1: the row takes no part):
    mode 0: (1/N) sum_f num_f / max(den_f, 1)     mode 1: num_0 / den_0     mode 2: (1/N) sum_f (1 - num_f / den_f).
    Returns (loss, num_f [N], den_f [N], sum of |terms| for the rounding budget)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    frame = np.zeros(len(num), dtype=np.int64) if frame is None else np.asarray(frame, dtype=np.int64)
    live = frame >= 0
    nf = np.bincount(frame[live], weights=num[live], minlength=N)[:N]
    df = np.bincount(frame[live], weights=den[live], minlength=N)[:N]
    with np.errstate(all='ignore'):
        if mode == 0:
            per = nf / np.maximum(df, 1.)
            loss, mag = per.mean(), (np.abs(nf) / np.maximum(df, 1.)).mean()
        elif mode == 1:
            loss = nf[0] / df[0]
            mag = np.abs(num[live]).sum() / df[0]
        else:
            loss = (1. - nf / df).mean()
            mag = (1. + np.abs(nf / df)).mean() + (np.abs(nf / df)).mean()         # num_f and den_f both carry the tree's error
    return float(loss), nf, df, float(mag)


# ------------------------------------------------------------------------------------------------ the inv3 users and the row losses
# Composite torch formulations of the cited reference lines, in the dtype of their inputs: float64 is the reference, float32 on the
# CPU is what calibrates C_N below.  A frame index of -1 masks a row out.
C_N = 8.0        # normal-term gradients per row / normal_grad_bounds(): 4 x the worst ratio of this composite in float32 on the CPU
COND_TOL = 4e-6  # per unit of condition number: the row tolerance tests/test_step_ops_gpu.py uses for the adjugate inverse


def inv3_users64(J, v):
    """float64 (ok, cardinal ray normalize(J^-1 v) or v, deformed normal normalize(J^-T v) or normalize(J v)) per row
    (utils/utils.py:132-169 with FastMinv's |det| < 1e-4 rule)."""
    Jd, vd = torch.as_tensor(J).double(), torch.as_tensor(v).double()
    ok = torch.as_tensor(inv3_rule64(Jd.numpy())[0])
    inv = torch.linalg.inv(torch.where(ok[:, None, None], Jd, torch.eye(3, dtype=torch.float64)))
    cr = torch.where(ok[:, None], (inv * vd.unsqueeze(-2)).sum(-1), vd)
    dn = torch.where(ok[:, None], (inv.transpose(-2, -1) * vd.unsqueeze(-2)).sum(-1), (Jd * vd.unsqueeze(-2)).sum(-1))
    return ok.numpy(), (cr / cr.norm(dim=1, keepdim=True)).numpy(), (dn / dn.norm(dim=1, keepdim=True)).numpy()


def cardinal_bwd64(J, v, gout):
    """(gJ, gv) of normalize(J^-1 v) for the cotangent gout in float64; rows that fail the rule get zeros (rays.detach())."""
    Jd = torch.as_tensor(J).double().requires_grad_(True)
    vd = torch.as_tensor(v).double().requires_grad_(True)
    ok = torch.as_tensor(inv3_rule64(Jd.detach().numpy())[0])
    inv = torch.linalg.inv(torch.where(ok[:, None, None], Jd, torch.eye(3, dtype=torch.float64)))
    cr = torch.where(ok[:, None], (inv * vd.unsqueeze(-2)).sum(-1), vd.detach())
    out = cr / cr.norm(dim=1, keepdim=True)
    gJ, gv = torch.autograd.grad(out, [Jd, vd], torch.as_tensor(gout).double())
    return gJ.numpy(), gv.numpy()


def implicit_solve64(gf, J, v, gl):
    """model/network.py:702-771 in float64: (ok, cot_f [P], rhs_tail [P,3], temp [P,3], cond(b^T b), |det| clear of the threshold)."""
    gf, J, v, gl = (torch.as_tensor(t).double() for t in (gf, J, v, gl))
    z = torch.zeros(len(v), dtype=torch.float64)
    vx = torch.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], dim=1).view(-1, 3, 3)
    b = torch.cat([gf.view(-1, 1, 3), vx @ J], dim=1)
    btb = b.permute(0, 2, 1) @ b
    ok, clear = inv3_rule64(btb.numpy())
    okt = torch.as_tensor(ok)
    inv = torch.linalg.inv(torch.where(okt[:, None, None], btb, torch.eye(3, dtype=torch.float64))) * okt[:, None, None]
    rhs = gl.view(-1, 1, 3) @ (inv @ b.permute(0, 2, 1))
    temp = (rhs[:, :, 1:] @ (-vx)).view(-1, 3)
    cond = torch.linalg.cond(btb).clamp(max=1e12)
    return ok, -rhs[:, 0, 0].numpy(), rhs[:, 0, 1:].numpy(), temp.numpy(), cond.numpy(), clear


def frame_mean(per, cnt, b, N):
    """(1/N) sum_f (sum of per over the rows of frame f) / max(sum of cnt, 1); rows with b = -1 take no part."""
    live = (b >= 0).to(per.dtype)
    idx = b.clamp(min=0)
    ssum = torch.zeros(N, dtype=per.dtype, device=per.device).index_add(0, idx, per * live)
    scnt = torch.zeros(N, dtype=per.dtype, device=per.device).index_add(0, idx, cnt * live)
    return (ssum / scnt.clamp(min=1)).mean()


def normal_rows(nx_raw, J, g_rows, R, rays, weighted):
    """model/network.py:620-639 per ray, in the dtype of nx_raw: g_rows [P,3] are the ground-truth camera-space normals of the rays'
    pixels.  Returns (per-row term, valid as 0/1, dict of the quantities the error budget needs)."""
    dt = nx_raw.dtype
    nlen = nx_raw.norm(dim=1, keepdim=True)
    nx = nx_raw / nlen
    flip = torch.tensor([[-1., 0., 0.], [0., 1., 0.], [0., 0., -1.]], dtype=dt, device=nx_raw.device)
    g = g_rows.to(dt) @ (R.to(dt) @ flip).t()
    gn = g.norm(dim=1, keepdim=True)
    valid = (gn > 0.0001)[..., 0]
    g = torch.where(valid[:, None], g / gn.clamp(min=1e-12), g)
    t = (J.transpose(-2, -1) * g.unsqueeze(-2)).sum(-1)
    e = t - nx
    elen = e.norm(2, dim=1)
    if weighted:
        Jn, nn = J.detach().double().cpu(), nx_raw.detach().double().cpu()
        cn = torch.as_tensor(inv3_users64(Jn.numpy(), nn.numpy())[2]).to(nx_raw.device)
        w = (torch.clamp((-rays.double() * cn).sum(1), max=1., min=0.) ** 2).to(dt)
    else:
        w = torch.ones_like(elen)
    per = torch.where(valid, elen * w, torch.zeros((), dtype=dt, device=nx_raw.device))
    return per, valid.to(dt), {'t': t.detach().norm(dim=1), 'elen': elen.detach(), 'nlen': nlen.detach()[:, 0], 'w': w.detach()}


def normal_grad_bounds(aux, scale):
    """Per-row budgets (times C_N) of the normal term's gradients: e = J^T g - n is a difference of O(1 + |t|) numbers divided by |e|,
    the gradient of the raw normal is divided by |nx_raw| once more.  scale [P] = g0 w / max(den_f, 1)."""
    ge = EPS * scale * (1. + aux['t']) / aux['elen'].clamp(max=1.)
    return ge / aux['nlen'], ge           # (gnx_raw, gJ)
