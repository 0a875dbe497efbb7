"""The per-row 3x3 kernels of the optimisation step and the loss reductions around them, launch by launch against float64:
sr_svd3x3 (csrc/small_ops.hip) and sr_svd3x3_bwd, sr_def_regu_loss_{fwd,bwd}, inv3 and its users, reduce_rows (csrc/step_ops.hip).

References, input families and error budgets are in tests/_step3x3_ref.py; the budget constants are calibrated there against
float64 with a float32 restatement of the contract on the CPU (tests/test_step3x3_ref_cpu.py), never with the kernels.  Every test
prints its worst observed ratio to its budget (`pytest -s`); profiles/step_tails_accuracy.md records them.

Two accuracy limits of the kernel's route (Jacobi on J^T J in float32) are design properties that these tests pin as they are:
singular values carry eps s_max^2 / s_k, so the deformation regulariser's gradient is accurate to eps cond(J)^2 per row, and a null
singular value comes back as about sqrt(eps) s_max instead of 0."""
import ctypes

import numpy as np
import pytest
import torch

import _step3x3_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = ref.EPS
MARGIN = 64                       # sentinel floats (bytes for the ok flags) on either side of every output buffer
SENTINEL = -7777.25
LAUNCH_CAP = 2048 * 256           # rows one pass of a capped sr_stream_grid launch covers
ROW_COUNTS = [0, 1, 255, 256, 257, LAUNCH_CAP, LAUNCH_CAP + 1, 1048579]
RED_ROWS = [1, 1023, 1024, 1025, 32768, 32769, 40960, 40961]


# ------------------------------------------------------------------------------------------------ helpers
class Guarded:
    """An output buffer of `shape` filled with NaN (0x77 for uint8) between two sentinel margins."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.flag = dtype == torch.uint8
        self.sent = 0xA5 if self.flag else SENTINEL
        self.buf = torch.full((n + 2 * MARGIN,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[MARGIN:MARGIN + n].view(shape)
        self.t.fill_(0x77 if self.flag else float('nan'))

    def intact(self):
        return bool((self.buf[:MARGIN] == self.sent).all()) and bool((self.buf[MARGIN + self.t.numel():] == self.sent).all())


def _lib():
    from selfreconcode_amd import _lib as lib
    return lib


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype).contiguous()


def rowmax(x):
    return x.abs().reshape(x.shape[0], -1).amax(1) if x.shape[0] else x.new_zeros((0,))


def worst(label, err, budget):
    """max err / budget over rows with a positive budget (printed); asserts err <= budget everywhere."""
    err, budget = err.double(), budget.double().expand_as(err)
    assert bool(torch.isfinite(err).all()), f"{label}: non-finite error"
    ratio = (err / budget.clamp(min=1e-300)).max().item() if err.numel() else 0.
    print(f"ratio {label}: {ratio:.3g}")
    bad = err > budget
    assert not bool(bad.any()), f"{label}: {int(bad.sum())} of {err.numel()} over budget, worst ratio {ratio:.4g}"
    return ratio


def svd_gpu(A, n=None):
    """(U, S, V, guards) of sr_svd3x3 on A [n,3,3] (device float32)."""
    n = A.shape[0] if n is None else n
    U, S, V = Guarded((n, 3, 3)), Guarded((n, 3)), Guarded((n, 3, 3))
    _lib().launch("sr_svd3x3", U.buf, A, n, U.t, S.t, V.t)
    return U.t, S.t, V.t, (U, S, V)


@pytest.fixture(scope="module")
def fam():
    return ref.cases(0)


@pytest.fixture(scope="module")
def bounds(fam):
    return {k: ref.first_order_bounds(v.astype(np.float64)) for k, v in fam.items()}


def check_svd_contract(label, A, U, S, V, b, idx=None):
    """The contract of sr_svd3x3 on device tensors; b = first_order_bounds of the distinct rows, idx maps rows to them."""
    pick = (lambda x: dev(x, torch.float64)) if idx is None else (lambda x: dev(x, torch.float64)[idx])
    A64, U64, S64, V64 = A.double(), U.double(), S.double(), V.double()
    eye = torch.eye(3, dtype=torch.float64, device=DEV)
    assert bool(torch.isfinite(S).all()) and bool(torch.isfinite(U).all()) and bool(torch.isfinite(V).all()), label
    assert bool((S >= 0).all()) and bool((S[:, 0] >= S[:, 1]).all()) and bool((S[:, 1] >= S[:, 2]).all()), label
    worst(f"{label} C_S", (S64 - pick(b['s64'])).abs(), ref.C_S * pick(b['s']))
    worst(f"{label} C_V", rowmax(torch.einsum('nka,nkb->nab', V64, V64) - eye), ref.C_V * pick(b['v']))
    D = torch.einsum('nka,nkl,nlb->nab', V64, torch.einsum('nka,nkb->nab', A64, A64), V64) * (1 - eye)
    worst(f"{label} C_D", rowmax(D), ref.C_D * pick(b['d']))
    # column k of V belongs to s_k: its Rayleigh quotient is s_k^2 (off by at most the residual coupling, C_D eps s_max^2, plus the
    # 2 s ds of the singular value's own budget) ...
    AV = torch.einsum('nrc,nck->nrk', A64, V64)
    smax = pick(b['s64'])[:, :1]
    worst(f"{label} V order", ((AV * AV).sum(1) - pick(b['s64']) ** 2).abs(), (ref.C_D + 2 * ref.C_S) * EPS * smax * smax)
    # ... and to u_k = A v_k / s_k: three products per entry (3 eps/2 |a_row| |v| <= 1.5 eps s_max), one reciprocal and one product
    # (eps |A v_k| <= eps s_max) bound |A v_k - s_k u_k| by 2.5 eps s_max; 8 allows for |v| = 1 + C_V eps and the row norms' slack
    worst(f"{label} U pairing", rowmax(AV - U64 * S64[:, None, :]), 8 * EPS * smax[:, 0])
    bu = pick(b['u'])
    live = ~torch.isnan(bu)
    if bool(live.any()):
        worst(f"{label} C_U", rowmax(torch.einsum('nka,nkb->nab', U64, U64) - eye)[live], ref.C_U * bu[live])


# ------------------------------------------------------------------------------------------------ SVD contract
FAMILIES = ['mild', 'cond1e2', 'cond1e3', 'rotation', 'reflection', 'repeat2', 'repeat3', 'identity', 'diagonal', 'rank2', 'rank1', 'zero',
            'tiny', 'huge']


@pytest.mark.parametrize("name", FAMILIES)
def test_svd3x3_contract(fam, bounds, name):
    """S finite, non-negative, descending and within C_S eps s_max^2 / max(s_k, sqrt(eps) s_max) of float64; V orthogonal to
    C_V eps and diagonalising A^T A to C_D eps s_max^2 (U S V^T = A alone would not show a wrong V: U is A V / S); U orthogonal to
    C_U eps cond^2.  Documented limit of the J^T J route: the null singular values of a rank-deficient matrix come back as up to
    C_0 sqrt(eps) s_max (about 3.5e-4 s_max per unit of C_0), not 0; U's columns for them are then not orthogonal and are not checked."""
    A = dev(fam[name])
    U, S, V, guards = svd_gpu(A)
    assert all(g.intact() for g in guards)
    b = bounds[name]
    if name == 'zero':
        assert bool((S == 0).all()) and bool((U == 0).all()) and bool(torch.isfinite(V).all())
        eye = torch.eye(3, dtype=torch.float64, device=DEV)
        worst("zero C_V", rowmax(torch.einsum('nka,nkb->nab', V.double(), V.double()) - eye), torch.full((len(A),), ref.C_V * EPS, device=DEV))
        return
    check_svd_contract(name, A, U, S, V, b)
    if name in ('identity', 'rotation', 'repeat3'):
        k = dev(np.round(b['s64'][:, 0] * 2) / 2, torch.float64)              # 0.5, 1 or 2
        worst(f"{name} |s - k|", (S.double() - k[:, None]).abs().amax(1), ref.C_S * EPS * k)
    if name in ('rank1', 'rank2'):
        null = S[:, (1 if name == 'rank1' else 2):].double().amax(1)
        worst(f"{name} C_0", null, ref.C_0 * dev(b['null'], torch.float64))
    if name == 'diagonal':                                                       # nothing to rotate: the sort alone, exactly
        want = np.sort(np.abs(np.einsum('nii->ni', fam[name])), axis=1)[:, ::-1]
        assert (np.abs(S.cpu().numpy() - want) <= 2 * EPS * want).all()
        assert bool(((V.abs() == 1).sum((1, 2)) == 3).all()) and bool(((V != 0).sum((1, 2)) == 3).all())


# ------------------------------------------------------------------------------------------------ backward entries
@pytest.mark.parametrize("name", ['mild', 'cond1e2', 'reflection', 'tiny', 'huge', 'repeat2', 'repeat3'])
def test_svd3x3_bwd_and_singular_values_autograd(fam, name):
    """sr_svd3x3_bwd through _lib.launch and ops.singular_values_3x3 through autograd against the float64 gradient of
    <gS, svdvals(J)> within C_B svals_grad_bound() per row, and against each other to 4 eps max|gJ| per row."""
    from selfreconcode_amd.ops import singular_values_3x3
    A = fam[name]
    gS = ref.cotangents(name, A)
    want = dev(ref.svals_grad64(A, gS), torch.float64)
    budget = ref.C_B * dev(ref.svals_grad_bound(A.astype(np.float64), gS), torch.float64)
    Ad, gSd = dev(A), dev(gS)
    U, S, V, _ = svd_gpu(Ad)
    gJ = Guarded(A.shape)
    _lib().launch("sr_svd3x3_bwd", gJ.buf, U, V, gSd, len(A), gJ.t)
    assert gJ.intact()
    worst(f"{name} C_B launch", rowmax(gJ.t.double() - want), budget)
    J = Ad.clone().requires_grad_(True)
    S2 = singular_values_3x3(J)
    assert torch.equal(S2, S)
    g2, = torch.autograd.grad(S2, J, gSd)
    assert g2.shape == J.shape
    worst(f"{name} C_B autograd", rowmax(g2.double() - want), budget)
    worst(f"{name} launch vs autograd", rowmax(g2.double() - gJ.t.double()), 4 * EPS * rowmax(want).clamp(min=1e-30))


# ------------------------------------------------------------------------------------------------ deformation regulariser
@pytest.mark.parametrize("c", [0.5, 2.0])
@pytest.mark.parametrize("name", ['mild', 'cond1e2', 'rotation', 'identity', 'repeat2', 'reflection'])
def test_def_regu_loss_value_and_gradient_per_row(fam, name, c):
    """DefReguLoss against def_regu64: the value within the summed first-order budget of the rows, the gradient per row within
    C_G first_order_bounds()['grad'] -- C_S eps s_max^2 / s_k propagated through gs_k = g0 GM'(x) 2 log(s_k) / s_k plus
    C_U eps cond^2 max|gJ64| -- which is an eps cond^2 statement, not a blanket rtol.  Rows with all s_k = 1 have a zero gradient in
    float64; there the budget is its absolute floor C_S eps g0 / c^2 and nothing non-finite may come from log(1) / s."""
    from selfreconcode_amd.step_ops import DefReguLoss
    A = fam[name]
    n = len(A)
    val64, g64 = ref.def_regu64(A, c)
    b = ref.first_order_bounds(A.astype(np.float64), c=c, g0=1. / n)
    J = dev(A).requires_grad_(True)
    loss = DefReguLoss.apply(J, c)
    g, = torch.autograd.grad(loss, J)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss))
    want, mag = val64.sum() / n, np.abs(val64).sum() / n
    tol = b['val'].sum() + ref.C_R * EPS * mag
    print(f"ratio {name} c={c} value: {abs(loss.item() - want) / tol:.3g}")
    assert abs(loss.item() - want) <= tol, (loss.item(), want, tol)
    worst(f"{name} c={c} C_G", rowmax(g.double() - dev(g64 / n, torch.float64)), ref.C_G * dev(b['grad'], torch.float64))
    if name in ('identity', 'rotation'):
        floor = ref.C_S * EPS / (c * c) / n
        assert np.abs(g64).max() / n <= 0.1 * floor                     # float64: zero up to the float32 rounding of the rotations' entries
        assert rowmax(g).max().item() <= ref.C_G * floor
    loss2 = DefReguLoss.apply(J, c)
    g2, = torch.autograd.grad(loss2, J)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


# ------------------------------------------------------------------------------------------------ inv3 threshold users
def _cond_tol(J64, want, cond=None):
    cond = np.minimum(np.linalg.cond(J64), 1e12) if cond is None else cond
    return ref.COND_TOL * cond * np.maximum(np.abs(want).reshape(len(want), -1).max(1), 1e-3)


def test_inv3_users_on_both_sides_of_the_determinant_threshold():
    """CardinalRays (forward, backward), deformed_normals, the weighted NormalLoss and implicit_solve on matrices whose determinant
    sits on both sides of 1e-4: |det| in {0, 5e-5, 9.9e-5, 1.01e-4, 2e-4, 1e-2}, both signs, 64 rows each, J = Q diag(1, 1, det).
    ok equals the float64 rule (rows within 8 eps sum|cofactor terms| of the threshold may flip: at most 1%, here none) and all
    users agree with one another; outputs on both branches are within the condition-scaled row tolerance of
    test_implicit_solve_vs_reference_lines.  implicit_solve inverts b^T b, which is positive semi-definite: with J = Q orthogonal and
    grad_f = sqrt(|det|) Q^T v its determinant is |det| exactly, so its rows cover the positive side twice."""
    from selfreconcode_amd.step_ops import CardinalRays, deformed_normals, NormalLoss, implicit_solve
    Jn, d = ref.det_threshold_cases(0)
    P = len(Jn)
    rng = np.random.default_rng(5)
    vn = rng.standard_normal((P, 3)); vn = (vn / np.linalg.norm(vn, axis=1, keepdims=True)).astype(np.float32)
    J64 = Jn.astype(np.float64)
    ok64, clear = ref.inv3_rule64(J64)
    assert (~clear).mean() <= 0.01
    ok_r, cr64, dn64 = ref.inv3_users64(Jn, vn)
    # the condition of what each branch computes: the inverse where the rule holds, v itself / J v where it does not
    cond_c = np.where(ok64, np.minimum(np.linalg.cond(J64), 1e12), 1.)
    cond_n = np.where(ok64, cond_c, 1. / np.linalg.norm(np.einsum('nab,nb->na', J64, vn.astype(np.float64)), axis=1))
    J, v = dev(Jn).requires_grad_(True), dev(vn).requires_grad_(True)
    out, ok = CardinalRays.apply(J, v)
    okn = ok.cpu().numpy()
    assert np.array_equal(okn[clear], ok64[clear]) and okn.sum() >= 3 * 128 - (~clear).sum()
    same = dev(okn == ok64, torch.bool)
    worst("inv3 cardinal", rowmax(out.double() - dev(cr64, torch.float64))[same], dev(_cond_tol(J64, cr64, cond_c), torch.float64)[same])
    gout = rng.standard_normal((P, 3)).astype(np.float32)
    gJ, gv = torch.autograd.grad(out, [J, v], dev(gout))
    gJ64, gv64 = ref.cardinal_bwd64(Jn, vn, gout)
    # the backward applies the inverse twice: twice the forward's condition-scaled tolerance, on the scale |J^-1| of the row
    scale = np.maximum(np.abs(gJ64).reshape(P, -1).max(1), np.abs(gv64).max(1))
    tol = dev(2 * _cond_tol(J64, scale[:, None], cond_c), torch.float64)
    worst("inv3 cardinal gJ", rowmax(gJ.double() - dev(gJ64, torch.float64))[same], tol[same])
    worst("inv3 cardinal gv", rowmax(gv.double() - dev(gv64, torch.float64))[same], tol[same])
    assert float(gJ[~ok].abs().max()) == 0. and float(gv[~ok].abs().max()) == 0.
    nx = deformed_normals(J.detach(), v.detach())
    worst("inv3 deformed normals", rowmax(nx.double() - dev(dn64, torch.float64))[same], dev(_cond_tol(J64, dn64, cond_n), torch.float64)[same])
    # weighted normal term: the weights go through the same rule (detached); one frame, every pixel valid
    N, H, W = 2, 8, 8
    g = torch.Generator().manual_seed(3)
    b = torch.randint(0, N, (P,), generator=g); r = torch.randint(0, H, (P,), generator=g); cc = torch.randint(0, W, (P,), generator=g)
    gtn = torch.randn(N, H, W, 3, generator=g)
    R = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    rays = torch.nn.functional.normalize(-torch.as_tensor(dn64).float() + 0.3 * torch.randn(P, 3, generator=g), dim=1)
    nraw = v.detach().clone().requires_grad_(True)
    J2 = J.detach().clone().requires_grad_(True)
    loss = NormalLoss.apply(nraw, J2, gtn.to(DEV), R.to(DEV), rays.to(DEV), True, b.to(DEV), r.to(DEV), cc.to(DEV))
    got = torch.autograd.grad(loss, [nraw, J2])
    a64, Jd = torch.as_tensor(vn).double().requires_grad_(True), torch.as_tensor(J64).requires_grad_(True)
    res = {}
    for weighted in (True, False):
        per, cnt, aux = ref.normal_rows(a64, Jd, gtn[b, r, cc], R, rays, weighted)
        l64 = ref.frame_mean(per, cnt, b, N)
        res[weighted] = (l64.item(), per.detach(), aux) + torch.autograd.grad(l64, [a64, Jd])
    den = torch.bincount(b, minlength=N).double().clamp(min=1)[b] * N
    cond = torch.as_tensor(cond_n)
    dw = 2 * ref.COND_TOL * cond                                        # of w = clamp(-v . n_deformed, 0, 1)^2
    keep = torch.as_tensor(okn == ok64)
    assert bool(keep.all())                                              # (no unclear rows in this list: the sums below need every row)
    tol_l = (res[False][1] * dw / den).sum().item() + ref.C_R * EPS * abs(res[True][0])
    print(f"ratio inv3 normal loss: {abs(loss.item() - res[True][0]) / tol_l:.3g}")
    assert abs(loss.item() - res[True][0]) <= tol_l
    bn, bJ = ref.normal_grad_bounds(res[True][2], res[True][2]['w'] / den)
    for name_, a, w64, unw, bb in (("gnx", got[0], res[True][3], res[False][3], bn), ("gJ", got[1], res[True][4], res[False][4], bJ)):
        worst(f"inv3 normal {name_}", rowmax(a.double().cpu() - w64), ref.C_N * bb + dw * rowmax(unw))
    # implicit solve
    Q = ref.orth(np.random.default_rng(6), P)
    gf = (np.sqrt(np.abs(d))[:, None] * np.einsum('nki,nk->ni', Q, vn.astype(np.float64))).astype(np.float32)
    gl = rng.standard_normal((P, 3)).astype(np.float32)
    Qf = Q.astype(np.float32)
    oki, cot, tail, temp, condb, cleari = ref.implicit_solve64(gf, Qf, vn, gl)
    assert (~cleari).mean() <= 0.01 and oki.sum() >= 300 and (~oki).sum() >= 300
    cot_g, tail_g, temp_g, ok_g = implicit_solve(dev(gf), dev(Qf), dev(vn), dev(gl))
    okg = ok_g.cpu().numpy()
    assert np.array_equal(okg[cleari], oki[cleari])
    same = dev(okg == oki, torch.bool)
    scale = np.maximum(np.abs(cot), np.abs(tail).max(1))
    tol = dev(ref.COND_TOL * condb * np.maximum(scale, 1e-3), torch.float64)
    for name_, a, w in (("cot_f", cot_g[:, None], cot[:, None]), ("rhs_tail", tail_g, tail), ("temp", temp_g, temp)):
        worst(f"inv3 implicit {name_}", rowmax(a.double() - dev(w, torch.float64))[same], tol[same])
    assert float(cot_g[~ok_g].abs().max()) == 0. and float(tail_g[~ok_g].abs().max()) == 0. and float(temp_g[~ok_g].abs().max()) == 0.


# ------------------------------------------------------------------------------------------------ launch edges of the row kernels
@pytest.fixture(scope="module")
def tile(fam):
    """The distinct rows every launch-edge size is tiled from, with their float64 references (computed once)."""
    A = fam['mild']
    T = len(A)
    rng = np.random.default_rng(9)
    t = {'A': A, 'T': T, 'b': ref.first_order_bounds(A.astype(np.float64))}
    t['gS'] = ref.cotangents('mild', A)
    t['svals_grad'] = ref.svals_grad64(A, t['gS'])
    t['svals_bound'] = ref.C_B * ref.svals_grad_bound(A.astype(np.float64), t['gS'])
    t['v'] = rng.standard_normal((T, 3)).astype(np.float32)
    t['gout'] = rng.standard_normal((T, 3)).astype(np.float32)
    t['gf'] = rng.standard_normal((T, 3)).astype(np.float32)
    t['gl'] = rng.standard_normal((T, 3)).astype(np.float32)
    ok, t['cr'], t['dn'] = ref.inv3_users64(A, t['v'])
    assert ok.all()
    t['crJ'], t['crv'] = ref.cardinal_bwd64(A, t['v'], t['gout'])
    t['imp'] = ref.implicit_solve64(t['gf'], A, t['v'], t['gl'])
    t['def'] = ref.def_regu64(A, 0.5)
    t['dev'] = {k: dev(t[k]) for k in ('A', 'gS', 'v', 'gout', 'gf', 'gl')}
    return t


def _eikonal_grad_budget(s, ln):
    """s (len - 1) / len v in float32: len - 1 carries 2 eps len, the quotient and the products 3 eps more, |v_k| <= len: the row is
    within s eps (2 len + 3 |len - 1|); 4 x that."""
    return 4 * s * EPS * (2 * ln + 3 * (ln - 1).abs())


def _tiled(t, key, idx):
    return t['dev'][key][idx].contiguous()


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_kernels_at_launch_edges(tile, n):
    """sr_svd3x3, sr_svd3x3_bwd, sr_def_regu_loss_bwd, sr_eikonal_loss_bwd, sr_cardinal_rays_{fwd,bwd}, sr_deformed_normals and
    sr_implicit_solve at row counts around the block size and around the 2048 x 256 grid cap (the last two sizes run the
    grid-stride loop), every row against float64, every output between untouched sentinel margins and fully written."""
    lib, t, T = _lib(), tile, tile['T']
    idx = torch.arange(n, device=DEV) % T
    f64 = lambda x: dev(x, torch.float64)[idx]
    A, gS, v, gout, gf, gl = (_tiled(t, k, idx) for k in ('A', 'gS', 'v', 'gout', 'gf', 'gl'))
    anchor = t['dev']['A']
    U, S, V, guards = svd_gpu(A, n)
    assert all(g.intact() for g in guards)
    gloss = torch.ones(1, device=DEV)
    c = 0.5
    if n == 0:
        out = Guarded((1, 9))
        lib.launch("sr_svd3x3_bwd", anchor, U, V, gS, 0, out.t)
        lib.launch("sr_cardinal_rays_fwd", anchor, A, v, 0, out.t, out.t)
        lib.launch("sr_cardinal_rays_bwd", anchor, A, v, 0, gout, out.t, out.t)
        lib.launch("sr_deformed_normals", anchor, A, v, 0, out.t)
        lib.launch("sr_implicit_solve", anchor, gf, A, v, gl, 0, out.t, out.t, out.t, out.t)
        for name in ("sr_def_regu_loss_bwd", "sr_eikonal_loss_bwd"):             # a mean over no rows is refused, not launched
            with pytest.raises(lib.SrError):
                args = (U, S, V, 0, c, gloss, out.t) if name == "sr_def_regu_loss_bwd" else (v, 0, gloss, out.t)
                lib.launch(name, anchor, *args)
        torch.cuda.synchronize()
        assert out.intact() and bool(torch.isnan(out.t).all())
        return
    check_svd_contract(f"n={n} svd", A, U, S, V, t['b'], idx)
    gJ = Guarded((n, 3, 3))
    lib.launch("sr_svd3x3_bwd", anchor, U, V, gS, n, gJ.t)
    assert gJ.intact()
    worst(f"n={n} svd_bwd", rowmax(gJ.t.double() - f64(t['svals_grad'])), f64(t['svals_bound']))
    gD = Guarded((n, 3, 3))
    lib.launch("sr_def_regu_loss_bwd", anchor, U, S, V, n, c, gloss, gD.t)
    assert gD.intact()
    b = ref.first_order_bounds(t['A'].astype(np.float64), c=c, g0=1. / n)
    worst(f"n={n} def_regu_bwd", rowmax(gD.t.double() - f64(t['def'][1]) / n), ref.C_G * f64(b['grad']))
    gE = Guarded((n, 3))
    lib.launch("sr_eikonal_loss_bwd", anchor, v, n, gloss, gE.t)
    assert gE.intact()
    v64 = v.double()
    ln = v64.norm(dim=1, keepdim=True)
    worst(f"n={n} eikonal_bwd", rowmax(gE.t.double() - 2. / n * (ln - 1) / ln * v64), _eikonal_grad_budget(2. / n, ln[:, 0]))
    cr, ok = Guarded((n, 3)), Guarded((n,), torch.uint8)
    lib.launch("sr_cardinal_rays_fwd", anchor, A, v, n, cr.t, ok.t)
    assert cr.intact() and ok.intact() and bool((ok.t == 1).all())
    cond = np.linalg.cond(t['A'].astype(np.float64))
    worst(f"n={n} cardinal_fwd", rowmax(cr.t.double() - f64(t['cr'])), ref.COND_TOL * f64(cond))
    cJ, cv = Guarded((n, 3, 3)), Guarded((n, 3))
    lib.launch("sr_cardinal_rays_bwd", anchor, A, v, n, gout, cJ.t, cv.t)
    assert cJ.intact() and cv.intact()
    scale = np.maximum(np.abs(t['crJ']).reshape(T, -1).max(1), np.abs(t['crv']).max(1))
    tol = 2 * ref.COND_TOL * f64(cond * np.maximum(scale, 1e-3))
    worst(f"n={n} cardinal_bwd gJ", rowmax(cJ.t.double() - f64(t['crJ'])), tol)
    worst(f"n={n} cardinal_bwd gv", rowmax(cv.t.double() - f64(t['crv'])), tol)
    dn = Guarded((n, 3))
    lib.launch("sr_deformed_normals", anchor, A, v, n, dn.t)
    assert dn.intact()
    worst(f"n={n} deformed_normals", rowmax(dn.t.double() - f64(t['dn'])), ref.COND_TOL * f64(cond))
    oki, cot, tail, temp, condb, _ = t['imp']
    o = [Guarded((n,)), Guarded((n, 3)), Guarded((n, 3)), Guarded((n,), torch.uint8)]
    lib.launch("sr_implicit_solve", anchor, gf, A, v, gl, n, o[0].t, o[1].t, o[2].t, o[3].t)
    assert all(g.intact() for g in o) and oki.mean() > 0.9
    clear_i, ok_i = dev(t['imp'][5], torch.bool)[idx], dev(oki, torch.bool)[idx]
    assert bool(((o[3].t == 1) == ok_i)[clear_i].all()) and bool((o[3].t <= 1).all())
    same = (o[3].t == 1) == ok_i
    tol = ref.COND_TOL * f64(condb * np.maximum(np.maximum(np.abs(cot), np.abs(tail).max(1)), 1e-3))
    worst(f"n={n} implicit cot_f", (o[0].t.double() - f64(cot)).abs()[same], tol[same])
    worst(f"n={n} implicit rhs_tail", rowmax(o[1].t.double() - f64(tail))[same], tol[same])
    worst(f"n={n} implicit temp", rowmax(o[2].t.double() - f64(temp))[same], tol[same])


# ------------------------------------------------------------------------------------------------ launch edges of the reductions
def _twice(fn):
    """fn() -> (loss, *grads), called twice: equal bits (step_ops.hip sums in a fixed order)."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    return a


def _value(label, loss, want, mag, extra=0.):
    tol = ref.C_R * EPS * mag + extra
    print(f"ratio {label} C_R: {abs(loss.item() - want) / max(tol, 1e-300):.3g}")
    assert np.isfinite(loss.item()) and abs(loss.item() - want) <= tol, (label, loss.item(), want, tol)


@pytest.mark.parametrize("n", RED_ROWS)
def test_mode1_reductions_at_launch_edges(fam, n):
    """Eikonal and deformation-regulariser losses (plain mean) around one wave-sized block (1024) and around the switch from one
    workgroup to several (32,768 rows; a block more per 8,192): value against reduce64 within C_R eps sum|terms|, gradients against
    float64, two calls bit-identical."""
    from selfreconcode_amd.step_ops import EikonalLoss, DefReguLoss
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, 3, generator=g) * 0.8).to(DEV).requires_grad_(True)

    def eik():
        loss = EikonalLoss.apply(x)
        return loss, torch.autograd.grad(loss * 0.1, x)[0]
    loss, gx = _twice(eik)
    x64 = x.detach().double()
    ln = x64.norm(dim=1, keepdim=True)
    per = ((ln[:, 0] - 1) ** 2).cpu().numpy()
    want, _, _, mag = ref.reduce64(1, per, np.ones(n), None, 1)
    # per row (len - 1)^2 in float32: 2 eps len / |len - 1| relative, i.e. 4 eps len |len - 1| absolute; 4 x that, averaged
    _value(f"eikonal n={n}", loss, want, mag, extra=(16 * EPS * ln[:, 0] * (ln[:, 0] - 1).abs()).mean().item())
    worst(f"eikonal n={n} grad", rowmax(gx.double() - 0.2 / n * (ln - 1) / ln * x64), _eikonal_grad_budget(0.2 / n, ln[:, 0]))
    A = np.tile(fam['mild'], (n // 2000 + 1, 1, 1))[:n]
    J = dev(A).requires_grad_(True)

    def regu():
        loss = DefReguLoss.apply(J, 0.5)
        return loss, torch.autograd.grad(loss, J)[0]
    loss, gJ = _twice(regu)
    val64, g64 = ref.def_regu64(A, 0.5)
    b = ref.first_order_bounds(A.astype(np.float64), c=0.5, g0=1. / n)
    want, _, _, mag = ref.reduce64(1, val64, np.ones(n), None, 1)
    _value(f"def_regu n={n}", loss, want, mag, extra=b['val'].sum())
    worst(f"def_regu n={n} C_G", rowmax(gJ.double() - dev(g64 / n, torch.float64)), ref.C_G * dev(b['grad'], torch.float64))


def _frames(P, N, kind, g):
    b = torch.randint(0, N, (P,), generator=g)
    if kind == 'sorted':
        b = b.sort().values
    elif kind == 'empty_bins':
        b[(b == 2) | (b == 5) | (b == 7)] = 3
    elif kind == 'masked':
        b[torch.rand(P, generator=g) < 0.3] = -1
    elif kind == 'all_bins' and P >= N:
        b[:N] = torch.arange(N)
    return b


def check_color_and_normal(P, N, kind, seed):
    """ColorLoss and NormalLoss (mode 0: scatter-mean over frames, then mean) on P rays of N frames against float64."""
    from selfreconcode_amd import step_ops
    from selfreconcode_amd.step_ops import ColorLoss, NormalLoss
    g = torch.Generator().manual_seed(seed)
    H, W = 16, 12
    b = _frames(P, N, kind, g)
    r, c = torch.randint(0, H, (P,), generator=g), torch.randint(0, W, (P,), generator=g)
    gt = torch.rand(N, H, W, 3, generator=g) * 2 - 1
    col0 = torch.rand(P, 3, generator=g) * 2 - 1
    live = b >= 0
    bd, rd, cd, gtd = b.to(DEV), r.to(DEV), c.to(DEV), gt.to(DEV)
    col = col0.to(DEV).requires_grad_(True)

    def colour():
        loss = ColorLoss.apply(col, gtd, bd, rd, cd)
        return loss, torch.autograd.grad(loss * 0.7, col)[0]
    loss, gc = _twice(colour)
    c64 = col0.double().requires_grad_(True)
    per = (gt.double()[b.clamp(min=0), r, c, :] - c64).abs().sum(1)
    l64 = ref.frame_mean(per, torch.ones(P, dtype=torch.float64), b, N)
    want, nf, df, mag = ref.reduce64(0, per.detach().numpy(), np.ones(P), b.numpy(), N)
    assert abs(want - l64.item()) <= 1e-12 * max(1., abs(want))
    _value(f"colour P={P} {kind}", loss, want, mag, extra=4 * EPS * mag)       # (the rows' own |d0| + |d1| + |d2| in float32)
    g64, = torch.autograd.grad(l64 * 0.7, c64)
    worst(f"colour P={P} {kind} grad", (gc.double().cpu() - g64).abs(), 4 * EPS * g64.abs())
    assert float(gc[~live.to(DEV)].abs().max()) == 0. if bool((~live).any()) else True
    # the per-frame denominators the backward reads, straight from the forward's output slots
    px, keep = step_ops._pixels(bd, rd, cd, N, H, W)
    out, partial = step_ops._loss_buffers(P, DEV)
    _lib().launch("sr_color_loss_fwd", col, ctypes.byref(px), col.detach(), gtd, partial, out)
    assert torch.equal(out[0], loss.detach())
    counts = torch.bincount(b[live], minlength=N).float()
    assert torch.equal(out[1 + 8:1 + 8 + N].cpu(), counts) and bool((out[1 + 8 + N:] == 0).all()) and df.tolist() == counts.tolist()
    # normal term, unweighted (the weights' inv3 path has its own test), with background pixels as invalid rows
    gtn = torch.randn(N, H, W, 3, generator=g)
    gtn[:, ::3] = 0.
    A = torch.as_tensor(np.tile(ref.cases(0)['mild'], (P // 2000 + 1, 1, 1))[:P])
    nraw0 = torch.randn(P, 3, generator=g) * 1.3
    R = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    nraw, J = nraw0.to(DEV).requires_grad_(True), A.to(DEV).requires_grad_(True)
    gtnd, Rd = gtn.to(DEV), R.to(DEV)

    def normal():
        loss = NormalLoss.apply(nraw, J, gtnd, Rd, None, False, bd, rd, cd)
        return (loss,) + torch.autograd.grad(loss, [nraw, J])
    loss, gn, gJ = _twice(normal)
    a64, J64 = nraw0.double().requires_grad_(True), A.double().requires_grad_(True)
    per, cnt, aux = ref.normal_rows(a64, J64, gtn[b.clamp(min=0), r, c], R, None, False)
    l64 = ref.frame_mean(per, cnt, b, N)
    want, _, dfn, mag = ref.reduce64(0, per.detach().numpy(), cnt.numpy(), b.numpy(), N)
    assert abs(want - l64.item()) <= 1e-12 * max(1., abs(want))
    _value(f"normal P={P} {kind}", loss, want, mag, extra=ref.C_N * EPS * mag)
    gn64, gJ64 = torch.autograd.grad(l64, [a64, J64])
    scale = cnt * live.double() / torch.as_tensor(dfn).clamp(min=1)[b.clamp(min=0)] / N
    bn, bJ = ref.normal_grad_bounds(aux, scale)
    worst(f"normal P={P} {kind} gnx", rowmax(gn.double().cpu() - gn64), ref.C_N * bn)
    worst(f"normal P={P} {kind} gJ", rowmax(gJ.double().cpu() - gJ64), ref.C_N * bJ)
    off = scale == 0
    if bool(off.any()):
        assert float(gn.cpu()[off].abs().max()) == 0. and float(gJ.cpu()[off].abs().max()) == 0.


@pytest.mark.parametrize("P", RED_ROWS)
def test_mode0_reductions_at_launch_edges(P):
    """Colour and normal terms with N = 3 at the row counts of the plain-mean test."""
    check_color_and_normal(P, 3, 'sorted', P)


@pytest.mark.parametrize("kind", ['all_bins', 'empty_bins', 'unsorted', 'masked'])
@pytest.mark.parametrize("P", [100, 6144, 40961])
def test_mode0_frame_logic(P, kind):
    """N = 8 = SR_STEP_MAX_FRAMES: every bin populated, bins 2, 5 and 7 empty, b unsorted, 30% of the rows masked with b = -1 (the
    value is that of the compacted rows, masked rows get exactly zero gradient, the denominators in out[1 + 8 + f] are the unmasked
    counts) -- in one workgroup (100, 6,144) and in several (40,961)."""
    check_color_and_normal(P, 8, kind, 1000 + P)


@pytest.mark.parametrize("N,hw", [(1, 1), (1, 32768), (1, 32769), (8, 262145), (3, 699051), (8, 540 * 540)])
def test_mask_iou_at_launch_edges(N, hw):
    """Mask IoU below, at and above the one-workgroup limit, above the 256-block cap (8 x 262,145 = 2,097,160 elements;
    3 x 699,051 with frame boundaries inside blocks) and at the product's own 8 x 540 x 540."""
    from selfreconcode_amd.step_ops import MaskIoULoss
    g = torch.Generator().manual_seed(N * hw)
    m0 = torch.rand(N, hw, generator=g)
    gt = (torch.rand(N, hw, generator=g) > 0.6).float()
    if hw == 1:
        gt[:] = 1.
    m, gtd = m0.to(DEV).requires_grad_(True), gt.to(DEV)

    def iou():
        loss = MaskIoULoss.apply(m, gtd)
        return loss, torch.autograd.grad(loss * 3., m)[0]
    loss, gm = _twice(iou)
    m64 = m0.double().requires_grad_(True)
    g64 = gt.double()
    num, den = m64 * g64, (m64 + g64 - m64 * g64).abs()
    l64 = (1. - num.sum(1) / den.sum(1)).mean()
    want, _, _, mag = ref.reduce64(2, num.detach().reshape(-1).numpy(), den.detach().reshape(-1).numpy(), np.repeat(np.arange(N), hw), N)
    assert abs(want - l64.item()) <= 1e-12
    _value(f"mask IoU {N}x{hw}", loss, want, mag)
    gw, = torch.autograd.grad(l64 * 3., m64)
    # the gradient is rational in the two frame sums, each within C_R eps of float64: 3 C_R eps relative, and the row's own few eps
    worst(f"mask IoU {N}x{hw} grad", (gm.double().cpu() - gw).abs(), 4 * ref.C_R * EPS * gw.abs().amax(1, keepdim=True))
