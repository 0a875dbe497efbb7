"""The skin-fit kernels (csrc/skinfit.hip, selfreconcode_amd/skinfit_ops.py) against the float64 restatement of
tests/_skinfit_ref.py.  Bounds, written before any run:

  * accumulate: |dH_ij| <= (T + 64) 2^-52 S2, S2 = sum_t (max_k |A q| + |y - trans|)^2 -- the accumulated rounding of T double sums of
    ~30-operation terms (ref.h_bound); the same between the fused and the composed path; equal bits between two runs.
  * solve, on the restatement's own H (equal input bits): objective <= (1 + 1e-9) x the restatement's optimum.
  * solve, on the H the kernel accumulated: supports equal the restatement's wherever its best and second-best supports are further
    apart than that bound carries through the objective (ref.near_ties; at most 2 % of the vertices are left out, which
    tests/test_gltf_cpu.py checks for these seeds in float64 alone); the weights there differ by at most 2^-23 (float32 storage, the
    largest weight takes the rounding residue) + 8 delta / lambda: the minimiser on a support is (H_SS + lambda I)^-1 applied to
    data of size lambda, so an error delta on H moves it by about delta / lambda; 8 covers the C entries of a row."""
import numpy as np
import pytest
import torch

import _skinfit_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(p):
    return {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}


def _accumulate(so, g, method="fused", splits=None):
    T, V = g['q'].shape[:2]
    H = so.new_normal_matrix(V, DEV)
    at = 0
    for n in splits or [T]:
        sl = slice(at, at + n)
        so.accumulate(H, g['q'][sl], g['y'][sl], g['A'][sl], g['trans'][sl], g['cands'], method)
        at += n
    assert at == T
    return H


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_accumulate_against_the_restatement(V):
    from selfreconcode_amd import skinfit_ops as so
    assert so.SLAB == 16 and so.TRI == ref.TRI and so.MAX_CANDS == 8
    worst = 0.
    for T in (1, 2, 7, so.SLAB + 1):                                            # the last crosses the kernel's frame slab by one
        for C in (1, 3, 8):
            p = ref.random_problem(1000 * V + 10 * T + C, V, T, C)
            want, S2 = ref.accumulate_ref(p['q'], p['y'], p['A'], p['trans'], p['cands'])
            bound = ref.h_bound(T, S2)[None, :]
            g = _gpu(p)
            H = _accumulate(so, g)
            E = C * (C + 1) // 2
            assert not H[E:].any()                                              # rows past the triangle are not written
            err = np.abs(H.cpu().numpy() - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (T, C, float((err / bound).max()))
            assert torch.equal(_accumulate(so, g), H)                           # two runs: equal bits
            composed = _accumulate(so, g, "composed")
            assert (np.abs(composed.cpu().numpy() - H.cpu().numpy()) <= bound).all(), (T, C)
            if T > 1:                                                           # batches of one, and of several
                for splits in ([1] * T, [T // 2, T - T // 2]):
                    again = _accumulate(so, g, splits=splits)
                    assert (np.abs(again.cpu().numpy() - want) <= bound).all(), (T, C, splits)
            # the transforms as [T,24,4,4] are the same call
            A44 = torch.cat([g['A'].view(T, 24, 3, 4), torch.tensor([0., 0., 0., 1.], device=DEV).expand(T, 24, 1, 4)], 2)
            assert torch.equal(so.accumulate(so.new_normal_matrix(V, DEV), g['q'], g['y'], A44, g['trans'], g['cands']), H)
    print("accumulate, V = %d: largest error / bound %.3g" % (V, worst))


@pytest.mark.parametrize("V,T,C,K,seed", ref.SOLVE_CASES)
def test_solve_against_the_restatement(V, T, C, K, seed):
    from selfreconcode_amd import skinfit_ops as so
    p = ref.random_problem(seed, V, T, C)
    g = _gpu(p)
    want_H, S2 = ref.accumulate_ref(p['q'], p['y'], p['A'], p['trans'], p['cands'])
    want = ref.solve_ref(want_H, p['xbar'], K)
    xbar = torch.from_numpy(np.ascontiguousarray(p['xbar'].T)).to(DEV)
    # (1) equal input bits: the objective
    same = so.solve(torch.from_numpy(want_H).to(DEV), xbar, g['cands'], K)
    ratio = same['objective'].cpu().numpy() / want['objective']
    print("solve: largest objective / optimum - 1 = %.3g" % (ratio.max() - 1.))
    assert (same['objective'].cpu().numpy() <= (1. + 1e-9) * want['objective']).all()
    assert np.allclose(same['lambda'].cpu().numpy(), want['lambda'], rtol=1e-14, atol=0.)
    # (2) the kernel's own H: supports and weights away from near-ties
    H = _accumulate(so, g)
    out = so.solve(H, xbar, g['cands'], K)
    delta = ref.h_bound(T, S2)
    tie = ref.near_ties(want, delta)
    assert tie.mean() <= ref.NEAR_TIE_CAP
    mask, joints, weights = out['mask'].cpu().numpy(), out['joints'].cpu().numpy(), out['weights'].cpu().numpy()
    assert np.array_equal(mask[~tie], want['mask'][~tie])
    x = so.scatter_weights(out['joints'], out['weights'], g['cands']).cpu().numpy().T
    tol = 2. ** -23 + 8. * delta / want['lambda']
    err = np.abs(x - want['x']).max(1)
    print("solve: %d near ties of %d; largest weight error %.3g (allowed there %.3g)" % (tie.sum(), V, err[~tie].max(), tol[~tie][err[~tie].argmax()]))
    assert (err[~tie] <= tol[~tie]).all()
    # the layout: chosen candidates in ascending order, then joint 0 with weight 0; float32 sums within 2 ulp of 1; at most K non-zeros
    assert joints.dtype == np.int32 and weights.dtype == np.float32 and joints.shape == weights.shape == (V, K)
    count = np.array([bin(int(m)).count("1") for m in mask])
    assert (count >= 1).all() and (count <= K).all()
    for v in range(V):
        chosen = [k for k in range(C) if (mask[v] >> k) & 1]
        named = np.where(weights[v, :len(chosen)] > 0., p['cands'][v, chosen], 0)       # (a weight that rounds to 0 names joint 0)
        assert joints[v, :len(chosen)].tolist() == named.tolist() and not joints[v, len(chosen):].any() and not weights[v, len(chosen):].any()
    assert (weights >= 0.).all()
    total = np.zeros(V, np.float32)
    for k in range(K):
        total = total + weights[:, k]                                           # float32, in slot order
    assert (np.abs(total.astype(np.float64) - 1.) <= 2. * 2. ** -23).all()
    # two runs: equal bits; the composed path: the same supports away from near-ties, the same objective
    again = so.solve(H, xbar, g['cands'], K)
    assert all(torch.equal(again[k], out[k]) for k in out)
    composed = so.solve(H, xbar, g['cands'], K, method="composed")
    assert np.array_equal(composed['mask'].cpu().numpy()[~tie], mask[~tie])
    assert np.allclose(composed['objective'].cpu().numpy(), out['objective'].cpu().numpy(), rtol=1e-9, atol=0.)
    assert (np.abs(composed['weights'].cpu().numpy() - weights)[~tie] <= tol[~tie, None]).all()
    # never worse than the naive weights (the prior's K largest, renormalised): their support lies inside the candidates (1e-12: the
    # two objectives are evaluated by different sums in double)
    naive = torch.from_numpy(np.ascontiguousarray(ref.top_k(p['xbar'], K)[0].T)).to(DEV)
    assert bool((out['objective'] <= so.objective_of(H, xbar, out['lambda'], naive) * (1. + 1e-12)).all())


def test_solve_special_cases():
    from selfreconcode_amd import skinfit_ops as so
    V, T, C, K = 70, 5, 8, 4
    p = ref.random_problem(77, V, T, C)
    # exact recovery: data made by weights with at most K non-zeros, and the prior on them
    true = ref.top_k(p['xbar'], 3)[0]
    Ac = p['A'].astype(np.float64).reshape(T, 24, 3, 4)[np.arange(T)[:, None, None], p['cands'][None]]
    Aq = (Ac[..., :3] * p['q'].astype(np.float64)[:, :, None, None, :]).sum(-1) + Ac[..., 3]
    p['y'] = ((true[None, :, :, None] * Aq).sum(2) + p['trans'][:, None, :]).astype(np.float32)
    g = _gpu(p)
    H = _accumulate(so, g)
    prior = torch.from_numpy(np.ascontiguousarray(true.T)).to(DEV)
    back = so.solve(H, prior, g['cands'], K)
    x = so.scatter_weights(back['joints'], back['weights'], g['cands']).cpu().numpy().T
    print("exact recovery: largest weight error %.3g" % np.abs(x - true).max())
    assert np.abs(x - true).max() <= 1e-6
    # H = 0 (a rigid or one-frame capture): the prior's K largest carry the weights; with K = C the prior itself
    xbar = torch.from_numpy(np.ascontiguousarray(p['xbar'].T)).to(DEV)
    zero = so.new_normal_matrix(V, DEV)
    flat = so.solve(zero, xbar, g['cands'], K)
    chosen = ref.top_k(p['xbar'], K)[1]
    want_mask = (chosen.astype(np.int64) << np.arange(C)[None, :]).sum(1)
    assert np.array_equal(flat['mask'].cpu().numpy(), want_mask)
    want = ref.solve_ref(np.zeros((ref.TRI, V)), p['xbar'], K)
    assert np.abs(so.scatter_weights(flat['joints'], flat['weights'], g['cands']).cpu().numpy().T - want['x']).max() <= 2. ** -23
    full = so.solve(zero, xbar, g['cands'], C)
    assert np.abs(so.scatter_weights(full['joints'], full['weights'], g['cands']).cpu().numpy().T - p['xbar']).max() <= 2. ** -23
    # a NaN input vertex: the prior's K largest, renormalised, a NaN objective, and no other vertex changes
    g = _gpu(ref.random_problem(78, V, T, C))
    clean = so.solve(_accumulate(so, g), xbar, g['cands'], K)
    g['q'][2, 5, 1] = float('nan')
    Hn = _accumulate(so, g)
    assert bool(torch.isnan(Hn[:, 5]).any()) and bool(torch.isfinite(Hn[:, :5]).all()) and bool(torch.isfinite(Hn[:, 6:]).all())
    for method in so.METHODS:
        out = so.solve(Hn, xbar, g['cands'], K, method=method)
        assert bool(torch.isnan(out['objective'][5])) and int(out['mask'][5]) == int(want_mask[5]), method
        got = so.scatter_weights(out['joints'], out['weights'], g['cands']).cpu().numpy().T[5]
        assert np.abs(got - ref.top_k(p['xbar'], K)[0][5]).max() <= 2. ** -23, method
        keep = torch.arange(V, device=DEV) != 5
        if method == "fused":
            assert all(torch.equal(out[k][keep], clean[k][keep]) for k in out)
        assert bool(torch.isfinite(out['objective'][keep]).all())


def test_bad_arguments_by_name():
    from selfreconcode_amd import _lib, skinfit_ops as so
    V, T, C, K = 3, 2, 4, 2
    g = _gpu(ref.random_problem(1, V, T, C))
    H = so.new_normal_matrix(V, DEV)
    xbar = torch.full((C, V), 1. / C, dtype=torch.float64, device=DEV)
    joints = torch.empty((V, K), dtype=torch.int32, device=DEV)
    weights = torch.empty((V, K), dtype=torch.float32, device=DEV)
    objective = torch.empty((V,), dtype=torch.float64, device=DEV)
    ptr = lambda t: t.data_ptr()
    acc = dict(q=ptr(g['q']), y=ptr(g['y']), A=ptr(g['A']), trans=ptr(g['trans']), T=T, V=V, cands=ptr(g['cands']), C=C, H=ptr(H), stream=0)
    sol = dict(H=ptr(H), xbar=ptr(xbar), cands=ptr(g['cands']), V=V, C=C, K=K, reg=1e-6, floor=1e-24, joints=ptr(joints), weights=ptr(weights),
               objective=ptr(objective), mask=0, lam=0, stream=0)
    torch.cuda.synchronize()
    assert _lib.raw("sr_skinfit_accumulate")(*acc.values()) == 0 and _lib.raw("sr_skinfit_solve")(*sol.values()) == 0     # (mask, lambda: optional)
    torch.cuda.synchronize()
    bad_acc = [dict(q=0), dict(y=0), dict(A=0), dict(trans=0), dict(cands=0), dict(H=0), dict(T=0), dict(T=-1), dict(V=0), dict(V=2 ** 31),
               dict(C=0), dict(C=9)]
    for change in bad_acc:
        assert _lib.raw("sr_skinfit_accumulate")(*{**acc, **change}.values()) == _lib.SR_EINVAL, change
    bad_sol = [dict(H=0), dict(xbar=0), dict(cands=0), dict(joints=0), dict(weights=0), dict(objective=0), dict(V=0), dict(V=2 ** 31), dict(C=0),
               dict(C=9), dict(K=0), dict(K=C + 1), dict(reg=-1.), dict(reg=float('nan')), dict(floor=0.), dict(floor=float('inf'))]
    for change in bad_sol:
        assert _lib.raw("sr_skinfit_solve")(*{**sol, **change}.values()) == _lib.SR_EINVAL, change
    with pytest.raises(_lib.SrError, match="SR_EINVAL"):
        _lib.call("sr_skinfit_solve", *{**sol, 'K': 0}.values())
    # the Python layer names what is wrong before any launch
    with pytest.raises(ValueError, match=r"K in \[1, C = 4\]"):
        so.solve(H, xbar, g['cands'], 5)
    with pytest.raises(ValueError, match="method must be one of"):
        so.solve(H, xbar, g['cands'], 2, method="greedy")
    with pytest.raises(ValueError, match=r"C in \[1, 8\]"):
        so.candidates(torch.rand(4, 24, device=DEV), 9)
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        so.accumulate(H.cpu(), g['q'], g['y'], g['A'], g['trans'], g['cands'])


def test_candidates_are_the_largest_mean_weights_with_stable_ties():
    from selfreconcode_amd import skinfit_ops as so
    w = torch.zeros((3, 24), device=DEV)
    w[0, [3, 7, 20]] = torch.tensor([0.5, 0.3, 0.2], device=DEV)
    w[1, [5, 2, 9]] = torch.tensor([0.4, 0.4, 0.2], device=DEV)                # a tie: the lower joint first
    w[2, 11] = 1.
    cands, xbar = so.candidates(w, 4)
    assert cands.dtype == torch.int32 and cands.tolist() == [[3, 7, 20, 0], [2, 5, 9, 0], [11, 0, 1, 2]]
    assert xbar.shape == (4, 3) and xbar.dtype == torch.float64
    assert torch.allclose(xbar.t(), torch.tensor([[0.5, 0.3, 0.2, 0.], [0.4, 0.4, 0.2, 0.], [1., 0., 0., 0.]], dtype=torch.float64, device=DEV), atol=1e-7)
