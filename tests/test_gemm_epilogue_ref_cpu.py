"""CPU-side proof that tests/test_gemm_epilogue_gpu.py can be trusted, and that it can fail (no GPU needed):

  * oracle/gemm_epilogue_ref.py::nt_ref is tied to torch's own derivative rules (forward-mode rows = jvp, SR_EPI_BWD = the
    vector-Jacobian product of that forward map), so it is not merely the kernel's formula restated;
  * the inputs of every case reach the branches of the Softplus device functions (region shares) and the ReLU mask is small;
  * every deliberately wrong variant of the epilogue exceeds the bound the GPU test applies, in every case it applies to;
  * the case table reaches every tile shape / K-loop variant / epilogue the dispatcher can choose (the tile choice is asked
    from the library: sr_mlp_gemm_nt_tile needs no device).
The case table, the bound and the variants live in the oracle module: the GPU file runs the very same cases."""
import ctypes
import functools
import pytest
import torch
from oracle import gemm_epilogue_ref as R

# device-function constants of the Softplus epilogues: measured on the MI355X, see profiles/gemm_epilogue_bounds.md
R_EPI, A_EPI = R.R_EPI, R.A_EPI


def tile_of(M, ncols):
    from selfreconcode_amd import _lib
    bm, bn = ctypes.c_int32(0), ctypes.c_int32(0)
    assert _lib.raw("sr_mlp_gemm_nt_tile")(M, ncols, ctypes.byref(bm), ctypes.byref(bn)) == 0
    return bm.value, bn.value


def coverage_problems(cases, tile):
    """-> list of what the case table misses (empty = complete).  Shared with the GPU file, which asks the library it runs."""
    seen, triples, g4 = {}, {}, {}
    for c in cases:
        bm, bn = tile(c.M, c.N + c.naux_fwd)
        kinds = R.tile_kinds(c, bm, bn)
        inner, edge = "interior" in kinds, bool(kinds - {"interior"})
        seen.setdefault(((bm, bn), c.K % 32 != 0), set()).update(kinds)
        t = triples.setdefault((c.mode, c.act, c.group), [False, False])
        t[0], t[1] = t[0] or inner, t[1] or edge
        if c.group == 4 and c.act == R.ACT_SOFTPLUS100:
            g4.setdefault((bm, bn), set()).add(c.mode)
    miss = []
    for shape in R.TILES:
        for ktail in (False, True):
            kinds = seen.get((shape, ktail), set())
            need = {"interior", "row", "col", "corner"} if shape[1] > 32 else {"interior", "row", "col"}
            if not need <= kinds:
                miss.append(("tile kinds", shape, ktail, sorted(need - kinds)))
        if g4.get(shape, set()) != {R.EPI_FWD, R.EPI_BWD}:
            miss.append(("group 4 softplus in both modes", shape))
    for tr in R.TRIPLES:
        if triples.get(tr) != [True, True]:
            miss.append(("triple on interior and edge tiles", tr, triples.get(tr)))
    return miss


def test_case_table_covers_every_tile_shape_and_epilogue():
    assert not coverage_problems(R.CASES, tile_of)
    assert any(c.mode == R.EPI_BWD and c.aux_scale != c.out_scale for c in R.CASES)
    assert any(c.mode == R.EPI_FWD and c.N == 473 and c.naux_fwd == 39 and c.K == 512 for c in R.CASES)
    for kind in ("N", "last", "interior", "zero"):          # the four nact_bwd placements
        assert any(c.mode == R.EPI_BWD and {"N": c.nact_bwd == c.N, "zero": c.nact_bwd == 0, "interior": c.nact_bwd == 473 and c.N == 512,
                                           "last": 0 < c.N - c.nact_bwd < 32}[kind] for c in R.CASES), kind
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)
    # chain cases: the live counts of the issue, one- and two-problem layers
    lives = {(cc.probs[0].group, cc.live * cc.probs[0].group) for cc in R.CHAIN_CASES}
    assert {(1, 0), (1, 1), (1, 63), (1, 64), (1, 65), (4, 4), (2, 2)} <= lives and any(r > 3000 for _, r in lives)
    assert {len(cc.probs) for cc in R.CHAIN_CASES} == {1, 2} and all(cc.cap > cc.live for cc in R.CHAIN_CASES)


def test_tile_query_matches_the_documented_cost_model():
    """The query is the launcher's own choice; pin the shapes the header and the kernel comments name."""
    assert tile_of(6144, 512) == (64, 64) and tile_of(6208, 512) == (128, 128) and tile_of(2100, 512) == (64, 128)
    assert tile_of(5000, 3) == (32, 32) and tile_of(10000, 3) == (64, 32) and tile_of(60000, 32) == (256, 32)
    assert tile_of(200, 512) == (64, 64) and tile_of(262144, 512) == (128, 128)


# ------------------------------------------------------------------------------------------------ nt_ref against torch's rules
def _torch_act(z, act):
    if act == R.ACT_SOFTPLUS100:
        return torch.nn.functional.softplus(z, beta=100, threshold=20)
    return torch.relu(z) if act == R.ACT_RELU else z


TIE_CASES = [c for c in R.CASES if c.M <= 3000]


@pytest.mark.parametrize("case", TIE_CASES, ids=[c.name for c in TIE_CASES])
def test_nt_ref_is_torch_jvp_and_vjp(case):
    inp = R.make_inputs(case)
    ref = R.reference(case, inp)
    g, S, N = case.group, case.M // case.group, case.N
    if case.mode == R.EPI_FWD:
        v = ref.acc.reshape(S, g, N)
        f = lambda z: case.out_scale * _torch_act(z + inp["bias"].double(), case.act)
        want = [f(v[:, 0])]
        for t in range(1, g):                                # tangents carry no bias: they are directions of the accumulator
            want.append(torch.autograd.functional.jvp(f, v[:, 0], v[:, t])[1])
        want = torch.stack(want, 1).reshape(case.M, N)
        if case.naux_fwd:
            want = torch.cat([want, inp["aux"][:, :case.naux_fwd].double() * case.out_scale], 1)
        torch.testing.assert_close(ref.C, want, rtol=1e-12, atol=1e-300)
        return
    # SR_EPI_BWD.  Forward map of a sample: (z, z_t) -> (s act(z), s act'(z) z_t); its VJP with the accumulator as cotangent, at the
    # pre-activations the stored values came from.  Those are recovered from the float32 stored values themselves (so that nt_ref and
    # torch see the same point): act' = stored factor, z from the inverse of softplus; tangents z_t = aux_t / (s act').
    n, s = min(case.nact_bwd, N), case.aux_scale
    torch.testing.assert_close(ref.C[:, n:], ref.acc[:, n:] * case.out_scale, rtol=1e-12, atol=1e-300)
    if n == 0:
        return
    sv = inp["aux"][:, :n].double().reshape(S, g, n)
    cot = ref.acc[:, :n].reshape(S, g, n)
    if case.act == R.ACT_SOFTPLUS100:
        x = 100.0 * sv[:, 0] / s
        z = torch.where(x > 20.0, x, torch.log(torch.expm1(x.clamp(max=21.0)))) / 100.0
    else:
        z = sv[:, 0] / s if case.act == R.ACT_NONE else torch.where(sv[:, 0] > 0, sv[:, 0] / s, -torch.ones_like(sv[:, 0]))
    z = z.clone().requires_grad_(True)
    zt = []
    with torch.enable_grad():
        a = _torch_act(z, case.act)
        d = torch.autograd.grad(a.sum(), z, create_graph=True)[0]
        for t in range(1, g):
            zt.append((sv[:, t] / (s * d.detach().clamp(min=1e-300))).requires_grad_(True))
        out = s * a * cot[:, 0]
        for t in range(1, g):
            out = out + s * d * zt[t - 1] * cot[:, t]
        grads = torch.autograd.grad(out.sum(), [z] + zt)
    want = torch.stack(grads, 1).reshape(case.M, n)
    got = ref.C[:, :n]
    if case.act != R.ACT_SOFTPLUS100:
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-300)
        return
    # Softplus: the identities act' = 1 - e^{-x}, act''/act' = 100 e^{-x} are exact below the threshold.  Above it torch's rule is
    # act' = 1, act'' = 0 where the identity gives 1 - e^{-x} and 100 e^{-x} with x > 20: 100 e^{-20} = 2.1e-7 times the cross term
    # and e^{-20} = 2.1e-9 times the direct term.  Stated, not hidden in a tolerance.  Below the threshold the recovery of z from the
    # stored value (log of expm1) costs a few roundings amplified by 1 / act' <= e^{-100 z} + 1 in z_t -> 1e-9 relative.
    above = (100.0 * z.detach() > 20.0)[:, None, :].expand(S, g, n).reshape(case.M, n)
    cross = sum((sv[:, t] * cot[:, t]).abs() for t in range(1, g)) if g > 1 else torch.zeros(S, n, dtype=torch.float64)
    slack = torch.zeros(S, g, n, dtype=torch.float64)
    slack[:, 0] = 2.1e-7 * cross
    slack = slack.reshape(case.M, n) + 2.1e-9 * s * ref.acc[:, :n].abs()
    err = (got - want).abs()
    assert (err[above] <= slack[above] * (1 + 1e-9) + 1e-300).all()
    tol = 1e-9 * (want.abs() + (s * cot.abs()).reshape(case.M, n) + torch.stack([100 * cross] + [torch.zeros_like(cross)] * (g - 1), 1).reshape(case.M, n)) + 1e-300
    assert (err[~above] <= tol[~above]).all(), (err[~above] / tol[~above]).max()


def test_sensitivities_match_finite_differences():
    case = next(c for c in R.CASES if c.mode == R.EPI_BWD and c.act == R.ACT_SOFTPLUS100 and c.group == 4 and c.M < 200 and c.nact_bwd > 20)
    inp = R.make_inputs(case)
    ref = R.reference(case, inp)
    A = inp["A"].double()
    h = 1e-6
    for j in range(case.group):
        dacc = torch.zeros_like(ref.acc)
        dacc[j::case.group] = h
        Cp = R._epilogue(ref.acc + dacc, None, case.group, case.act, case.mode, case.out_scale, inp["aux"].double(), 0, case.nact_bwd, case.aux_scale)
        torch.testing.assert_close((Cp - ref.C) / h, ref.sens_acc[j], rtol=1e-6, atol=1e-6)       # (C is linear in acc)
    assert A.shape[0] == case.M and ref.sens_aux is not None and ref.sens_aux.abs().max() > 0


def test_tn_ref_sums_primal_rows_only():
    Z = torch.arange(24, dtype=torch.float32).reshape(8, 3)
    A = torch.ones(8, 2)
    dW, db = R.tn_ref(Z, A, 4)
    assert torch.equal(db, (Z[0] + Z[4]).double()) and torch.equal(dW, Z.double().sum(0)[:, None].expand(3, 2))
    dW2, db2 = R.tn_ref(Z, A, 4, dW0=torch.ones(3, 2), db0=torch.ones(3), accumulate=True)
    assert torch.equal(dW2, dW + 1) and torch.equal(db2, db + 1)
    dW0, db0 = R.tn_ref(Z[:0], A[:0], 2)
    assert dW0.abs().sum() == 0 and db0.abs().sum() == 0


# ------------------------------------------------------------------------------------------------ inputs, variants
@functools.lru_cache(maxsize=None)
def _variants_caught():
    """One pass over the table: region shares, mask share and the wrong variants per case (the float64 reference is built once)."""
    shares, masks, report = {}, {}, {}
    for case in R.CASES:
        inp = R.make_inputs(case)
        ref = R.reference(case, inp)
        bm, _ = tile_of(case.M, case.N + case.naux_fwd)
        keep = R.relu_mask(case, ref, inp)
        masks[case.name] = 1.0 - keep.double().mean().item()
        if case.act == R.ACT_RELU and case.mode == R.EPI_FWD:
            z = ref.acc[::case.group] + inp["bias"].double()
            shares[case.name] = [(z > 0).double().mean().item(), (z < 0).double().mean().item()]
        if case.act == R.ACT_SOFTPLUS100 and (case.mode == R.EPI_FWD or case.nact_bwd > 0):
            t = R.preactivation_t(case, ref, inp)
            sh = [(t > 20).double().mean().item(), (t < -6.9).double().mean().item(), (t.abs() < 1).double().mean().item()]
            if case.mode == R.EPI_BWD:
                sh.append((100.0 * inp["aux"][::case.group, :case.nact_bwd].double() / case.aux_scale < 1e-3).double().mean().item())
            shares[case.name] = sh
        bnd = R.case_bound(case, inp, ref, R_EPI, A_EPI)
        for name in R.MUTATIONS:
            m = R.mutant(case, inp, ref, name, bm)
            if m is None:
                continue
            C, affected = m
            affected = affected & keep
            over = ((C - ref.C).abs() > bnd) & affected
            report[(case.name, name)] = over.sum().item() / max(affected.sum().item(), 1)
    return shares, masks, report


def test_inputs_reach_every_branch_of_the_device_functions():
    shares, masks, _ = _variants_caught()
    for c in R.CASES:
        if c.act == R.ACT_SOFTPLUS100 and (c.mode == R.EPI_FWD or c.nact_bwd > 0):
            assert min(shares[c.name]) >= 0.02, (c.name, shares[c.name])      # threshold, series, centre (, stored-series) shares
        if c.act == R.ACT_RELU and c.mode == R.EPI_FWD:
            assert min(shares[c.name]) >= 0.20, (c.name, shares[c.name])
        assert masks[c.name] <= 1e-3, (c.name, masks[c.name])


@pytest.mark.parametrize("name", R.MUTATIONS)
def test_every_wrong_variant_exceeds_the_bound(name):
    _, _, report = _variants_caught()
    rows = {k[0]: v for k, v in report.items() if k[1] == name}
    assert rows, f"no case can see the variant {name}"
    missed = {k: v for k, v in rows.items() if v < 0.01}
    assert not missed, (name, missed)


def test_variants_meet_every_path_they_concern():
    """A variant that only some corner of the table can see would be a hole: each must be applicable on interior and on edge tiles."""
    _, _, report = _variants_caught()
    by_name = {c.name: c for c in R.CASES}
    for name in R.MUTATIONS:
        kinds = set()
        for (cn, mn) in report:
            if mn == name:
                c = by_name[cn]
                kinds |= R.tile_kinds(c, *tile_of(c.M, c.N + c.naux_fwd))
        need = {"interior"} if name not in ("filler_next_column", "filler_no_out_scale", "nact_plus1") else set()
        assert need <= kinds and kinds - {"interior"}, (name, kinds)
