"""sr_mlp_gemm_nt / sr_mlp_chain launch by launch against the float64 statement of the epilogue contract
(oracle/gemm_epilogue_ref.py): both modes, three activations, groups 1 / 2 / 4, filler columns, the nact_bwd split, both scales,
on every tile shape and K-loop variant the dispatcher can choose, with interior and edge tiles in the same launch.

Every case is ONE launch; the whole of C is compared with the reference under the bound of the oracle module
  sum |dC/dacc| e_acc (+ |dC/daux| |aux| 2^-24) + r_epi |C_ref| + a_epi
(e_acc: the project's bare-GEMM bound; r_epi, a_epi: device-function constants, profiles/gemm_epilogue_bounds.md), and every float
of the allocation outside the logical C must keep the bit pattern it was filled with.  tests/test_gemm_epilogue_ref_cpu.py proves
on the CPU that this bound is missed by every wrong variant of the epilogue it lists, on these very cases."""
import ctypes
import pytest
import torch
from oracle import gemm_epilogue_ref as R
from test_gemm_epilogue_ref_cpu import coverage_problems, tile_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# device-function constants of the Softplus epilogues: measured on the MI355X, see profiles/gemm_epilogue_bounds.md
R_EPI, A_EPI = R.R_EPI, R.A_EPI
GUARD_BITS = 0x7FA5C3E1        # a NaN with a payload nothing computes
GUARD_ROWS = 3


def pad4(n):
    return (n + 3) // 4 * 4


def _padded(t, pitch, rows=None):
    """t [M, w] -> device matrix of row pitch `pitch` whose padding is NaN (every float the kernel may read but must not use)."""
    rows = t.shape[0] if rows is None else rows
    out = torch.full((max(rows, 1), pitch), float("nan"))
    out[:t.shape[0], :t.shape[1]] = t
    return out.to(DEV)


def _guarded_c(rows, ldc):
    """C of `rows` rows with GUARD_ROWS rows in front and behind, every float = GUARD_BITS.  -> (whole allocation as int32, C view)."""
    whole = torch.full(((rows + 2 * GUARD_ROWS), ldc), GUARD_BITS, dtype=torch.int32, device=DEV)
    return whole, whole.view(torch.float32)[GUARD_ROWS:GUARD_ROWS + rows]


def _device_operands(case, inp, rows=None):
    """Row pitches wider than the logical widths, different for every operand.  SR_EPI_BWD: the aux columns >= nact_bwd are not the
    kernel's to use either: NaN.  SR_EPI_FWD: likewise the columns >= naux_fwd."""
    K, N = case.K, case.N
    A = _padded(inp["A"], pad4(K) + 4, rows)
    B = _padded(inp["B"], pad4(K) + 8)
    bias = None if inp["bias"] is None else inp["bias"].to(DEV)
    aux = None
    if inp["aux"] is not None:
        used = case.naux_fwd if case.mode == R.EPI_FWD else min(case.nact_bwd, N)
        aux = _padded(inp["aux"][:, :used], pad4(max(used, 1)) + 12, rows)
    return A, B, bias, aux


def _where(case, bm, bn, r, c):
    """Tile, wave, 32x32 block, quad and row-in-group of element (r, c) for the assertion message."""
    W = case.N + case.naux_fwd
    i, j = r // bm, c // bn
    lr, lc = r % bm, c % bn
    return (f"tile ({i},{j}) of {bm}x{bn} [{'interior' if R.is_interior(case, bm, bn, i, j) else 'edge'}], block row {lr // 32} col {lc // 32}, "
            f"quad {(lr % 32) // 8} half {(lr % 8) // 4}, lane column {lc % 32}, row-in-group {r % case.group}, "
            f"{'filler' if c >= case.N else 'plain' if case.mode == R.EPI_BWD and c >= case.nact_bwd else 'activated'} column of {W}")


def _compare(case, inp, got, whole, rows, ldc, bm, bn):
    """got: C [rows, ldc] (device, float32 view of `whole`).  Value check of the logical C and bit check of everything else."""
    W = case.N + case.naux_fwd
    bits = whole.cpu()
    live = torch.zeros_like(bits, dtype=torch.bool)
    live[GUARD_ROWS:GUARD_ROWS + rows, :W] = True
    touched = (bits != GUARD_BITS) & ~live
    assert not touched.any(), (case.name, "guard floats written at (row, column) relative to C:",
                               [(int(r) - GUARD_ROWS, int(c)) for r, c in touched.nonzero()[:8]])
    if rows == 0:
        return
    ref = R.reference(case, inp)
    bnd = R.case_bound(case, inp, ref, R_EPI, A_EPI)
    keep = R.relu_mask(case, ref, inp)
    C = got[:, :W].cpu().double()
    err = (C - ref.C).abs()
    bad = ~(err <= bnd) & keep                       # (NaN fails)
    worst = (err / bnd.clamp(min=1e-300))[keep].max().item()
    print(f"{case.name}: tile {bm}x{bn}, worst err/bound {worst:.3g}, masked {(~keep).sum().item()}")
    if bad.any():
        idx = bad.nonzero()
        lines = [f"({int(r)},{int(c)}): got {C[r, c].item():.9g} want {ref.C[r, c].item():.9g} bound {bnd[r, c].item():.3g} -- {_where(case, bm, bn, int(r), int(c))}"
                 for r, c in idx[:6]]
        raise AssertionError(f"{case.name}: {len(idx)} of {keep.sum().item()} elements outside the bound "
                             f"(mode {R.MODE_NAME[case.mode]}, act {R.ACT_NAME[case.act]}, group {case.group}, tile {bm}x{bn}, "
                             f"K-tail {case.K % 32 != 0}); rows-in-group hit {sorted(set((idx[:, 0] % case.group).tolist()))}, "
                             f"interior {sum(R.is_interior(case, bm, bn, int(r) // bm, int(c) // bn) for r, c in idx[:2000])} of the first {min(len(idx), 2000)}\n  "
                             + "\n  ".join(lines))


def test_case_table_coverage_with_the_loaded_library():
    """The same assertion as on the CPU, asked from the library these tests launch (a stale build cannot pass by accident)."""
    assert not coverage_problems(R.CASES, tile_of)


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_gemm_nt_epilogue_vs_float64(case):
    from selfreconcode_amd import mlp_engine as me
    assert (me.ACT_NONE, me.ACT_SOFTPLUS100, me.ACT_RELU, me.EPI_FWD, me.EPI_BWD) == (R.ACT_NONE, R.ACT_SOFTPLUS100, R.ACT_RELU, R.EPI_FWD, R.EPI_BWD)
    inp = R.make_inputs(case)
    A, B, bias, aux = _device_operands(case, inp)
    W = case.N + case.naux_fwd
    ldc = pad4(W) + 8
    whole, C = _guarded_c(case.M, ldc)
    bm, bn = tile_of(case.M, W)
    me._gemm_nt(A, A.stride(0), B, B.stride(0), C, ldc, case.M, case.N, case.K, bias, case.group, case.act, case.mode,
                out_scale=case.out_scale, aux=aux, ldaux=0 if aux is None else aux.stride(0), naux_fwd=case.naux_fwd,
                nact_bwd=case.nact_bwd, aux_scale=case.aux_scale)
    torch.cuda.synchronize()
    _compare(case, inp, C, whole, case.M, ldc, bm, bn)


@pytest.mark.parametrize("cc", R.CHAIN_CASES, ids=[c.name for c in R.CHAIN_CASES])
def test_layer_chain_epilogue_vs_float64(cc):
    """The same contract through sr_mlp_chain (64x64 tiles): the row count lives in device memory, the grid is sized for m_cap, rows
    past the live count are not touched.  One layer of one or two problems."""
    from selfreconcode_amd import _lib, mlp_engine as me
    g = cc.probs[0].group
    rows, cap_rows = cc.live * g, cc.cap * g
    live = torch.tensor([cc.live], dtype=torch.int32, device=DEV)
    a = _lib.SrChainArgs()
    a.nlayers, a.nprob[0] = 1, len(cc.probs)
    a.m_dev, a.m_mul, a.m_cap = live.data_ptr(), g, cc.cap
    held = []
    for p, prob in enumerate(cc.probs):
        case = prob._replace(M=rows, seed=prob.seed + 31 * cc.live + p)
        inp = R.make_inputs(case)
        A, B, bias, aux = _device_operands(case, inp, rows=cap_rows)            # rows past the live count: NaN
        W = case.N + case.naux_fwd
        ldc = pad4(W) + 4
        whole, C = _guarded_c(cap_rows, ldc)
        me.set_gemm_args(a.g[0][p], A, B, C, 0, case.N, case.K, bias, g, case.act, case.mode, case.out_scale, aux, case.naux_fwd,
                         case.nact_bwd, case.aux_scale)
        held.append((case, inp, A, B, bias, aux, whole, C, ldc))
    _lib.call("sr_mlp_chain", ctypes.byref(a), _lib.stream_of(live))
    torch.cuda.synchronize()
    for case, inp, A, B, bias, aux, whole, C, ldc in held:
        _compare(case, inp, C[:rows], whole, rows, ldc, 64, 64)
