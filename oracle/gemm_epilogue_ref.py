"""TEST INFRASTRUCTURE -- float64 statement of the layer-GEMM epilogue contract (include/selfrecon_hip.h, the block above
`sr_gemm_args`), the error bound the GPU tests apply to it, the table of cases both test files run, and the deliberately
wrong variants tests/test_gemm_epilogue_ref_cpu.py uses to prove that the bound can be missed.

Written from the header's contract and from the reference network, not from the kernel:
  model/network.py:70      nn.Softplus(beta=100)  (threshold 20: torch's default)
  model/network.py:88-89   x = cat([x, input], 1) / sqrt(2)  -- the skip concat: filler columns, out_scale = 1/sqrt(2)
  model/network.py:91-94   x = lin(x); x = softplus(x)
Rows are tangent-interleaved: a sample owns `group` consecutive rows, its primal followed by group-1 forward tangents.
Pure torch, float64, CPU.  The product never imports this module."""
import collections
import math
import torch

ACT_NONE, ACT_SOFTPLUS100, ACT_RELU = 0, 1, 2
EPI_FWD, EPI_BWD = 0, 1
ACT_NAME = {ACT_NONE: "none", ACT_SOFTPLUS100: "softplus", ACT_RELU: "relu"}
MODE_NAME = {EPI_FWD: "fwd", EPI_BWD: "bwd"}
BETA, THRESHOLD = 100.0, 20.0
U32 = 2.0 ** -24                     # one float32 rounding, relative
# the accumulator bound the project accepts for the bare GEMM (tests/test_mlp_gpu.py::test_gemm_kernels_ragged_shapes_vs_float64)
E_ACC_REL, E_ACC_ABS = 2e-5, 2e-5    # absolute part times max(1, sqrt(K))

NtRef = collections.namedtuple("NtRef", "C acc sens_acc sens_aux")


def f32(x):
    """The value a C float argument carries."""
    return float(torch.tensor(x, dtype=torch.float32).item())


def act_and_derivative(z, act, threshold_at=THRESHOLD):
    """-> (act(z), act'(z)) by torch's rules: Softplus(beta=100, threshold=20) is the identity (derivative 1) where 100 z > 20."""
    if act == ACT_SOFTPLUS100:
        t = BETA * z
        lin = t > threshold_at
        ts = torch.where(lin, torch.zeros_like(t), t)
        return torch.where(lin, z, torch.log1p(torch.exp(ts)) / BETA), torch.where(lin, torch.ones_like(t), torch.sigmoid(ts))
    if act == ACT_RELU:
        return torch.clamp(z, min=0.0), (z > 0).to(z.dtype)
    return z, torch.ones_like(z)


def stored_factors(a, act, aux_scale):
    """Derivative factors from the STORED primal activation a = aux_scale * act(z): -> (act', act''/act').
    Softplus(beta = 100): 1 + e^{100 z} = e^{100 a / aux_scale}  =>  act' = 1 - e^{-x}, act''/act' = 100 e^{-x}, x = 100 a / aux_scale."""
    if act == ACT_SOFTPLUS100:
        x = BETA * a / aux_scale
        return -torch.expm1(-x), BETA * torch.exp(-x)
    if act == ACT_RELU:
        return (a > 0).to(a.dtype), torch.zeros_like(a)
    return torch.ones_like(a), torch.zeros_like(a)


def _epilogue(acc, bias, group, act, mode, out_scale, aux, naux_fwd, nact_bwd, aux_scale, wrong=None):
    """acc [M, N] float64 -> C [M, N (+ naux_fwd)].  `wrong` names one deliberately wrong variant (see MUTATIONS); None = the contract."""
    M, N = acc.shape
    g = group
    if wrong == "group4_for_group2":
        M4 = M - M % 4
        if M4 == 0:
            return _epilogue(acc, bias, g, act, mode, out_scale, aux, naux_fwd, nact_bwd, aux_scale)
        head = _epilogue(acc[:M4], bias, 4, act, mode, out_scale, None if aux is None else aux[:M4], naux_fwd, nact_bwd, aux_scale)
        if M4 == M:
            return head
        tail = _epilogue(acc[M4:], bias, g, act, mode, out_scale, None if aux is None else aux[M4:], naux_fwd, nact_bwd, aux_scale)
        return torch.cat([head, tail], 0)
    S = M // g
    v = acc.reshape(S, g, N)
    src = g - 1 if wrong == "dact_from_last_row" else 0        # the row of a sample the derivative factors are taken from
    if mode == EPI_FWD:
        b = bias if bias is not None else torch.zeros(N, dtype=acc.dtype)
        z = v[:, 0, :] + b
        a, _ = act_and_derivative(z, act, 0.0 if wrong == "threshold_at_zero" else THRESHOLD)
        _, d = act_and_derivative(v[:, src, :] + b, act, 0.0 if wrong == "threshold_at_zero" else THRESHOLD)
        rows = [a * out_scale]
        for t in range(1, g):
            vt = v[:, t, :] + b if wrong == "bias_on_tangents" else v[:, t, :]
            rows.append(d * vt * (1.0 if wrong == "tangents_no_out_scale" else out_scale))
        C = torch.stack(rows, 1).reshape(M, N)
        if naux_fwd > 0:
            off = 1 if wrong == "filler_next_column" else 0
            C = torch.cat([C, aux[:, off:off + naux_fwd] * (1.0 if wrong == "filler_no_out_scale" else out_scale)], 1)
        return C
    if wrong == "scales_swapped":
        out_scale, aux_scale = aux_scale, out_scale
    n = min(max(nact_bwd + {"nact_plus1": 1, "nact_minus1": -1}.get(wrong, 0), 0), N)
    sv = aux[:, :n].reshape(S, g, n)
    d, c2 = stored_factors(sv[:, src, :], act, aux_scale)
    cross = torch.zeros_like(d)
    last = g - 1 if wrong == "cross_missing_last_tangent" else g
    for t in range(1, last):
        cross = cross + sv[:, t, :] * v[:, t, :n]
    if wrong == "no_c2_cross":
        cross = torch.zeros_like(d)
    rows = [d * aux_scale * v[:, 0, :n] + c2 * cross] + [d * aux_scale * v[:, t, :n] for t in range(1, g)]
    return torch.cat([torch.stack(rows, 1).reshape(M, n), acc[:, n:] * out_scale], 1)


def nt_ref(A, B, bias, group, act, mode, out_scale=1.0, aux=None, naux_fwd=0, nact_bwd=0, aux_scale=1.0, sens=True):
    """The contract of sr_mlp_gemm_nt in float64 on the logical widths: A [M, K], B [N, K], bias [N] or None, aux [M, >= naux_fwd]
    (SR_EPI_FWD) or [M, >= nact_bwd] (SR_EPI_BWD) -> NtRef with
      C         [M, N (+ naux_fwd)]
      acc       [M, N] = A B^T
      sens_acc  [group, M, W]: sens_acc[j, r, c] = dC[r, c] / dacc[first row of r's sample + j, c]  (an element depends on the
                accumulator entries of its own sample and column only)
      sens_aux  the same with respect to the stored activations (SR_EPI_BWD, else None)."""
    A, B = A.double(), B.double()
    bias = None if bias is None else bias.double()
    aux = None if aux is None else aux.double()
    M, N = A.shape[0], B.shape[0]
    if mode != EPI_FWD:
        naux_fwd = 0
    acc = A @ B.t()
    if not sens or M == 0:
        return NtRef(_epilogue(acc, bias, group, act, mode, out_scale, aux, naux_fwd, nact_bwd, aux_scale), acc, None, None)
    g, S, W = group, M // group, N + naux_fwd
    accv = acc.clone().requires_grad_(True)
    auxv = aux[:, :min(nact_bwd, N)].clone().requires_grad_(True) if mode == EPI_BWD else aux
    C = _epilogue(accv, bias, g, act, mode, out_scale, auxv, naux_fwd, nact_bwd, aux_scale)
    sa = torch.zeros(g, M, W, dtype=torch.float64)
    sx = torch.zeros(g, M, W, dtype=torch.float64) if mode == EPI_BWD else None
    Cv = C.reshape(S, g, W)
    for i in range(g):                     # the rows i of all samples at once: different samples and columns do not interact
        ins = [accv] + ([auxv] if mode == EPI_BWD and auxv.shape[1] > 0 else [])
        gr = torch.autograd.grad(Cv[:, i, :].sum(), ins, retain_graph=i + 1 < g, allow_unused=True)
        ga = gr[0].reshape(S, g, N)
        for j in range(g):
            sa[j].reshape(S, g, W)[:, i, :N] = ga[:, j, :]
        if len(ins) > 1 and gr[1] is not None:
            gx = gr[1].reshape(S, g, -1)
            for j in range(g):
                sx[j].reshape(S, g, W)[:, i, :gx.shape[2]] = gx[:, j, :]
    return NtRef(C.detach(), acc, sa, sx)


def acc_error(acc, K):
    """What the bare GEMM may be off by, per accumulator entry (the project's own bound, see E_ACC_*)."""
    return E_ACC_REL * acc.abs() + E_ACC_ABS * max(1.0, math.sqrt(K))


def bound(ref, K, group, aux, r_epi, a_epi):
    """Allowed |C - C_ref| per element:  sum_j |dC/dacc_j| e_acc_j  (+ sum_j |dC/daux_j| |aux_j| 2^-24)  +  r_epi |C_ref|  +  a_epi."""
    M, W = ref.C.shape
    g, S, N = group, M // group, ref.acc.shape[1]
    e = torch.zeros(M, W, dtype=torch.float64)
    e[:, :N] = acc_error(ref.acc, K)
    ev = e.reshape(S, g, W)
    out = r_epi * ref.C.abs() + a_epi
    for j in range(g):
        out = out + (ref.sens_acc[j].abs().reshape(S, g, W) * ev[:, j:j + 1, :]).reshape(M, W)
    if ref.sens_aux is not None:
        x = torch.zeros(M, W, dtype=torch.float64)
        n = min(aux.shape[1], W)
        x[:, :n] = aux[:, :n].double().abs() * U32
        xv = x.reshape(S, g, W)
        for j in range(g):
            out = out + (ref.sens_aux[j].abs().reshape(S, g, W) * xv[:, j:j + 1, :]).reshape(M, W)
    return out


def tn_ref(Z, A, group, dW0=None, db0=None, accumulate=False):
    """Weight gradient: dW [N, K] = Z^T A over all rows, db [N] = sum of the primal rows (r % group == 0) of Z; `accumulate`
    adds onto dW0 / db0."""
    Z, A = Z.double(), A.double()
    dW, db = Z.t() @ A, Z[::group].sum(0)
    if accumulate:
        dW, db = dW + dW0.double(), db + db0.double()
    return dW, db


# ------------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "name mode act group M N K naux_fwd nact_bwd out_scale aux_scale seed")
RSQRT2 = f32(1.0 / math.sqrt(2.0))
TILES = ((32, 32), (64, 32), (256, 32), (64, 64), (64, 128), (128, 128))
TRIPLES = [(m, a, g) for m in (EPI_FWD, EPI_BWD) for a in (ACT_NONE, ACT_SOFTPLUS100, ACT_RELU) for g in (1, 2, 4)]
# seeds chosen on the CPU so that every case meets the region shares of tests/test_gemm_epilogue_ref_cpu.py (default: the index)
SEED_OF = {38: 202}


def _case(cases, mode, act, group, M, N, K, naux_fwd=0, nact_bwd=None, out_scale=1.0, aux_scale=1.0):
    M -= M % group
    if mode == EPI_BWD:
        naux_fwd, nact_bwd = 0, N if nact_bwd is None else nact_bwd
    else:
        nact_bwd, aux_scale = 0, 1.0
    name = f"{len(cases):03d}-{MODE_NAME[mode]}-{ACT_NAME[act]}-g{group}-M{M}-N{N}-K{K}" + (f"-fill{naux_fwd}" if naux_fwd else "") + \
        (f"-nact{nact_bwd}" if mode == EPI_BWD else "")
    cases.append(Case(name, mode, act, group, M, N, K, naux_fwd, nact_bwd, f32(out_scale), f32(aux_scale), SEED_OF.get(len(cases), len(cases))))


def _build_cases():
    c = []
    K_ALIGNED, K_RAGGED = (32, 64, 96, 512), (39, 41, 167, 289, 473)
    # 32x32 tiles (ncols <= 32, up to 8192 rows): every triple; N = 32 has interior tiles, N < 32 column-cut ones
    for i, (mode, act, g) in enumerate(TRIPLES):
        M = (31, 32, 32 + g, 100, 1000, 33)[i % 6]
        K = (K_ALIGNED + K_RAGGED)[i % 9]
        if mode == EPI_FWD:
            _case(c, mode, act, g, max(M, 64 + g), 32, K, out_scale=(1.0, RSQRT2)[i % 2])
            _case(c, mode, act, g, M, (31, 20, 3)[i % 3], K, naux_fwd=(0, 12, 5)[i % 3], out_scale=RSQRT2)
        else:
            _case(c, mode, act, g, max(M, 64 + g), 32, K, out_scale=RSQRT2, aux_scale=(0.5, RSQRT2)[i % 2])
            _case(c, mode, act, g, M, (31, 32, 7)[i % 3], K, nact_bwd=(31, 20, 0)[i % 3], out_scale=1.0, aux_scale=RSQRT2)
    for g in (1, 2, 4):                                  # one sample
        _case(c, EPI_FWD, ACT_SOFTPLUS100, g, g, 31, 39)
        _case(c, EPI_BWD, ACT_SOFTPLUS100, g, g, 32, 64, nact_bwd=31, aux_scale=RSQRT2)
    # 64x32 (8193 .. 49152 rows) and 256x32 (above): tile height minus one sample, exactly, plus one sample
    for base, k_al, k_rg in ((129 * 64, 64, 41), (193 * 256, 32, 39)):
        for i, (mode, act, g) in enumerate([(EPI_FWD, ACT_SOFTPLUS100, 4), (EPI_BWD, ACT_SOFTPLUS100, 4), (EPI_FWD, ACT_RELU, 2),
                                            (EPI_BWD, ACT_RELU, 1), (EPI_FWD, ACT_NONE, 1), (EPI_BWD, ACT_NONE, 2)]):
            M = base + (-g, 0, g)[i % 3]
            if mode == EPI_FWD:
                _case(c, mode, act, g, M, 32, (k_al, k_rg)[i % 2], out_scale=RSQRT2)
                _case(c, mode, act, g, M, 17, (k_rg, k_al)[i % 2], naux_fwd=13, out_scale=RSQRT2)
            else:
                _case(c, mode, act, g, M, 32, (k_al, k_rg)[i % 2], out_scale=1.0, aux_scale=RSQRT2)
                _case(c, mode, act, g, M, 30, (k_rg, k_al)[i % 2], nact_bwd=(30, 17, 0)[i % 3], out_scale=RSQRT2, aux_scale=0.5)
    # 64x64: every triple on a launch with interior, row-cut, column-cut and corner tiles
    for i, (mode, act, g) in enumerate(TRIPLES):
        M = (63, 64, 64 + g, 132, 3001, 200)[i % 6] + (0 if i % 6 > 2 else 64)
        K = (K_RAGGED + K_ALIGNED)[i % 9]
        if mode == EPI_FWD:
            fill = (0, 39, 7)[i % 3]
            _case(c, mode, act, g, M, 150 - fill + (0, 42, 3)[i % 3], K, naux_fwd=fill, out_scale=(RSQRT2, 1.0, RSQRT2)[i % 3])
        else:
            _case(c, mode, act, g, M, 150, K, nact_bwd=(150, 140, 100, 0)[i % 4], out_scale=(1.0, RSQRT2)[i % 2], aux_scale=(RSQRT2, 0.5)[i % 2])
    for g in (1, 2, 4):                                  # one sample, wide
        _case(c, EPI_FWD, ACT_SOFTPLUS100, g, g, 150, 167, naux_fwd=39, out_scale=RSQRT2)
        _case(c, EPI_BWD, ACT_SOFTPLUS100, g, g, 189, 96, nact_bwd=150, out_scale=RSQRT2, aux_scale=0.5)
    # 64x128 (257 .. 512 tiles of 64x64: 33 row tiles x 8) and 128x128 (about 6.2k rows at 512 columns; 49 row tiles)
    for base, bm, k_al, k_rg in ((33 * 64, 64, 64, 41), (49 * 128, 128, 32, 39)):
        for i, (mode, act, g) in enumerate([(EPI_FWD, ACT_SOFTPLUS100, 4), (EPI_BWD, ACT_SOFTPLUS100, 4), (EPI_FWD, ACT_RELU, 2),
                                            (EPI_BWD, ACT_SOFTPLUS100, 2), (EPI_FWD, ACT_NONE, 1), (EPI_BWD, ACT_RELU, 1),
                                            (EPI_FWD, ACT_SOFTPLUS100, 1), (EPI_BWD, ACT_NONE, 4)]):
            M = base + (-g, 0, g, 37 * g)[i % 4]
            K = (k_al, k_rg)[(i // 2) % 2]
            if mode == EPI_FWD:
                N, fill = ((473, 39), (500, 0), (490, 6), (512, 0))[i // 2]
                _case(c, mode, act, g, M, N, K, naux_fwd=fill, out_scale=RSQRT2)
            else:
                N, nact = ((512, 473), (500, 500), (512, 0), (512, 512))[i // 2]
                _case(c, mode, act, g, M, N, K, nact_bwd=nact, out_scale=(RSQRT2, 1.0)[i % 2], aux_scale=(RSQRT2, 0.5)[(i // 2) % 2])
    # the project's own layer: 512 -> 473 + 39 filler at K = 512 on 128x128 tiles, and its reverse
    _case(c, EPI_FWD, ACT_SOFTPLUS100, 4, 6276, 473, 512, naux_fwd=39, out_scale=RSQRT2)
    _case(c, EPI_BWD, ACT_SOFTPLUS100, 4, 6276, 512, 512, nact_bwd=473, out_scale=RSQRT2, aux_scale=RSQRT2)
    return c


CASES = _build_cases()

# Layer-chain launches (sr_mlp_chain, 64x64 tiles, row count in device memory): (m_cap samples, live samples, [problems of the layer]);
# a problem is a Case whose M is ignored (rows = live * group).
ChainCase = collections.namedtuple("ChainCase", "name cap live probs")


def _build_chain_cases():
    def P(mode, act, g, N, K, **kw):
        tmp = []
        _case(tmp, mode, act, g, g, N, K, **kw)
        return tmp[0]
    out = []
    layers = [
        (1, [P(EPI_FWD, ACT_SOFTPLUS100, 1, 111, 39, naux_fwd=39, out_scale=RSQRT2)]),
        (1, [P(EPI_BWD, ACT_SOFTPLUS100, 1, 150, 64, nact_bwd=111, out_scale=RSQRT2, aux_scale=RSQRT2),
             P(EPI_FWD, ACT_RELU, 1, 70, 167)]),
        (4, [P(EPI_FWD, ACT_SOFTPLUS100, 4, 128, 96), P(EPI_BWD, ACT_SOFTPLUS100, 4, 128, 41, nact_bwd=128, aux_scale=0.5)]),
        (2, [P(EPI_BWD, ACT_RELU, 2, 130, 32, nact_bwd=64, out_scale=0.5, aux_scale=RSQRT2), P(EPI_FWD, ACT_NONE, 2, 3, 289)]),
    ]
    lives = {1: (0, 1, 63, 64, 65, 3001), 4: (0, 1, 16, 777), 2: (1, 32, 1501)}
    for g, probs in layers:
        for live in lives[g]:
            cap = max(live + 7, 100) if live < 1000 else live + 333
            out.append(ChainCase(f"chain{len(out):02d}-g{g}-live{live}-cap{cap}-" + "+".join(p.name[4:] for p in probs), cap, live, probs))
    return out


CHAIN_CASES = _build_chain_cases()


def make_inputs(case, M=None):
    """Float32 CPU inputs of a case (logical widths): A [M, K], B [N, K], bias [N] or None, aux or None.  Pre-activations of
    the Softplus cases are spread over |100 z| up to about 50 (standard deviation 15); the others have unit scale.
    SR_EPI_FWD: aux [M, naux_fwd + 1] (one column more than the kernel may read: the filler_next_column variant reads it).
    SR_EPI_BWD: aux [M, N] = stored activations of a forward pass of the same layout in columns < nact_bwd (primal rows
    aux_scale * act(z), tangent rows aux_scale * act'(z) * z_t), arbitrary values beyond."""
    M = case.M if M is None else M
    gen = torch.Generator().manual_seed(1000003 * (case.seed + 1) + 17)
    N, K, g = case.N, case.K, case.group
    soft = case.act == ACT_SOFTPLUS100
    A = torch.randn(M, K, generator=gen)
    if case.mode == EPI_FWD:
        B = torch.randn(N, K, generator=gen) * ((0.14 if soft else 1.0) / math.sqrt(K))
        bias = torch.randn(N, generator=gen) * (0.05 if soft else 0.5)
        aux = torch.randn(M, case.naux_fwd + 1, generator=gen) if case.naux_fwd else None
        return {"A": A, "B": B, "bias": bias, "aux": aux}
    B = torch.randn(N, K, generator=gen) * (0.5 / math.sqrt(K))
    z = torch.randn(M // g, 1, N, generator=gen, dtype=torch.float64) * (0.15 if soft else 1.0)
    zt = torch.randn(M // g, g - 1, N, generator=gen, dtype=torch.float64)
    a, d = act_and_derivative(z, case.act)
    aux = (torch.cat([a, d * zt], 1) * case.aux_scale).reshape(M, N).float()
    if case.nact_bwd < N:
        aux[:, case.nact_bwd:] = torch.randn(M, N - case.nact_bwd, generator=gen)
    return {"A": A, "B": B, "bias": None, "aux": aux}


def reference(case, inp, sens=True):
    return nt_ref(inp["A"], inp["B"], inp["bias"], case.group, case.act, case.mode, case.out_scale, inp["aux"], case.naux_fwd,
                  case.nact_bwd, case.aux_scale, sens=sens)


def epi_constants(case, r_epi, a_epi):
    """Softplus cases: the measured device-function constants; others: one float32 rounding of the result."""
    return (r_epi, a_epi) if case.act == ACT_SOFTPLUS100 else (U32, 0.0)


def case_bound(case, inp, ref, r_epi, a_epi):
    r, a = epi_constants(case, r_epi, a_epi)
    return bound(ref, case.K, case.group, inp["aux"], r, a)


def relu_mask(case, ref, inp):
    """True where the comparison holds.  SR_EPI_FWD ReLU: a pre-activation within the accumulator bound of zero may take either
    branch on the device; such elements and the tangent rows of their sample are left out (computed from the reference alone)."""
    M, W = ref.C.shape
    keep = torch.ones(M, W, dtype=torch.bool)
    if case.act != ACT_RELU or case.mode != EPI_FWD or M == 0:
        return keep
    g, S, N = case.group, M // case.group, case.N
    z = ref.acc.reshape(S, g, N)[:, 0, :] + inp["bias"].double()
    near = z.abs() <= acc_error(ref.acc, case.K).reshape(S, g, N)[:, 0, :]
    keep.reshape(S, g, W)[:, :, :N] = ~near[:, None, :]
    return keep


def preactivation_t(case, ref, inp):
    """100 z of the activated primal elements (Softplus cases), from the reference alone: SR_EPI_FWD z = acc + bias;
    SR_EPI_BWD from the stored activation, 100 z = log(expm1(100 a / aux_scale))."""
    g, N = case.group, case.N
    if case.mode == EPI_FWD:
        return BETA * (ref.acc[::g] + inp["bias"].double()).reshape(-1)
    x = BETA * inp["aux"][::g, :case.nact_bwd].double().reshape(-1) / case.aux_scale
    return torch.where(x > THRESHOLD, x, torch.log(torch.expm1(x.clamp(max=THRESHOLD + 1.0))))


def is_interior(case, bm, bn, i, j):
    """The kernel's rule, restated: tile (i, j) lies inside the rows and inside the activated columns."""
    return (i + 1) * bm <= case.M and (j + 1) * bn <= (case.N if case.mode == EPI_FWD else min(case.N, case.nact_bwd))


def tile_kinds(case, bm, bn):
    """-> set of 'interior', 'row' (cut by the last row), 'col' (by the last column), 'corner', 'inner-edge' (takes the
    bounds-checked epilogue although no edge of C crosses it: filler / non-activated columns)."""
    kinds = set()
    W = case.N + case.naux_fwd
    for i in range(-(-case.M // bm)):
        for j in range(-(-W // bn)):
            rc, cc = (i + 1) * bm > case.M, (j + 1) * bn > W
            kinds.add("interior" if is_interior(case, bm, bn, i, j) else "corner" if rc and cc else "row" if rc else "col" if cc else "inner-edge")
    return kinds


# ------------------------------------------------------------------------------------------------ wrong variants
MUTATIONS = ("bias_on_tangents", "dact_from_last_row", "tangents_no_out_scale", "no_c2_cross", "cross_missing_last_tangent",
             "scales_swapped", "nact_plus1", "nact_minus1", "filler_next_column", "filler_no_out_scale", "threshold_at_zero",
             "group4_for_group2", "swap_row_blocks", "drop_k_step")


def mutant(case, inp, ref, name, bm):
    """-> (C of the wrong variant, mask of the elements the variant can affect), or None where it does not apply to the case."""
    fwd, soft, g, M, N, W = case.mode == EPI_FWD, case.act == ACT_SOFTPLUS100, case.group, case.M, case.N, case.N + case.naux_fwd
    nact = N if fwd else min(case.nact_bwd, N)
    S = M // g
    mask = torch.zeros(S, g, W, dtype=torch.bool)
    acc = ref.acc
    bias = None if inp["bias"] is None else inp["bias"].double()
    aux = None if inp["aux"] is None else inp["aux"].double()
    scales_matter = case.act != ACT_NONE or case.aux_scale != case.out_scale
    if name == "bias_on_tangents":
        ok = fwd and g > 1
        mask[:, 1:, :N] = True
    elif name == "dact_from_last_row":
        ok = g > 1 and case.act != ACT_NONE and nact > 0
        mask[:, :, :nact] = True
        if fwd:
            mask[:, 0, :] = False
    elif name == "tangents_no_out_scale":
        ok = fwd and g > 1 and case.out_scale != 1.0
        mask[:, 1:, :N] = True
    elif name in ("no_c2_cross", "cross_missing_last_tangent"):
        ok = not fwd and soft and g > 1 and nact > 0
        mask[:, 0, :nact] = True
    elif name == "scales_swapped":
        ok = not fwd and case.aux_scale != case.out_scale
        mask[:] = True
    elif name == "nact_plus1":
        ok = not fwd and case.nact_bwd < N and scales_matter
        mask[:, :, nact:nact + 1] = True
    elif name == "nact_minus1":
        ok = not fwd and 0 < case.nact_bwd <= N and scales_matter
        mask[:, :, nact - 1:nact] = True
    elif name in ("filler_next_column", "filler_no_out_scale"):
        ok = fwd and case.naux_fwd > 0 and (name == "filler_next_column" or case.out_scale != 1.0)
        mask[:, :, N:] = True
    elif name == "threshold_at_zero":
        ok = fwd and soft
        mask[:, :, :N] = True
    elif name == "group4_for_group2":
        ok = g == 2 and M >= 4 and not (not fwd and case.act == ACT_NONE) and nact > 0
        m4 = mask.reshape(M, W)[:M - M % 4].reshape(-1, 4, W)
        m4[:, 2:, :nact] = True
    elif name == "swap_row_blocks":
        ok = bm >= 64 and M >= 64
        mask.reshape(M, W)[:64] = True
    elif name == "drop_k_step":
        ok = True
        mask[:, :, :N] = True
    else:
        raise KeyError(name)
    if not ok:
        return None
    mask = mask.reshape(M, W)
    if name == "swap_row_blocks":          # two neighbouring 32-row blocks of the first tile change places
        C = ref.C.clone()
        C[:32], C[32:64] = ref.C[32:64], ref.C[:32]
        return C, mask
    if name == "drop_k_step":              # the first K step of 32 is missing from the product
        k = min(32, case.K)
        acc = acc - inp["A"][:, :k].double() @ inp["B"][:, :k].double().t()
        name = None
    return _epilogue(acc, bias, g, case.act, case.mode, case.out_scale, aux, case.naux_fwd, case.nact_bwd, case.aux_scale, wrong=name), mask


# Device-function constants of the Softplus epilogues (hardware exp2 / log2 / rcp): 4 x the maxima measured on the MI355X against
# float64, see profiles/gemm_epilogue_bounds.md (values, regimes, and the command that produced them).
R_EPI, A_EPI = 5.0e-6, 4.5e-7
