"""Measures the device functions of the Softplus epilogues (softplus100, dsoftplus100, softplus100_from_stored in
csrc/mlp_gemm.hip: hardware exp2 / log2 / rcp) against float64, for profiles/gemm_epilogue_bounds.md.

An ACT_SOFTPLUS100 launch with K = 4 and one weight of 1 per output column makes the accumulator exact (acc[r, c] = A[r, c]), so
what comes out is the device function alone:
  SR_EPI_FWD, group 2, primal rows z, tangent rows 1:          C = (softplus100(z), dsoftplus100(z))
  SR_EPI_BWD, group 2, acc rows (0, 1), aux rows (a, 1):      C = (c2(a), d(a) * aux_scale)      [c2 * cross with cross = 1]
z covers 100 z in [-80, 80] (the tests' inputs reach about +-70), uniformly and densely around the branch points.
Per function: max |err| where |ref| < 0.1 (the absolute regime: 1 + e and 1 - e^-x round at 6e-8 whatever the result), max
|err| / |ref| where |ref| >= 0.1, and both over everything.

    python tools/measure_epilogue_units.py [out.json]"""
import json
import math
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gemm_epilogue_ref as R          # noqa: E402
from selfreconcode_amd import mlp_engine as me     # noqa: E402

DEV = "cuda:0"
SPLIT = 0.1


def grid():
    t = [torch.linspace(-80, 80, 1 << 20, dtype=torch.float64)]
    for centre, half in ((20.0, 0.01), (math.log(1e-3), 0.01), (0.0, 1.0), (-6.9, 0.5), (20.0, 2.0)):
        t.append(torch.linspace(centre - half, centre + half, 1 << 16, dtype=torch.float64))
    t = torch.cat(t)
    t = t[:t.numel() // 4 * 4]
    return (t / 100.0).float()                       # the float32 z the kernel sees


def stats(got, ref):
    err = (got.double() - ref).abs()
    small = ref.abs() < SPLIT
    rel = err / ref.abs().clamp(min=1e-300)
    return {"max_abs_where_ref_lt_0.1": err[small].max().item() if small.any() else 0.0,
            "max_rel_where_ref_ge_0.1": rel[~small].max().item() if (~small).any() else 0.0,
            "max_abs_all": err.max().item(), "max_rel_all": rel.max().item(), "n": int(err.numel())}


def launch(A, aux, mode, aux_scale):
    M = A.shape[0]
    B = torch.eye(4, device=DEV)
    C = torch.full((M, 4), float("nan"), device=DEV)
    me._gemm_nt(A, 4, B, 4, C, 4, M, 4, 4, None, 2, me.ACT_SOFTPLUS100, mode, out_scale=1.0, aux=aux, ldaux=4, nact_bwd=4, aux_scale=aux_scale)
    torch.cuda.synchronize()
    return C.cpu()


def main():
    z = grid().reshape(-1, 4)
    S = z.shape[0]
    out = {}
    A = torch.ones(S, 2, 4)
    A[:, 0] = z
    C = launch(A.reshape(2 * S, 4).to(DEV), None, me.EPI_FWD, 1.0).reshape(S, 2, 4)
    a64, d64 = R.act_and_derivative(z.double(), R.ACT_SOFTPLUS100)
    out["softplus100"] = stats(C[:, 0], a64)
    out["dsoftplus100"] = stats(C[:, 1], d64)
    for name, s in (("1", 1.0), ("rsqrt2", R.RSQRT2)):
        stored = (a64 * s).float()                   # what a forward pass leaves behind
        aux = torch.ones(S, 2, 4)
        aux[:, 0] = stored
        acc = torch.ones(S, 2, 4)
        acc[:, 0] = 0.0
        C = launch(acc.reshape(2 * S, 4).to(DEV), aux.reshape(2 * S, 4).to(DEV), me.EPI_BWD, s).reshape(S, 2, 4)
        d, c2 = R.stored_factors(stored.double(), R.ACT_SOFTPLUS100, s)
        out[f"from_stored.c2 (aux_scale {name})"] = stats(C[:, 0], c2)
        out[f"from_stored.d * aux_scale (aux_scale {name})"] = stats(C[:, 1], d * s)
    out["r_meas"] = max(v["max_rel_where_ref_ge_0.1"] for v in out.values() if isinstance(v, dict))
    out["a_meas"] = max(v["max_abs_where_ref_lt_0.1"] for v in out.values() if isinstance(v, dict))
    txt = json.dumps(out, indent=1)
    print(txt)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
