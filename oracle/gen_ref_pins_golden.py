"""TEST INFRASTRUCTURE -- freezes what the reference-pin tests take from the host builds of the reference's own kernels (oracle/_ref,
see oracle/Makefile) into tests/golden/ref_pins.npz, so that the pins hold where neither the reference tree nor oracle/_ref exists:
  mc*    marching cubes (tests/test_mc_reference_pin.py): digests of the canonical (vertices, edge keys, faces) of both builds per case,
         the largest vertex difference between them, the iso-value cases, the vertices / sorted faces of the GPU cases, and the
         all-cases block volume of tests/_mc_volumes.py (tests/test_mc_paths_cpu.py);
  minv*  3x3 inverse (tests/test_minv_reference_pin.py): digests of inverse / flag / backward of the uncontracted build, its backward
         as an array (compared with a tolerance), and the agreement statistics of the contracted build;
  gs*    grid sampler (tests/test_gs_reference_pin.py): the relative difference of the contracted build's outputs from the uncontracted
         ones (whose outputs are tests/golden/gs_ref.npz).
Digests are oracle.fixtures.digest.  Run where the reference tree is present (oracle/Makefile builds its kernels):
    python -m oracle.gen_ref_pins_golden"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import mc as mco, minv_ref, gs_ref  # noqa: E402
from oracle.fixtures import digest  # noqa: E402
import test_mc_reference_pin as tmc  # noqa: E402
import _mc_volumes as mv  # noqa: E402
import test_minv_reference_pin as tmi  # noqa: E402
import test_gs_reference_pin as tgs  # noqa: E402

assert mco.reference_available() and minv_ref.reference_available() and gs_ref.reference_available(), "needs the reference tree"
out = {}
for n, (shape, kind) in enumerate(tmc.CASES):
    s = tmc.field(shape, kind)
    vf, kf, ff = mco.canonical(*mco.reference_marching_cubes(s, tmc.STEP, tmc.ORG, 0.0, "fma"))
    vn, kn, fn = mco.canonical(*mco.reference_marching_cubes(s, tmc.STEP, tmc.ORG, 0.0, "nofma"))
    out.update({f"mc{n}_vf": digest(vf), f"mc{n}_kf": digest(kf), f"mc{n}_ff": digest(ff), f"mc{n}_kn": digest(kn), f"mc{n}_fn": digest(fn),
                f"mc{n}_dvn": np.float64(np.abs(vf.astype(np.float64) - vn).max()) if vf.shape == vn.shape else np.float64(np.inf)})
for i, iso in enumerate(tmc.ISOS):
    for name, x in zip("vkf", mco.canonical(*mco.reference_marching_cubes(tmc.field((28, 20, 24), "two_blobs"), (1., 1., 1.), (0., 0., 0.), iso, "fma"))):
        out[f"mc_iso{i}_{name}"] = digest(x)
for n, (shape, kind) in enumerate(tmc.GPU_CASES):
    vf, kf, ff = mco.canonical(*mco.reference_marching_cubes(tmc.field(shape, kind), tmc.STEP, tmc.ORG, 0.0, "fma"))
    out[f"mcgpu{n}_v"], out[f"mcgpu{n}_f"] = digest(vf), digest(ff)
for name, x in zip("vkf", mco.canonical(*mco.reference_marching_cubes(mv.volume(mv.ALL_CASES), mv.STEP, mv.ORG, 0.0, "fma"))):
    out[f"mc_all_cases_{name}"] = digest(x)              # tests/test_mc_paths_cpu.py: each of the 256 cases in a block of its own
for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
    m = tmi._matrices(5000, dtype)
    inv_r, ok_r = minv_ref.forward(m, "nofma")
    g = tmi._cotangents(5000, dtype)
    out.update({f"minv_{tag}_inv": digest(inv_r), f"minv_{tag}_ok": digest(ok_r), f"minv_{tag}_bwd": minv_ref.backward(g, inv_r, "nofma")})
    out[f"minv_{tag}_fma_same"], out[f"minv_{tag}_fma_rel_median"] = tmi._fma_agreement(m, inv_r, ok_r)
    for n in tmi.GPU_SIZES:
        m = tmi._matrices(n, dtype)
        inv_r, ok_r = minv_ref.forward(m, "nofma")
        out.update({f"minv_{tag}_{n}_inv": digest(inv_r), f"minv_{tag}_{n}_ok": digest(ok_r),
                    f"minv_{tag}_{n}_bwd": digest(minv_ref.backward(tmi._cotangents(n, dtype), inv_r, "nofma"))})
    r, f = tgs.reference_outputs(dtype), tgs.reference_outputs(dtype, "fma")
    for k in r:
        out[f"gs_{tag}_fma_err_{k}"] = np.float64(tgs._rel_err(f[k], r[k]))
path = os.path.join(ROOT, "tests", "golden", "ref_pins.npz")
np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
print("wrote", path, os.path.getsize(path), "bytes,", len(out), "entries")
