"""What of the ICP alignment can be checked without a GPU: the numpy restatement of tests/_icp_ref.py meets the
conditions the GPU tests rely on (it recovers the known transform and reaches `done` well inside the launches they use; a flat target
gives rank 3 and a finite answer), the command's new flags and refusals, the refusal of CPU tensors and of an `init` with shear, and
the header."""
import os

import numpy as np
import pytest
import torch

import _icp_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2. ** -23


@pytest.mark.parametrize("name", ["rigid", "similarity"])
def test_restatement_recovers_the_transform(name):
    """n = 16, S = 2003, 12 iterations: the answer is (s0, R0, t0) far inside 8 2^-23 scale, the bound the GPU tests use, and the
    float32-search variant stays as close to the float64 one."""
    pred, gt, answer = ir.case(name, 16)
    assert len(gt[0]) == 1538 and len(gt[1]) == 3072
    scale = max(float(np.abs(pred[0]).max()), float(np.abs(gt[0]).max()))
    r = ir.icp(pred, gt, 2003, iters=12, scale=name == "similarity")
    r32 = ir.icp(pred, gt, 2003, iters=12, scale=name == "similarity", dtype=np.float32)
    err = float(np.abs(r["matrix"] - ir.truth_matrix(answer)).max())
    e32 = float(np.abs(r["matrix"] - r32["matrix"]).max())
    print(f"{name}: {r['iterations']} iterations, |matrix - truth| {err:.3g}, float32 search against float64 {e32:.3g}; bound {8 * EPS * scale:.3g}")
    assert r["converged"] and r32["converged"] and r["iterations"] <= 8 and r32["iterations"] <= 8
    assert r["rank"] == (7 if name == "similarity" else 6)
    assert err <= 8. * EPS * scale / 16. and e32 <= 8. * EPS * scale / 16.             # (more than an order inside the GPU tests' bound)
    h = r["history"]
    assert (h[:, 0] == 2003).all() and (h[r["iterations"]:, 5] == 1).all() and (h[:r["iterations"] - 1, 5] == 0).all()
    assert np.array_equal(h[r["iterations"]:, :5], np.repeat(h[r["iterations"] - 1:r["iterations"], :5], 12 - r["iterations"], 0))
    assert h[r["iterations"] - 1, 1] < 1e-3 * h[0, 1]                                    # the rms distance fell by orders
    M = r["matrix"][:3, :3]
    s = np.sqrt((M * M).sum() / 3.)
    assert np.abs(M @ M.T / (s * s) - np.eye(3)).max() <= 64 * 2. ** -52 and np.linalg.det(M) > 0


def test_restatement_small_shape_converges_too():
    pred, gt, answer = ir.case("rigid", 8)
    r = ir.icp(pred, gt, 2003, iters=12)
    assert r["converged"] and r["iterations"] <= 8
    assert np.abs(r["matrix"] - ir.truth_matrix(answer)).max() <= 8. * EPS * float(np.abs(gt[0]).max())


def test_restatement_solve_against_lstsq():
    """The restatement's own Cholesky and numpy's least squares agree on a full-rank system to the noise of float64."""
    pred, gt, _ = ir.case("similarity", 8)
    q = ir.samples_of(pred, 501, 0)
    d, f, c = ir.sr.closest(q, gt[0], gt[1])
    o, rho = ir.frame(gt[0])
    W = ir.rows(q.astype(np.float64), c, ir.sr.face_normals(gt[0], gt[1])[f], o, rho)
    for scale in (False, True):
        xi, rank = ir.solve(W.T @ W, 501., scale)
        assert rank == (7 if scale else 6) and (xi[6] != 0.) == scale
        assert np.abs(xi - ir.solve_lstsq(W.T @ W, 501., scale)).max() < 1e-10


def test_flat_target_has_rank_three_and_a_finite_answer():
    """A flat square against itself, lifted along its normal: rotation about the normal and the two translations in the plane are not
    constrained -- exactly 0, rank 3 -- and the lift is undone in one step."""
    pred, gt = ir.flat_pair(0.05)
    q = ir.samples_of(pred, 257, 0)
    d, f, c = ir.sr.closest(q, gt[0], gt[1])
    o, rho = ir.frame(gt[0])
    W = ir.rows(q.astype(np.float64), c, ir.sr.face_normals(gt[0], gt[1])[f], o, rho)
    xi, rank = ir.solve(W.T @ W, 257., False)
    assert rank == 3 and np.isfinite(xi).all()
    assert xi[2] == 0. and xi[3] == 0. and xi[4] == 0. and xi[6] == 0.
    assert abs(xi[5] * rho + 0.05) < 1e-7
    xi, rank = ir.solve(W.T @ W, 257., True)                                             # sigma is the lift again: the pivot drops it
    assert rank == 3 and xi[6] == 0. and np.isfinite(xi).all()
    r = ir.icp(pred, gt, 257, iters=5, init="none")
    assert r["converged"] and r["iterations"] == 2 and r["rank"] == 3 and np.isfinite(r["matrix"]).all()
    assert abs(r["matrix"][2, 3] + 0.05) < 1e-7 and np.abs(r["matrix"][:3, :3] - np.eye(3)).max() < 1e-12
    xi, rank = ir.solve(np.zeros((8, 8)), 0., True)                                      # no pairs at all
    assert rank == 0 and (xi == 0.).all()


# ---------------------------------------------------------------------------------------------------------------- command, refusals
def test_parser_alignment_flags():
    from selfreconcode_amd.evaluate import build_parser, parse_args
    a = parse_args(["--pred", "a.ply", "--gt", "b.obj"])
    assert (a.align, a.align_samples, a.align_iters, a.align_max_dist, a.align_shared) == ("none", 100_000, 30, None, False)
    a = parse_args(["--pred", "a.ply", "--gt", "b.obj", "--align", "similarity", "--align-samples", "5000", "--align-iters", "12",
                    "--align-max-dist", "0.25"])
    assert (a.align, a.align_samples, a.align_iters, a.align_max_dist) == ("similarity", 5000, 12, 0.25)
    a = parse_args(["--rec-root", "R", "--gt-root", "G", "--align", "rigid", "--align-shared"])
    assert a.align == "rigid" and a.align_shared
    pair, folder = ["--pred", "a.ply", "--gt", "b.ply"], ["--rec-root", "R", "--gt-root", "G"]
    for argv in (pair + ["--align", "affine"], pair + ["--align", "rigid", "--align-samples", "0"], pair + ["--align", "rigid", "--align-iters", "0"],
                 pair + ["--align", "rigid", "--align-max-dist", "-1"], pair + ["--align", "rigid", "--align-shared"], folder + ["--align-shared"],
                 folder + ["--align", "none", "--align-shared"]):
        with pytest.raises(SystemExit):
            parse_args(argv)
    text = " ".join(build_parser().format_help().split())
    assert "No alignment and no scaling" in text and "--align-shared" in text


def test_cpu_tensors_are_refused():
    from selfreconcode_amd import align, evaluate
    v, f = torch.from_numpy(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])), torch.from_numpy(np.int64([[0, 1, 2]]))
    with pytest.raises(RuntimeError):
        align.icp_align((v, f), (v, f), samples=10)
    with pytest.raises(RuntimeError):
        evaluate.surface_metrics((v, f), (v, f), 10, align="rigid")
    with pytest.raises(RuntimeError):
        evaluate.vertex_to_surface(v, (v, f), align="rigid", faces=f)
    t = align.Alignment(np.eye(4), 1., np.eye(3), np.zeros(3), 1, True, 6, 10, 0., 0., np.zeros((1, 6)))
    with pytest.raises(RuntimeError):
        t.apply(v)


def test_init_matrix_is_checked():
    from selfreconcode_amd.align import check_init
    _, _, answer = ir.case("similarity", 4)
    good = ir.truth_matrix(answer)
    M, t = check_init(good)
    assert np.array_equal(M, good[:3, :3]) and np.array_equal(t, good[:3, 3])
    check_init(torch.from_numpy(good.astype(np.float32)))                                # a float32 matrix passes
    shear = good.copy()
    shear[0, 1] += 1e-3
    mirror = good.copy()
    mirror[:3, 0] *= -1.
    stretch = good.copy()
    stretch[:3, :3] = stretch[:3, :3] @ np.diag([1., 1., 1.01])
    projective = good.copy()
    projective[3, 0] = 0.1
    nan = good.copy()
    nan[1, 3] = np.nan
    for bad in (shear, mirror, stretch, projective, nan, np.zeros((4, 4)), np.eye(3)):
        with pytest.raises(ValueError):
            check_init(bad)


def test_blocks_are_fixed_from_the_sample_count():
    from selfreconcode_amd import align
    assert [align.blocks_of(s) for s in (1, 256, 257, 1031, 1024 * 256, 1024 * 256 + 257, 10 ** 7)] == [1, 1, 2, 5, 1024, 1024, 1024]


def test_header_declares_the_entries_and_python_mirrors_its_constants():
    import re
    from selfreconcode_amd import align
    txt = open(os.path.join(ROOT, "include", "selfrecon_hip.h")).read()
    for name in ("sr_icp_accumulate", "sr_icp_solve"):
        assert ("int %s(" % name) in txt, name
    d = {k: int(v) for k, v in re.findall(r"^#define (SR_ICP_\w+) (\d+)$", txt, flags=re.M)}
    assert d == {"SR_ICP_MAX_BLOCKS": align.MAX_BLOCKS, "SR_ICP_COLS": align.COLS, "SR_ICP_HISTORY": align.HISTORY, "SR_ICP_STATE": align.STATE,
                 "SR_ICP_DONE": align.DONE}
    src = open(os.path.join(ROOT, "selfreconcode_amd", "csrc", "icp.hip")).read()
    assert '#include "surfdist_device.h"' in src and '#include "surfdist_device.h"' in open(os.path.join(ROOT, "selfreconcode_amd", "csrc", "surfdist.hip")).read()
