"""Host side of the rotation search in front of the ICP (align.rotation_candidates, the argument checks of align.icp_index and of the
command) without a GPU: the candidate tables against the restatement of tests/_icp_search_ref.py, their group
properties, how well they cover SO(3), and the errors."""
import numpy as np
import pytest
import torch

import _icp_search_ref as isr

ULP = 2. ** -52


@pytest.mark.parametrize("kind,n", [("axes", None), ("search", 1), ("search", 64), ("search", 4096)])
def test_rotation_candidates_against_the_restatement(kind, n):
    from selfreconcode_amd.align import rotation_candidates
    got, want = rotation_candidates(kind, n), isr.rotation_candidates(kind, n)
    assert got.dtype == np.float64 and got.shape == want.shape == (24 + (n or 0), 3, 3)
    err = float(np.abs(got - want).max())
    ortho = float(np.abs(got @ got.transpose(0, 2, 1) - np.eye(3)).max())
    det = float(np.abs(np.linalg.det(got) - 1.).max())
    print(f"rotation_candidates {kind} {n}: |table - restatement| {err / ULP:.3g} ulp of 1 (bound 4), |R R^T - I| {ortho:.3g}, |det - 1| {det:.3g} (bound 1e-14)")
    assert err <= 4 * ULP and ortho <= 1e-14 and det <= 1e-14
    assert np.array_equal(got[:24], rotation_candidates("axes")) and np.array_equal(got[0], np.eye(3))
    assert np.array_equal(rotation_candidates(kind, n), got)                              # deterministic


def test_the_24_are_the_distinct_signed_permutations_of_determinant_one():
    from selfreconcode_amd.align import rotation_candidates
    cube = rotation_candidates("axes")
    assert cube.shape == (24, 3, 3) and set(np.unique(cube)) == {-1., 0., 1.}
    assert (np.abs(cube).sum(1) == 1).all() and (np.abs(cube).sum(2) == 1).all()          # one entry of +-1 per row and per column
    assert (np.linalg.det(cube) > 0).all()
    assert len({m.tobytes() for m in (cube + 0.)}) == 24                                  # (+ 0.: no -0 among the bytes)
    products = {(a @ b + 0.).tobytes() for a in cube for b in cube}
    assert products == {m.tobytes() for m in (cube + 0.)}                                 # a group: closed under the product
    # the stated order: permutations x sign triples, those with det > 0
    import itertools
    k = 0
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            m = np.zeros((3, 3))
            m[np.arange(3), perm] = signs
            if np.linalg.det(m) > 0:
                assert np.array_equal(cube[k], m)
                k += 1
    assert k == 24


def test_the_candidates_cover_the_rotations():
    """The largest angle from 4000 random rotations to the nearest candidate: 13.3 deg measured for the 4096 spiral rotations (bound
    15: inside the basin of the ICP on a body-like shape), 61.9 for the cube's 24 alone."""
    from selfreconcode_amd.align import rotation_candidates
    spiral = isr.nearest_angle_deg(rotation_candidates("search", 4096)[24:])
    both = isr.nearest_angle_deg(rotation_candidates("search", 4096))
    cube = isr.nearest_angle_deg(rotation_candidates("axes"))
    print(f"covering: largest angle to the nearest candidate {spiral:.1f} deg (n = 4096 alone), {both:.1f} (with the 24), {cube:.1f} (the 24 alone)")
    assert both <= spiral <= 15. and 55. < cube < 65.


def test_argument_errors():
    from selfreconcode_amd import align, evaluate
    for kind, n in (("pca", 4), ("search", 0), ("search", -3), ("search", None), ("search", 2.5), (None, 4)):
        with pytest.raises(ValueError):
            align.rotation_candidates(kind, n)
    mesh = (torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int64))
    # the search keywords are checked before anything touches the meshes, also when `init` does not use them
    for opts in (dict(candidates=0), dict(search_samples=0), dict(top=0), dict(refine_iters=0), dict(init="centroid", top=-1), dict(init="pca"),
                 dict(init="Search")):
        with pytest.raises(ValueError):
            align.icp_index(mesh, None, **opts)
    assert align.INITS == ("centroid", "none", "axes", "search")
    base = ["--pred", "a.ply", "--gt", "b.ply"]
    args = evaluate.parse_args(base + ["--align", "rigid"])
    assert (args.align_init, args.align_candidates, args.align_top) == ("centroid", 4096, 8)
    assert evaluate._align_args(args)[1]["init"] == "centroid"
    args = evaluate.parse_args(base + ["--align", "similarity", "--align-init", "search", "--align-candidates", "512", "--align-top", "4"])
    assert evaluate._align_args(args) == ("similarity", {"samples": 100_000, "seed": 0, "iters": 30, "max_dist": None, "init": "search",
                                                         "candidates": 512, "top": 4})
    for bad in (["--align", "rigid", "--align-init", "pca"], ["--align", "rigid", "--align-candidates", "0"], ["--align", "rigid", "--align-top", "0"],
                ["--align-init", "search"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(base + bad)


def test_summary_carries_the_search_only_when_set():
    from selfreconcode_amd.align import Alignment
    a = Alignment(matrix=np.eye(4), scale=1., rotation=np.eye(3), translation=np.zeros(3), iterations=1, converged=True, rank=6, pairs=1,
                  rms_before=0., rms_after=0., history=np.zeros((1, 6)))
    assert a.search is None and set(a.summary()) == {"matrix", "scale", "iterations", "converged", "rank", "rms_before", "rms_after"}
    found = {"kind": "axes", "candidates": 24, "top": [3, 0], "score": [1., 2.], "refined": [0.5, 0.25], "winner": 0, "angle_deg": 90.}
    a.search = found
    assert a.summary()["search"] == found and list(a.summary())[-1] == "search"
    from selfreconcode_amd.evaluate import search_line
    assert search_line(found) == "      search axes: candidate 0 of 24, 90.0 deg from the centroid start, J 2 -> 0.25"
