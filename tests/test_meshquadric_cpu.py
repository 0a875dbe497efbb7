"""Host side of the quadric vertex placement (no GPU): the float64 restatement of tests/_meshquadric_ref.py on shapes whose answer is
known, the quality conditions the GPU test holds the product to -- met by the restatement alone, with the margin stated there --, the
command's new arguments, and the refusals that come before any GPU work."""
import numpy as np
import pytest

import _meshprep_ref as mr
import _meshquadric_ref as mq


def test_shapes():
    v, f = mq.shape("sphere")
    assert v.shape == (1986, 3) and f.shape == (3968, 3) and v.dtype == np.float32
    assert abs(mq.volume(v, f) - 4 * np.pi / 3) < 0.02 and np.allclose(np.linalg.norm(v, axis=1), 1., atol=1e-6)
    v, f = mq.shape("cube")
    assert v.shape == (866, 3) and f.shape == (1728, 3) and mq.volume(v, f) == pytest.approx(8., abs=1e-12) and mq.cube_distance(v).max() == 0.
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()                             # closed
    np.testing.assert_allclose(mq.cube_distance(np.float64([[0, 0, 0], [0.5, 0, 0], [2, 0, 0], [2, 2, 1], [1, 1, 1]])), [1, 0.5, 1, np.sqrt(2.), 0])
    v, f = mq.flat_grid(800)
    assert len(v) == 640000 and len(f) == 1276802 and v[801].tolist() == [1., 1., 0.]
    assert np.array_equal(mq.shape("cube_jitter")[1], mq.shape("cube")[1]) and 0 < np.abs(mq.shape("cube_jitter")[0] - mq.shape("cube")[0]).max() < 0.012


def test_restatement_finds_the_corners_of_a_cube():
    """With reg -> 1e-9 a cell at a corner of the cube puts its vertex on the corner, one on an edge onto the edge (at the mean along
    it), one inside a side onto the side; the mean placement is up to 0.19 away."""
    v, f = mq.shape("cube")
    q = mq.simplify_quadric(v, f, 0.61, reg=1e-9)
    x, m = q["verts"], q["mean"]
    assert not q["clamped"].any() and not q["no_planes"].any()
    on = np.isclose(np.abs(x), 1., atol=1e-7)
    assert on.any(1).all()                                                                          # every vertex lies on the cube
    corners = on.all(1)
    assert corners.sum() == 8 and np.abs(np.abs(x[corners]) - 1.).max() < 1e-7
    assert 0.18 < mq.cube_distance(m).max() < 0.2 and mq.cube_distance(x).max() < 1e-7
    free = ~on                                                                                      # the directions no plane constrains stay at the mean
    assert np.abs(x[free] - m[free]).max() < 1e-7
    # reg = 1e-3, the default, leaves 1e-3 of that distance
    d = mq.simplify_quadric(v, f, 0.61)
    assert mq.cube_distance(d["verts"]).max() <= 1.01e-3 * mq.cube_distance(m).max()


def test_restatement_on_a_plane():
    """On a flat grid b - A m is zero: every vertex stays at its cell's mean, at any cell; one vertex per cell returns the input."""
    for z in (0., 0.25):
        v, f = mq.flat_grid(40, z)
        for cell in (0.75, 2.5, 3.0, 7.3):
            q = mq.simplify_quadric(v, f, cell)
            assert np.abs(q["verts"] - q["mean"]).max() <= 1e-13 and not q["clamped"].any() and not q["no_planes"].any() and q["max_shift"] <= 1e-13
            assert mq.face_flips(v, f, q["verts"], q["faces"], q["source"]) == (0, 0)
        assert np.array_equal(mq.simplify_quadric(v, f, 0.75)["verts"], v.astype(np.float64))


def test_restatement_degenerate_input():
    v = np.float32([[0, 0, 0], [1, 0, 0.1], [0, 1, 0.2], [5, 5, 5], [5.1, 5.1, 5.1], [5.2, 5.2, 5.2], [9, 0, 0]])
    f = np.int64([[0, 1, 2], [3, 4, 5], [-1, -1, -1], [3, 3, 4]])
    q = mq.simplify_quadric(v, f, 0.5)
    assert q["no_planes"].tolist() == [False, False, True, False, True] and np.array_equal(q["verts"][[2, 4]], q["mean"][[2, 4]])
    assert mq.simplify_quadric(v, np.zeros((0, 3), np.int64), 0.5)["no_planes"].all()
    flipped = mq.face_flips(v, f[:1], v[[0, 2, 1]], np.int64([[0, 1, 2]]), np.int64([0]))
    assert flipped == (1, 0) and mq.face_flips(v, f[:1], v[[0, 0, 0]], np.int64([[0, 1, 2]]), np.int64([0])) == (0, 1)


@pytest.mark.parametrize("name", mq.SHAPES)
def test_restatement_meets_the_quality_conditions(name):
    """The conditions of tests/test_meshquadric_gpu.py::test_quality_against_the_mean_placement, on the restatement alone (its
    docstring lists the values); 0.2 - 7 % of the sphere's cells are clamped, none of the cube's."""
    v, f = mq.shape(name)
    for cell in mq.CELLS:
        q, m = mq.simplify_quadric(v, f, cell), mr.simplify(v, f, cell)
        assert np.array_equal(q["faces"], m["faces"]) and np.array_equal(q["mean"], m["verts"])
        a, b = mq.quality(name, q["verts"], q["faces"]), mq.quality(name, m["verts"], m["faces"])
        fq, fm = mq.face_flips(v, f, q["verts"], q["faces"], q["source"]), mq.face_flips(v, f, m["verts"], m["faces"], q["source"])
        print(f"{name} {cell}: clamped {q['clamped'].mean():.3f}, surface {a['surface'] / b['surface']:.4f}, volume {a['volume']:.4f} / {b['volume']:.4f} = "
              f"{a['volume'] / b['volume']:.4f}, vertex {a['vertex']:.3g} / {b['vertex']:.3g}, flips {fq} / {fm}")
        if name.startswith("sphere"):
            assert 0.25 <= a["surface"] / b["surface"] <= 0.36 and 0.2 <= a["volume"] / b["volume"] <= 0.37
            assert 0.002 <= q["clamped"].mean() <= 0.08
        elif name == "cube":
            assert a["vertex"] <= 0.0011 * b["vertex"] and not q["clamped"].any()
        else:
            assert a["surface"] <= 0.11 * b["surface"] and not q["clamped"].any()
        assert fq[0] <= fm[0] and fq[1] == fm[1] == 0 and not q["no_planes"].any() and q["near_wall"].sum() <= (0.35 if name == "cube" else 0.01) * len(q["verts"])


def test_parser_accepts_the_placement_arguments(capsys):
    from selfreconcode_amd.texture import build_parser
    a = build_parser().parse_args(['--rec-root', 'r'])
    assert a.placement == 'mean' and a.simplify_report is False
    a = build_parser().parse_args(['--rec-root', 'r', '--placement', 'quadric', '--simplify-report'])
    assert a.placement == 'quadric' and a.simplify_report is True
    with pytest.raises(SystemExit):
        build_parser().parse_args(['--placement', 'median'])
    assert 'median' in capsys.readouterr().err


def test_refusals_come_before_any_gpu_work():
    """CPU tensors: reaching the GPU check would be a RuntimeError, so a ValueError shows the order."""
    import torch
    from selfreconcode_amd.mesh_prep import prepare_template, simplify_mesh, simplify_to
    v, f = mq.flat_grid(4)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for kw in (dict(placement="median"), dict(placement=None), dict(placement="quadric", reg=0.), dict(placement="quadric", reg=-1e-3),
               dict(reg=float("nan")), dict(reg=float("inf")), dict(reg="small")):
        with pytest.raises(ValueError, match="placement|reg"):
            simplify_mesh(tv, tf, 1.5, **kw)
        with pytest.raises(ValueError, match="placement|reg"):
            simplify_to(tv, tf, 4, **kw)
        with pytest.raises(ValueError, match="placement|reg"):
            prepare_template(None, "unused", TmpVs=tv, Tmpfs=tf, **kw)
    for placement in ("mean", "quadric"):
        with pytest.raises(RuntimeError):
            simplify_mesh(tv, tf, 1.5, placement=placement)
