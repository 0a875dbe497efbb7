"""Host side of the template preparation (no GPU): the shelf packer `mesh_prep.pack_charts`, and the float64 restatement of
tests/_meshprep_ref.py on meshes whose answer is known."""
import numpy as np
import pytest

import _meshprep_ref as mr


def _disjoint_inside(origin, size, R):
    lo, hi = origin, origin + size
    assert (lo >= 0).all() and (hi <= R).all()
    apart = (hi[:, None, :] <= lo[None, :, :]) | (hi[None, :, :] <= lo[:, None, :])          # separated along x or along y
    ok = apart.any(-1) | np.eye(len(lo), dtype=bool)
    assert ok.all(), np.argwhere(~ok)[:4]


@pytest.mark.parametrize("C, R, padding", [(1, 64, 2), (6, 256, 2), (57, 256, 1), (300, 512, 0), (1000, 1680, 2)])
def test_pack_charts_rectangles(C, R, padding):
    from selfreconcode_amd.mesh_prep import pack_charts
    rng = np.random.default_rng(C)
    extent = rng.uniform(0., 1., (C, 2)) ** 3                     # a few large charts, many small ones
    if C > 1:
        extent[rng.integers(0, C)] = 0.                            # and a point
    scale, origin, size = pack_charts(extent, R, padding)
    assert scale > 0 and origin.dtype == np.int64 and size.dtype == np.int64 and origin.shape == size.shape == (C, 2)
    assert np.array_equal(size, np.ceil(extent * scale).astype(np.int64) + 2 * padding + 1)
    _disjoint_inside(origin, size, R)
    again = pack_charts(extent.copy(), R, padding)
    assert again[0] == scale and np.array_equal(again[1], origin) and np.array_equal(again[2], size)
    # shelves: rectangles in the order (height desc, width desc, label asc) run left to right, and a row starts at x = 0
    order = np.lexsort((np.arange(C), -size[:, 0], -size[:, 1]))
    o, s = origin[order], size[order]
    assert tuple(o[0]) == (0, 0)
    for i in range(1, C):
        same = o[i, 1] == o[i - 1, 1]
        assert (same and o[i, 0] == o[i - 1, 0] + s[i - 1, 0]) or (not same and o[i, 0] == 0 and o[i, 1] > o[i - 1, 1] and o[i - 1, 0] + s[i - 1, 0] + s[i, 0] > R)


@pytest.mark.parametrize("R, padding, extent", [(64, 2, (0.5, 2.)), (1680, 2, (3., 1.)), (256, 0, (1., 1.))])
def test_pack_charts_single_chart_fills_the_atlas(R, padding, extent):
    from selfreconcode_amd.mesh_prep import pack_charts
    scale, origin, size = pack_charts(np.float64([extent]), R, padding)
    best = (R - 2 * padding - 1) / max(extent)
    step = R / max(extent) * 2. ** -24                             # the bracket [0, R / max extent] after 24 halvings
    assert best - step <= scale <= best
    assert tuple(origin[0]) == (0, 0) and size.max() <= R


def test_pack_charts_refusal_and_points():
    from selfreconcode_amd.mesh_prep import pack_charts
    with pytest.raises(ValueError, match=r"10000 charts.*64"):
        pack_charts(np.ones((10000, 2)), 64, 2)
    scale, origin, size = pack_charts(np.zeros((7, 2)), 64, 2)
    assert scale == 0. and (size == 5).all()
    _disjoint_inside(origin, size, 64)
    scale, origin, size = pack_charts(np.zeros((0, 2)), 64, 2)
    assert scale == 0. and origin.shape == (0, 2)


def test_restatement_on_a_cube():
    from selfreconcode_amd.synthetic import cube_sphere
    v, f = [x.numpy() for x in cube_sphere(1)]                     # 8 vertices, 12 faces: the cube itself
    assert v.shape == (8, 3) and f.shape == (12, 3)
    ref = mr.charts(v, f)
    assert len(ref["labels"]) == 6 and np.bincount(ref["chart"]).tolist() == [2] * 6
    assert sorted(ref["cls"][ref["labels"]].tolist()) == [0, 1, 2, 3, 4, 5]
    side = 2. / np.sqrt(3.)
    np.testing.assert_allclose(ref["extent"], side, rtol=1e-6)
    assert (mr.tri_area2(ref["uv"].astype(np.float64)) > 0).all()  # outward faces project with positive area
    # a zero-area face is class +x, and three faces on one edge are one chart
    cls, n = mr.face_classes(np.float32([[0, 0, 0], [1, 1, 1], [2, 2, 2]]), np.int64([[0, 1, 2]]))
    assert cls.tolist() == [0] and not n.any()
    fv, ff = mr.fan_on_edge()
    assert mr.charts(fv, ff)["chart"].tolist() == [0, 0, 0]


def test_restatement_simplify_small():
    v = np.float32([[0, 0, 0], [0.01, 0, 0], [1, 0, 0], [1.01, 0, 0], [0, 1, 0], [0.01, 1, 0], [0.5, 0, 0]])
    f = np.int64([[4, 2, 0], [0, 2, 4], [1, 3, 5], [-1, -1, -1], [0, 1, 2], [0, 6, 4]])
    ref = mr.simplify(v, f, 0.5)
    assert ref["vertex_map"].tolist() == [0, 0, 2, 2, 3, 3, 1]     # 0.5 / 0.5 = 1 exactly: the vertex on the boundary belongs to the upper cell
    assert ref["faces"].tolist() == [[3, 2, 0], [0, 1, 3]]
    np.testing.assert_allclose(ref["verts"][0], [0.005, 0, 0], atol=1e-9)
