"""CPU-side checks of the winding-number feature: the restatement of tests/_winding_ref.py against closed forms and its
tree against its exact sum, the extension header, the coloured PLY, the colour map and the command line's refusals.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _meshprep_ref as mr
import _winding_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _sphere(n, jittered=True):
    from selfreconcode_amd.synthetic import cube_sphere
    key = (n, jittered)
    if key not in _CACHE:
        v, f = [x.numpy() for x in cube_sphere(n)]
        _CACHE[key] = (mr.jitter(v, 5, 0.004) if jittered else v, f)
    return _CACHE[key]


def test_closed_forms():
    one = wr.exact(np.zeros((1, 3)), np.float64([[1, 0, 0], [0, 1, 0], [0, 0, 1]]), np.int64([[0, 1, 2]]))
    assert abs(abs(one[0]) - 0.125) < 1e-15 and one[0] > 0                     # an octant, its normal pointing away from the origin
    v, f = _sphere(8, jittered=False)
    rng = np.random.default_rng(1)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside, outside = wr.exact(0.5 * d, v.astype(np.float64), f), wr.exact(2. * d, v.astype(np.float64), f)
    print(f"closed cube_sphere(8): |w - 1| at radius 0.5 {np.abs(inside - 1).max():.3g}, |w| at radius 2 {np.abs(outside).max():.3g}")
    assert np.abs(inside - 1.).max() <= 1e-12 and np.abs(outside).max() <= 1e-12
    assert wr.signed_volume(v, f) > 0 > wr.signed_volume(v, f[:, ::-1])
    # a corner of a face, a point of a face's plane outside the face, a face without area, a non-finite point
    assert wr.exact(v[f[0, :1]], v, f[:1])[0] == 0. and wr.exact(v[f[0, :1]], v, f[:1], np.float32)[0] == 0.
    a, b, c = v[f[0]].astype(np.float64)
    assert abs(wr.exact((a + 3. * (b - a) + 2. * (c - a))[None], v, f[:1])[0]) < 1e-12
    assert abs(wr.exact(np.float64([[0.3, 0.2, 0.1]]), v, np.int64([[5, 5, 9]]))[0]) < 1e-15       # (the determinant's rounding)
    assert np.isnan(wr.exact(np.float64([[np.nan, 0, 0], [0, np.inf, 0]]), v, f)).all()


@pytest.mark.parametrize("mesh", ["closed", "open"])
def test_restated_tree_vs_restated_exact_sum(mesh):
    """The condition on the approximation at the default beta: |w_tree - w_exact| <= 0.05, a tenth of the decision margin of a closed
    mesh, on the jittered cube_sphere(16) and on it with the cap removed; on the closed mesh every decision equals the exact one."""
    v, f = _sphere(16)
    if mesh == "open":
        f = wr.open_sphere(v, f)
        assert 0 < len(f) < 3072
    p = wr.shell_points(600, 11)
    tree = wr.build_tree(v, f)
    assert tree["levels"] == 4 and tree["nodes"].shape == (4681, 8) and tree["leaf_start"][-1] == len(f)
    counts = {}
    w_tree, w_exact = wr.tree_query(p, tree, 3.0, counts=counts), wr.exact(p, v, f)
    err = float(np.abs(w_tree - w_exact).max())
    print(f"restated tree vs exact sum, {mesh} cube_sphere(16), beta 3, {tree['levels']} levels: max |dw| {err:.3g} (condition 0.05); "
          f"accepted nodes per point {counts['accepted'].min()}-{counts['accepted'].max()}, exact faces {counts['faces'].min()}-{counts['faces'].max()}")
    assert err <= 0.05
    if mesh == "closed":
        assert np.array_equal(w_tree >= 0.5, w_exact >= 0.5)
        assert np.array_equal(w_exact >= 0.5, np.linalg.norm(p, axis=1) < 1.)
    # opening every node sums the same faces: the exact sum
    assert np.abs(wr.tree_query(p, tree, np.inf) - w_exact).max() < 1e-12
    # the root carries the whole mesh
    tri = v.astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum()
    assert abs(tree["nodes"][0, 6] - area) <= 1e-5 * area
    r = tree["nodes"][0, 7]
    assert (np.linalg.norm(tri.reshape(-1, 3) - tree["nodes"][0, 3:6], axis=1) <= r * (1 + 1e-5)).all()      # the radius covers every corner


def test_extension_header_declares_exactly_the_new_entry_points():
    from selfreconcode_amd import _abi, _lib, winding_ops
    with open(os.path.join(ROOT, "selfreconcode_amd", "csrc", "winding_abi.h")) as fh:
        defines, structs, functions = _abi.parse(fh.read())
    assert set(functions) == {"sr_winding_keys", "sr_winding_leaves", "sr_winding_fold", "sr_winding_query", "sr_winding_brute"}
    assert defines == {"SR_WINDING_MAX_LEVELS": 7, "SR_WINDING_NODE_FLOATS": 8} and not structs
    assert winding_ops.MAX_LEVELS == 7 and winding_ops.NODE_FLOATS == 8 and winding_ops.LEAF_FACTOR == 2.0
    c = ctypes
    assert functions["sr_winding_brute"] == (c.c_int, [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p])
    for name, (restype, argtypes) in functions.items():
        assert name not in _lib.SIGNATURES and not hasattr(_lib, "SR_WINDING_MAX_LEVELS")
        f = _lib.raw(name)                                  # bound by winding_ops' import, through the same table as the rest
        assert f.restype is restype and list(f.argtypes) == argtypes and argtypes[-1] is c.c_void_p
    assert not os.path.exists(os.path.join(ROOT, "include", "winding_abi.h")) and len(_lib.SIGNATURES) == 148


def test_bind_header_refuses_a_missing_symbol_and_a_redeclaration(tmp_path):
    from selfreconcode_amd import _lib
    (tmp_path / "a.h").write_text("int sr_winding_no_such_entry(int64_t n, void* stream);\n")
    with pytest.raises(ImportError, match="sr_winding_no_such_entry"):
        _lib.bind_header(str(tmp_path / "a.h"))
    (tmp_path / "b.h").write_text("int sr_mesh_sample(int64_t n, void* stream);\n")
    with pytest.raises(ImportError, match="sr_mesh_sample"):
        _lib.bind_header(str(tmp_path / "b.h"))
    assert _lib.raw("sr_mesh_sample").argtypes == _lib.SIGNATURES["sr_mesh_sample"]
    with pytest.raises(ImportError):
        _lib.bind_header(str(tmp_path / "none.h"))


PLAIN = ("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
         "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
         "0 0 0\n1 0 0.5\n0 1.25 0\n0.100000001 0.200000003 -3\n3 0 1 2\n3 0 2 3\n")


def test_write_ply_with_and_without_colours(tmp_path):
    from selfreconcode_amd.mesh_io import read_ply, write_ply
    v = np.float32([[0, 0, 0], [1, 0, 0.5], [0, 1.25, 0], [0.1, 0.2, -3]])
    f = np.int64([[0, 1, 2], [0, 2, 3]])
    write_ply(str(tmp_path / "plain.ply"), v, f)
    assert open(tmp_path / "plain.ply", "rb").read() == PLAIN.encode()         # byte for byte what the writer gave before colours
    colors = np.uint8([[255, 0, 0], [0, 255, 7], [255, 255, 255], [1, 2, 3]])
    write_ply(str(tmp_path / "c.ply"), v, f, colors)
    lines = open(tmp_path / "c.ply").read().splitlines()
    assert lines[6:9] == ["property uchar red", "property uchar green", "property uchar blue"] and lines[12] == "0 0 0 255 0 0"
    assert lines[15] == "0.100000001 0.200000003 -3 1 2 3" and lines[16:] == ["3 0 1 2", "3 0 2 3"]
    rv, rf = read_ply(str(tmp_path / "c.ply"))
    assert rv.dtype == np.float32 and np.array_equal(rv, v) and np.array_equal(rf, f)
    for bad in (colors[:3], colors.astype(np.int32), colors[:, :2]):
        with pytest.raises(ValueError):
            write_ply(str(tmp_path / "bad.ply"), v, f, bad)


def test_error_colors():
    from selfreconcode_amd.evaluate import error_colors, error_range
    d = torch.tensor([-0.2, -0.1, 0., 0.1, 0.2, 0.5, -7., float("nan"), 0.05], dtype=torch.float64)
    got = error_colors(d, 0.2, True)
    assert got.dtype == torch.uint8 and got.shape == (9, 3)
    assert got.tolist() == [[0, 0, 255], [128, 128, 255], [255, 255, 255], [255, 128, 128], [255, 0, 0], [255, 0, 0], [0, 0, 255],
                            [128, 128, 128], [255, 191, 191]]                # 127.5 -> 128, 191.25 -> 191: half up
    red = error_colors(d, 0.2, False).tolist()                     # unsigned: the red half only
    assert red[:3] == [[255, 255, 255]] * 3 and red[3:7] == [[255, 128, 128], [255, 0, 0], [255, 0, 0], [255, 255, 255]]
    assert error_colors(torch.tensor([0.1], dtype=torch.float32), 0.2, True).tolist() == [[255, 127, 127]]     # float32(0.1) / 0.2 > 1/2
    for limit in (0., -1., float("nan"), float("inf")):
        with pytest.raises(ValueError):
            error_colors(d, limit, True)
    assert error_range(torch.arange(-100, 0, dtype=torch.float32)) == 95. and error_range(torch.zeros(5)) == 1.
    assert error_range(torch.tensor([float("nan"), 2.])) == 2.


def test_parse_args_refusals():
    from selfreconcode_amd.evaluate import parse_args
    pair, folder = ["--pred", "a.ply", "--gt", "b.ply"], ["--rec-root", "R", "--gt-root", "G"]
    ok = parse_args(pair + ["--signed", "--beta", "2", "--error-range", "0.05", "--error-mesh", "e.ply"])
    assert ok.signed and ok.beta == 2. and ok.error_range == 0.05 and ok.error_mesh == "e.ply" and not ok.error_meshes
    ok = parse_args(folder + ["--error-meshes", "--beta", "inf"])
    assert ok.error_meshes and ok.beta == float("inf") and not ok.signed and ok.error_range is None
    plain = parse_args(pair)
    assert not plain.signed and plain.beta == 3.0 and plain.error_mesh is None and not plain.error_meshes and plain.error_range is None
    for bad in (folder + ["--error-mesh", "e.ply"], pair + ["--error-meshes"], pair + ["--error-range", "0"], pair + ["--error-range", "-1"],
                pair + ["--error-range", "nan"], pair + ["--beta", "0.5"], folder + ["--beta", "nan"], pair + ["--signed", "--beta", "-3"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
