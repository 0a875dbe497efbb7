"""The file writers of selfreconcode_amd/infer_export.py (infer.py:102-183 of the reference) without a GPU: errors.txt in the
reference's exact layout, PNG round trips, the template PLY."""
import numpy as np

from _png import read_png


def test_errors_txt_layout_and_filtered_maxinds(tmp_path):
    from selfreconcode_amd.infer_export import write_errors
    p = tmp_path / "errors.txt"
    write_errors(str(p), np.array([-1., .25, .5, -1., .125]))
    # maxinds index the array filtered to e >= 0: the largest error (frame 2) is index 1 there, then frame 1 (index 0), frame 4 (2)
    assert p.read_text() == ("      mask\n"
                             "   1: 0.2500\n"
                             "   2: 0.5000\n"
                             "   4: 0.1250\n"
                             "mask mean: 0.2917, max: 0.5000, min: 0.1250, maxinds:1 0 2 ")


def test_png_round_trip_odd_sizes(tmp_path):
    from selfreconcode_amd.infer_export import write_png
    rng = np.random.default_rng(7)
    for shape in [(1, 1, 3), (3, 5, 3), (3, 5, 4), (5, 3), (1, 1, 4)]:
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        p = tmp_path / ("%s.png" % "x".join(map(str, shape)))
        write_png(str(p), a)
        b = read_png(str(p))
        assert b.dtype == np.uint8 and b.shape == a.shape and np.array_equal(a, b), shape
    # non-contiguous views (the writers pass img[:, :, :3] and color[:, :, ::-1])
    a = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    write_png(str(tmp_path / "v.png"), a[:, :, ::-1][:, :, 1:])
    assert np.array_equal(read_png(str(tmp_path / "v.png")), a[:, :, 2::-1])


def test_ply_parses_back(tmp_path):
    from selfreconcode_amd.mesh_io import write_ply
    rng = np.random.default_rng(3)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (5, 3))
    p = tmp_path / "tmp.ply"
    write_ply(str(p), v, f)
    lines = p.read_text().splitlines()
    end = lines.index("end_header")
    head = lines[:end]
    assert head[:2] == ["ply", "format ascii 1.0"] and "element vertex 7" in head and "element face 5" in head
    vv = np.array([[float(t) for t in ln.split()] for ln in lines[end + 1:end + 8]], dtype=np.float32)
    ff = np.array([[int(t) for t in ln.split()] for ln in lines[end + 8:]])
    assert np.array_equal(vv, v) and ff.shape == (5, 4) and (ff[:, 0] == 3).all() and np.array_equal(ff[:, 1:], f)
