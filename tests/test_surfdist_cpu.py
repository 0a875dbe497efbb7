"""What of the surface-distance evaluation can be checked without a GPU: the numpy restatement of tests/_surfdist_ref.py
against hand values, the stratified-count property of its sampler, the mesh readers, the command's parser, the refusal of CPU tensors
and the header."""
import os
import struct

import numpy as np
import pytest
import torch

import _meshprep_ref as mr
import _surfdist_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2 = 2. ** 0.5


# one triangle a = (0,0,0), b = (1,0,0), c = (0,1,0): a point in each of the seven Voronoi regions -> (closest, distance)
REGIONS = [((0.25, 0.25, 0.5), (0.25, 0.25, 0.), 0.5),             # interior
           ((-1., -1., 0.), (0., 0., 0.), R2),                     # vertex a
           ((2., -1., 0.), (1., 0., 0.), R2),                      # vertex b
           ((-1., 2., 0.), (0., 1., 0.), R2),                      # vertex c
           ((0.5, -1., 1.), (0.5, 0., 0.), R2),                    # edge ab
           ((1., 1., 0.), (0.5, 0.5, 0.), 0.5 ** 0.5),             # edge bc
           ((-1., 0.5, 0.), (0., 0.5, 0.), 1.)]                    # edge ca
TRI_V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.int64([[0, 1, 2]])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("prune", [False, True])
def test_restatement_seven_regions(dtype, prune):
    p = np.float32([r[0] for r in REGIONS])
    d, f, q = sr.closest(p, TRI_V, TRI_F, dtype, prune=prune)
    assert d.dtype == dtype and (f == 0).all()
    tol = 1e-12 if dtype == np.float64 else 1e-6
    assert np.abs(d - np.float64([r[2] for r in REGIONS])).max() < tol
    assert np.abs(q - np.float64([r[1] for r in REGIONS])).max() < tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_degenerate_triangles(dtype):
    """A collinear triangle is the segment it spans, a triangle with a repeated vertex its edge, a point triangle the point: no NaN."""
    verts = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 1, 1]])
    for face, p, want_d, want_q in (((0, 1, 2), (1.5, 1., 0.), 1., (1.5, 0., 0.)), ((0, 2, 1), (3., 0., 1.), R2, (2., 0., 0.)),
                                    ((0, 0, 1), (-1., 0., 0.), 1., (0., 0., 0.)), ((0, 0, 1), (0.5, 0., 2.), 2., (0.5, 0., 0.)),
                                    ((3, 3, 3), (1., 1., 3.), 2., (1., 1., 1.))):
        d, f, q = sr.closest(np.float32([p]), verts, np.int64([face]), dtype)
        assert np.isfinite(d).all() and np.isfinite(q).all()
        assert abs(d[0] - want_d) < 1e-6 and np.abs(q[0] - np.float64(want_q)).max() < 1e-6, (face, p, d, q)


def test_restatement_pruned_equals_exhaustive():
    """The candidate selection drops no face that holds the minimum: both paths give the same bits, ties (the mesh's own vertices)
    included."""
    from selfreconcode_amd.synthetic import cube_sphere
    v, f = [x.numpy() for x in cube_sphere(6)]
    v = mr.jitter(v, 3, 0.004)
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.normal(size=(150, 3)) * 0.7, v[:60], 20. * rng.normal(size=(20, 3)), 1e-3 * rng.normal(size=(10, 3))]).astype(np.float32)
    for dtype in (np.float64, np.float32):
        a, b = sr.closest(p, v, f, dtype, prune=False), sr.closest(p, v, f, dtype, prune=True)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    d, f_hit, q = sr.closest(p, v, f)
    assert np.abs(sr.face_distance(p, v, f, f_hit) - d).max() == 0.
    assert np.abs(np.linalg.norm(p.astype(np.float64) - q, axis=1) - d).max() < 1e-12
    assert d[150:210].max() < 1e-15


@pytest.mark.parametrize("n", [4099, 100003])
def test_restatement_sampler_is_stratified(n):
    """Every face receives its share of the samples to within 2: |count - n a_f / A| < 2 (a face's interval of the cumulative area
    cuts at most two strata)."""
    from selfreconcode_amd.synthetic import cube_sphere
    v, f = [x.numpy() for x in cube_sphere(32)]
    v = mr.jitter(v, 5, 0.004)
    f = np.concatenate([f[:100], np.int64([[7, 7, 9]]), f[100:]])                 # a face without area in the middle
    cum = sr.face_areas_cum(v, f)
    pts, face, nrm = sr.sample(cum, v, f, n, 11)
    area = np.diff(cum, prepend=0.)
    dev = np.abs(np.bincount(face, minlength=len(f)) - n * area / cum[-1])
    print(f"n {n}: max |count - expected| {dev.max():.3f}")
    assert dev.max() < 2. and not (face == 100).any()
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.).max() < 1e-12
    assert sr.face_distance(pts, v, f, face).max() < 1e-7                          # (on their faces)
    again = sr.sample(cum, v, f, n, 11)
    assert all(np.array_equal(x, y) for x, y in zip((pts, face, nrm), again))
    assert not np.array_equal(sr.sample(cum, v, f, n, 12)[0], pts)


# ---------------------------------------------------------------------------------------------------------------- mesh_io
def _small_mesh():
    from selfreconcode_amd.synthetic import icosphere
    v, f = icosphere(1)
    return v.numpy(), f.numpy()


def test_ply_ascii_round_trip(tmp_path):
    from selfreconcode_amd.mesh_io import read_mesh, read_ply, write_ply
    v, f = _small_mesh()
    path = str(tmp_path / "m.ply")
    write_ply(path, v, f)
    v2, f2 = read_ply(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int64
    assert np.array_equal(v2, v) and np.array_equal(f2, f)                         # (%.9g round-trips a float32)
    v3, f3 = read_mesh(path)
    assert np.array_equal(v3, v) and np.array_equal(f3, f)


def _binary_ply(path, v, faces, index_name="vertex_indices"):
    head = ("ply\nformat binary_little_endian 1.0\ncomment made by a test\nelement vertex %d\nproperty double x\nproperty double y\n"
            "property uchar red\nproperty double z\nelement face %d\nproperty list uchar int %s\nend_header\n" % (len(v), len(faces), index_name))
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        for i, p in enumerate(v.tolist()):
            fh.write(struct.pack("<ddBd", p[0], p[1], i % 256, p[2]))
        for t in faces:
            fh.write(struct.pack("<B%di" % len(t), len(t), *t))


@pytest.mark.parametrize("index_name", ["vertex_indices", "vertex_index"])
def test_ply_binary_double_with_extra_property(tmp_path, index_name):
    from selfreconcode_amd.mesh_io import read_ply
    v, f = _small_mesh()
    v = v.astype(np.float64) + 1e-11                                               # (not representable in float32)
    path = str(tmp_path / "b.ply")
    _binary_ply(path, v, f.tolist(), index_name)
    v2, f2 = read_ply(path)
    assert v2.dtype == np.float64 and np.array_equal(v2, v) and np.array_equal(f2, f)


def test_quads_are_refused(tmp_path):
    from selfreconcode_amd.mesh_io import read_obj, read_ply
    v, _ = _small_mesh()
    path = str(tmp_path / "q.ply")
    _binary_ply(path, v.astype(np.float64), [[0, 1, 2], [0, 1, 2, 3]])
    with pytest.raises(ValueError):
        read_ply(path)
    asc = tmp_path / "q_ascii.ply"
    asc.write_text("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                   "property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError):
        read_ply(str(asc))
    obj = tmp_path / "q.obj"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    with pytest.raises(ValueError):
        read_obj(str(obj))
    big = tmp_path / "be.ply"
    big.write_text("ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError):
        read_ply(str(big))


def test_obj_corners_and_negative_indices(tmp_path):
    from selfreconcode_amd.mesh_io import read_mesh, read_obj
    obj = tmp_path / "m.obj"
    obj.write_text("# a comment\nv 0 0 0\nv 1 0 0 0.5 0.5 0.5\nvt 0 0\nvn 0 0 1\nv 0 1 0\nf 1/1/1 2/1/1 3/1/1\nv 0 0 1.5\nf -1 -4//1 2/1\ng part\nf 4 -2 -3\n")
    v, f = read_obj(str(obj))
    assert v.dtype == np.float64 and f.dtype == np.int64
    assert np.array_equal(v, np.float64([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]]))
    assert np.array_equal(f, np.int64([[0, 1, 2], [3, 0, 1], [3, 2, 1]]))
    assert np.array_equal(read_mesh(str(obj))[1], f)
    with pytest.raises(ValueError):
        read_mesh(str(tmp_path / "m.stl"))


# ---------------------------------------------------------------------------------------------------------------- command, refusals
def test_parser_modes():
    from selfreconcode_amd.evaluate import build_parser, parse_args
    a = parse_args(["--pred", "a.ply", "--gt", "b.obj", "--samples", "1000", "--tau", "0.01", "0.02", "--out", "m.json"])
    assert (a.pred, a.gt, a.samples, a.tau, a.seed, a.gpu_ids, a.out) == ("a.ply", "b.obj", 1000, [0.01, 0.02], 0, [0], "m.json")
    a = parse_args(["--gpu-ids", "1", "--rec-root", "R", "--gt-root", "G", "--frames", "5"])
    assert (a.rec_root, a.gt_root, a.frames, a.samples, a.gpu_ids) == ("R", "G", 5, 1_000_000, [1])
    for argv in ([], ["--samples", "10"], ["--pred", "a.ply", "--gt", "b.ply", "--rec-root", "R", "--gt-root", "G"], ["--pred", "a.ply"],
                 ["--rec-root", "R"], ["--pred", "a.ply", "--gt-root", "G"], ["--pred", "a.ply", "--gt", "b.ply", "--samples", "0"]):
        with pytest.raises(SystemExit):
            parse_args(argv)
    text = " ".join(build_parser().format_help().split())
    assert "No alignment and no scaling" in text


def test_cpu_tensors_are_refused():
    from selfreconcode_amd import evaluate, surfdist_ops as sd
    v, f = torch.from_numpy(TRI_V), torch.from_numpy(TRI_F)
    with pytest.raises(RuntimeError):
        sd.closest_point(torch.zeros(4, 3), None)
    with pytest.raises(RuntimeError):
        sd.MeshIndex.build(v, f)
    with pytest.raises(RuntimeError):
        sd.sample_surface(v, f, 10, 0)
    with pytest.raises(RuntimeError):
        sd.face_areas_cum(v, f)
    with pytest.raises(RuntimeError):
        evaluate.surface_metrics((v, f), (v, f), 10)
    with pytest.raises(RuntimeError):
        evaluate.vertex_to_surface(v, (v, f))


def test_header_declares_the_entries():
    txt = open(os.path.join(ROOT, "include", "selfrecon_hip.h")).read()
    for name in ("sr_surfdist_face_cells", "sr_surfdist_emit_pairs", "sr_surfdist_query", "sr_surfdist_brute", "sr_mesh_sample"):
        assert ("int %s(" % name) in txt, name
