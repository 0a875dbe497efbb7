"""The volumes of tests/_mc_volumes.py reach the launch paths of csrc/mc.hip they are built for, and the sequential oracle behaves on
them as the GPU comparison of tests/test_mc_paths_gpu.py assumes: what keeps that file honest.  No GPU is needed here.

The launch plan (_mc_volumes.launch_plan) restates the host arithmetic of sr_mc_count / sr_mc_emit; its four constants are tied to
the source text below, so a changed constant fails here and does not silently move the edges the shapes sit on."""
import os
import re
import numpy as np
import pytest

import _mc_volumes as mv
from oracle import mc as mco
from oracle.fixtures import digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "selfreconcode_amd", "csrc")
PINS = os.path.join(ROOT, "tests", "golden", "ref_pins.npz")
MAX_NAN = 0.05                    # of the oracle's vertex coordinates: what the GPU comparison may hold to "NaN too" instead of to the bits


# ------------------------------------------------------------------------------------------------ the launch plan
def test_the_plan_constants_are_the_kernels():
    with open(os.path.join(CSRC, "mc.hip")) as fh:
        mc = fh.read()
    with open(os.path.join(CSRC, "sr_common.h")) as fh:
        common = fh.read()
    for name, value in (("MC_CHUNK", mv.MC_CHUNK), ("MC_BATCH", mv.MC_BATCH), ("SCAN_ITEMS", mv.SCAN_ITEMS)):
        (found,) = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, mc)
        assert int(found) == value, name
    (body,) = re.findall(r"static inline int sr_stream_grid\(int64_t work_items, int block\)\s*\{(.*?)\n\}", common, re.S)
    (cap, cap2) = re.findall(r"if \(g > (\d+)\) g = (\d+);", body)[0]
    assert int(cap) == int(cap2) == mv.GRID_CAP
    # the shape of the launches the plan restates: a wave per chunk in blocks of 256 rounded up to the 8 XCDs, 8 threads per group for emit
    assert "sr_stream_grid(sr_cdiv(L.G, MC_CHUNK) * 64, 256) + 7) & ~7" in mc
    assert "sr_stream_grid(L.G * 8 < (int64_t)1 << 22 ? L.G * 8 : (int64_t)1 << 22, 256)" in mc
    assert "(nchunks + 7) / 8" in mc and "blockIdx.x & 7" in mc


# shape -> (total, G, chunks) of the table in tests/test_mc_paths_gpu.py
TABLE = {
    (1, 1, 1): (1, 1, 1), (1, 5, 7): (35, 1, 1), (5, 1, 7): (35, 1, 1), (5, 7, 1): (35, 1, 1),
    (2, 2, 2): (8, 1, 1), (3, 3, 3): (27, 1, 1), (4, 4, 4): (64, 1, 1),
    (9, 2, 2): (36, 1, 1), (40, 3, 5): (600, 10, 1),
    (7, 5, 63): (2205, 35, 3), (7, 5, 64): (2240, 35, 3), (7, 5, 65): (2275, 36, 3),
    (3, 3, 255): (2295, 36, 3), (3, 3, 256): (2304, 36, 3), (3, 3, 257): (2313, 37, 3),
    (3, 2, 1030): (6180, 97, 7),
    (7, 31, 33): (7161, 112, 7), (8, 32, 32): (8192, 128, 8), (8, 32, 33): (8448, 132, 9),
    (23, 89, 64): (131008, 2047, 128), (32, 64, 64): (131072, 2048, 128), (33, 41, 97): (131241, 2051, 129),
    (131, 257, 251): (8450417, 132038, 8253),
}


def test_every_shape_of_the_table_is_a_volume_and_has_the_listed_plan():
    shapes = {shape for shape, kind, _, _ in mv.VOLUMES.values() if kind in ("dense", "shell")}
    assert shapes == set(TABLE)
    for shape, (total, G, chunks) in TABLE.items():
        p = mv.launch_plan(shape)
        assert (p["total"], p["G"], p["chunks"]) == (total, G, chunks), shape
        assert sum(p["ranges"]) == chunks and p["grid"] % 8 == 0 and p["grid"] <= mv.GRID_CAP + 7
        print("%-16s total %-8d G %-7d chunks %-5d per_xcd %-5d empty XCD ranges %d  grid %-5d waves/XCD %-5d scan blocks %d" % (
            shape, total, G, chunks, p["per_xcd"], p["empty_xcds"], p["grid"], p["waves_per_xcd"], p["scan_blocks"]))


def _plans(*shapes):
    return [mv.launch_plan(s) for s in shapes]


def test_axis_of_one_and_single_group_shapes():
    for shape in ((1, 1, 1), (1, 5, 7), (5, 1, 7), (5, 7, 1)):
        p = mv.launch_plan(shape)
        assert min(shape) == 1 and p["G"] == 1 and mv.cube_cases(mv.dense(shape)).size == 0            # no cell at all
    a, b, c = _plans((2, 2, 2), (3, 3, 3), (4, 4, 4))
    assert a["total"] < 64 and b["total"] < 64 and c["total"] == 64 and c["tail"] == 0
    for p in (a, b, c):
        assert p["G"] == 1 and p["empty_xcds"] == 7 and p["ranges"][0] == 1


def test_small_planes_put_several_i_planes_in_a_group():
    """NY*NZ < 64: the carry `while (nk >= d.NZ)` wraps more than once per 64-voxel step and steps i as well as j."""
    a, b = _plans((9, 2, 2), (40, 3, 5))
    assert a["planes_per_group"] == 16 and b["planes_per_group"] > 4 and a["rows_per_group"] == 32 and b["rows_per_group"] > 12
    assert b["G"] % mv.MC_BATCH == 2 and b["chunks"] == 1
    assert mv.launch_plan((5, 7, 1))["rows_per_group"] == 64


def test_row_ends_against_group_ends():
    """NZ = 63 / 64 / 65: lane 63's k+1 neighbour is lane 0 of the next group except where the row ends with the group."""
    a, b, c = _plans((7, 5, 63), (7, 5, 64), (7, 5, 65))
    assert (a["tail"], b["tail"], c["tail"]) == (29, 0, 35)
    assert a["G"] % mv.MC_BATCH == 3 and b["G"] % mv.MC_BATCH == 3 and c["G"] % mv.MC_BATCH == 0
    assert a["rows_per_group"] > 1 and b["rows_per_group"] == 1 and c["rows_per_group"] < 1
    # NZ = 255 / 256 / 257: a batch of MC_BATCH groups (256 voxels) lies inside one row, is one row, is one voxel short of one
    for shape in ((3, 3, 255), (3, 3, 256), (3, 3, 257)):
        p = mv.launch_plan(shape)
        assert abs(shape[2] - 64 * mv.MC_BATCH) <= 1 and p["chunks"] == 3 and p["empty_xcds"] == 5
    assert mv.launch_plan((3, 3, 257))["G"] % mv.MC_BATCH == 1


def test_chunks_against_the_eight_xcd_ranges():
    long_row = mv.launch_plan((3, 2, 1030))
    assert 1030 > 64 * mv.MC_CHUNK and long_row["chunks"] == 7 and long_row["empty_xcds"] == 1
    a, b, c = _plans((7, 31, 33), (8, 32, 32), (8, 32, 33))
    assert a["ranges"] == [1] * 7 + [0]
    assert b["ranges"] == [1] * 8
    assert c["per_xcd"] == 2 and c["ranges"] == [2, 2, 2, 2, 1, 0, 0, 0]
    assert c["G"] % mv.MC_CHUNK == 4                                    # and the last chunk is a short one (4 of 16 groups)


def test_scan_lengths_sit_on_the_block_edge():
    a, b, c = _plans((23, 89, 64), (32, 64, 64), (33, 41, 97))
    assert a["scan_n"] == mv.SCAN_ITEMS and a["scan_blocks"] == 1
    assert b["scan_n"] == mv.SCAN_ITEMS + 1 and b["scan_blocks"] == 2   # the second block holds the sentinel off[G] alone
    assert c["scan_n"] == mv.SCAN_ITEMS + 4 and c["scan_blocks"] == 2
    for name in ("dense_23x89x64", "dense_32x64x64", "dense_33x41x97"):
        v, _, f = mv.reference(name)
        p = mv.launch_plan(mv.VOLUMES[name][0])
        # dense: the per-output kernels launch G * 8 threads for about 1.4 / 3 outputs per voxel -- they grid-stride many times
        assert len(v) > 10 * p["out_threads"] and len(f) > 20 * p["out_threads"]


def test_the_big_shell_caps_every_grid():
    p = mv.launch_plan(mv.BIG_SHELL)
    assert p["grid"] == mv.GRID_CAP and p["waves_per_xcd"] == 1024 and p["per_xcd"] == 1032 and p["second_chunk"]
    assert p["empty_xcds"] == 0 and p["ranges"][-1] == 8253 - 7 * 1032
    assert p["scan_blocks"] == 65 and p["out_grid"] == mv.GRID_CAP and p["tag_grid"] == -(-p["G"] // 256) < mv.GRID_CAP
    assert not any(mv.launch_plan(s)["second_chunk"] for s in TABLE if s != mv.BIG_SHELL)
    v, _, f = mv.reference("shell_131x257x251")
    assert len(v) > 50_000 and f.min() >= 0                             # a closed shell well inside the volume


# ------------------------------------------------------------------------------------------------ case coverage
def test_all_256_cases_occur():
    s = mv.all_cases()
    p = mv.ALL_CASES_PITCH
    assert p >= 4 and s.shape == mv.ALL_CASES_SHAPE
    cases = mv.cube_cases(s)
    assert len(np.unique(cases)) == 256
    assert np.array_equal(cases[1::p, 1::p, 1::p].ravel(), np.arange(256))          # block n's own cell has case n
    assert (np.abs(s) >= np.float32(0.1)).all() and (np.abs(s) < np.float32(1.1)).all()
    neg = np.argwhere(s < 0)
    assert ((neg % p >= 1) & (neg % p <= 2)).all()                      # nothing negative outside the blocks
    assert len(np.unique(mv.cube_cases(mv.dense((64, 80, 48))))) == 256
    half = (mv.dense((64, 80, 48)) < 0).mean()
    assert 0.49 < half < 0.51


# ------------------------------------------------------------------------------------------------ the oracle on every volume
def _unowned_edge_is_crossed(s, iso):
    """True when some crossed lattice edge starts on a far face of the volume: no cell owns it, faces that use it get -1."""
    neg = s < np.float32(iso)
    NX, NY, NZ = s.shape
    x = neg[:-1] != neg[1:]; y = neg[:, :-1] != neg[:, 1:]; z = neg[:, :, :-1] != neg[:, :, 1:]
    # a crossed edge is used by a face only if a CELL contains it: the other two axes must have a cell (length >= 2)
    if min(NX, NY, NZ) < 2:
        return False
    return bool(x[:, -1, :].any() or x[:, :, -1].any() or y[-1].any() or y[:, :, -1].any() or z[-1].any() or z[:, -1].any())


@pytest.mark.parametrize("name", list(mv.VOLUMES))
def test_oracle_self_checks(name):
    shape, kind, iso, _ = mv.VOLUMES[name]
    NX, NY, NZ = shape
    s = mv.volume(name)
    assert s.dtype == np.float32 and s.shape == shape
    assert np.array_equal(s.view(np.uint32), mv.volume(name).view(np.uint32))       # a pure function of the name
    v, k, f = mv.reference(name)
    V, F = len(v), len(f)
    print("%-28s iso %-5r V %-7d F %-7d faces with a -1: %d" % (name, iso, V, F, (f < 0).any(1).sum()))
    assert (np.diff(k) > 0).all()                                       # one vertex per lattice edge
    assert f.size == 0 or (f.min() >= -1 and f.max() < V)
    # the vertex set IS the set of crossed lattice edges owned by an interior cell
    neg = s < np.float32(iso)
    own = np.zeros(shape + (3,), bool)
    if min(shape) >= 2:
        own[:-1, :-1, :-1, 0] = neg[:-1, :-1, :-1] != neg[1:, :-1, :-1]
        own[:-1, :-1, :-1, 1] = neg[:-1, :-1, :-1] != neg[:-1, 1:, :-1]
        own[:-1, :-1, :-1, 2] = neg[:-1, :-1, :-1] != neg[:-1, :-1, 1:]
    assert np.array_equal(k, np.nonzero(own.ravel())[0])
    # -1 only where an axis border is involved: present exactly when an unowned edge is crossed, and a face that has one lies in the last
    # layer of cells -- its other vertices sit on lattice edges whose origin is within one step of a far face
    has = (f < 0).any(1) if F else np.zeros(0, bool)
    assert has.any() == _unowned_edge_is_crossed(s, iso)
    if has.any() and V:
        cell = k[np.clip(f[has], 0, None)] // 3
        bi, bj, bk = cell // (NY * NZ), cell // NZ % NY, cell % NZ
        near = (bi >= NX - 2) | (bj >= NY - 2) | (bk >= NZ - 2)
        assert (near | (f[has] < 0)).all()
    if name in mv.AXIS_OF_ONE or (kind == "ties" and iso == -1.0):
        assert V == 0 and F == 0
    elif kind in ("dense", "ties", "nonfinite"):
        assert V > 0 and F > V
    if kind == "ties":
        assert (s == np.float32(iso)).mean() > 0.25 and set(np.unique(s)) == {-1.0, 0.0, 1.0}    # a third of the samples equal iso
    if name == mv.FAR_CORNER:
        assert V == 0 and F == 1 and (f == -1).all()
    nan = float(np.isnan(v).mean()) if V else 0.0
    if kind == "nonfinite":
        plants = mv.nonfinite_plants(shape)
        assert sum(np.isnan(p[3]) for p in plants) == 1 and sum(np.isinf(p[3]) for p in plants) == 2 and len(plants) == 9
        for a, p in enumerate(plants):                                  # away from each other: only a +-3e38 pair is adjacent
            for q in plants[a + 1:]:
                d = max(abs(p[0] - q[0]), abs(p[1] - q[1]), abs(p[2] - q[2]))
                assert d >= 2 or (d == 1 and p[3] == -q[3] == 3e38), (p, q)
        # between a +3e38 and a -3e38 sample v2 - v1 overflows to inf: t = 0, the vertex sits ON the edge's first sample -- the cell's origin
        # for the x and z edges, the far end (j + 1) for the y edge, which runs towards the origin.  (lattice * step + origin is exact in
        # float64 here, so one rounding to float32 is the fused multiply-add)
        for a, b in zip(plants[3::2], plants[4::2]):
            axis = [a[n] != b[n] for n in range(3)].index(True)
            o = [min(a[n], b[n]) for n in range(3)]
            (row,) = np.nonzero(k == ((o[0] * NY + o[1]) * NZ + o[2]) * 3 + axis)[0]
            lattice = o[axis] + (1 if axis == 1 else 0)
            assert v[row, axis] == np.float32(lattice * np.float64(np.float32(mv.STEP[axis])) + np.float64(np.float32(mv.ORG[axis])))
        print("%-28s NaN coordinates %.3f %% (cap %.0f %%), infinite %d" % (name, 100 * nan, 100 * MAX_NAN, np.isinf(v).sum()))
        assert 0 < nan <= MAX_NAN
    else:
        assert nan == 0.0


@pytest.mark.parametrize("shape", mv.SPECIAL_SHAPES)
def test_denormal_crossings_lie_at_two_thirds(shape):
    """Unit steps, zero origin: the moving coordinate of every vertex is n + 1/3 or n + 2/3 -- a third of the edge from the -1e-45
    sample, offset 2/3 from the 3e-45 one.  0.5 (delta flushed to zero) or no vertex at all would mean the denormals were lost."""
    s = mv.denormal(shape)
    assert set(np.unique(s.view(np.uint32))) == {mv.DENORM_POS, mv.DENORM_NEG}
    assert s.max() > 0 and s.max() < 2.0 ** -126 and s.min() < 0        # denormal, not flushed by numpy
    v, k, f = mco.canonical(*mco.marching_cubes(s, full=True))
    assert len(v) > 100 or shape == (40, 3, 5) and len(v) > 50
    cell, d = k // 3, k % 3
    base = np.stack([cell // (shape[1] * shape[2]), cell // shape[2] % shape[1], cell % shape[2]], 1)
    negative_first = s.ravel()[cell] < 0                                # the edge's origin sample is the negative one
    # t = (float)(d / 3d) or (float)(2d / 3d) in double; the x and z edges run from the cell's origin (t from there), the y edge -- cube
    # edge 3 -- runs TOWARDS it, so its t is measured from the far end and the coordinate is j + (1 + -t): all in float32, as the kernels do
    third, two_thirds, one = np.float32(1.0 / 3.0), np.float32(2.0 / 3.0), np.float32(1.0)
    t_xz = np.where(negative_first, third, two_thirds)
    t_y = np.where(negative_first, two_thirds, third)
    expect = base.astype(np.float32)
    rows = np.arange(len(v))
    expect[rows, d] = np.where(d == 1, expect[rows, d] + (one + -t_y), expect[rows, d] + (np.float32(0.0) + t_xz))
    assert expect.dtype == np.float32 and np.array_equal(v.view(np.uint32), expect.view(np.uint32))
    frac = v[rows, d].astype(np.float64) - base[rows, d]
    assert (np.abs(frac - np.where(negative_first, 1 / 3, 2 / 3)) < 4e-6).all() and (np.abs(frac - 0.5) > 0.1).all()    # (float32 ulp at 64 is 7.6e-6)


# ------------------------------------------------------------------------------------------------ capacity
def test_default_capacity_is_unchanged_and_full_capacity_cannot_overflow():
    from test_mc_seg3d_gpu import _field
    s = _field((24, 24, 24), "noisy")
    assert mco.capacity(s.size) == (max(1024, int(s.size * 0.5)), 2 * max(1024, int(s.size * 0.5)))
    assert mco.capacity(8) == (1024, 2048) and mco.capacity(8, full=True) == (1024, 2048)
    assert mco.capacity(10 ** 6, full=True) == (3 * 10 ** 6, 5 * 10 ** 6)
    old = mco.marching_cubes(s, mv.STEP, mv.ORG, 0.0)
    full = mco.marching_cubes(s, mv.STEP, mv.ORG, 0.0, full=True)
    assert len(old[0]) > 1000
    for a, b in zip(old, full):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    g = np.load(os.path.join(ROOT, "tests", "golden", "mc_ref.npz"))   # ... and the arrays frozen before the capacity argument existed
    from test_mc_reference_pin import field
    for a, b in zip(mco.canonical(*mco.marching_cubes(field((24, 24, 24), "noisy"), mv.STEP, mv.ORG, 0.0)), (g["v2"], g["k2"], g["f2"])):
        assert np.array_equal(a, b)
    with pytest.raises(AssertionError):                                 # what the default did, and does, on white noise
        mco.marching_cubes(mv.dense((7, 5, 63)))


# ------------------------------------------------------------------------------------------------ the case table itself
def test_all_cases_equal_the_reference_kernels():
    """oracle/mc_oracle.c includes the product's mc_tables.h: the oracle and the HIP kernels share one case table, and only the
    reference's own kernels can catch a wrong row of it.  Live where their host build exists or can be made; the digests frozen by
    oracle/gen_ref_pins_golden.py hold everywhere."""
    vo, ko, fo = mv.reference(mv.ALL_CASES)
    assert fo.min() >= 0
    g = np.load(PINS)
    for x, n in zip((vo, ko, fo), "vkf"):
        assert digest(x) == g["mc_all_cases_" + n], n
    if mco.reference_available():
        s = mv.volume(mv.ALL_CASES)
        for mode in ("fma", "nofma"):
            vr, kr, fr = mco.canonical(*mco.reference_marching_cubes(s, mv.STEP, mv.ORG, 0.0, mode))
            assert np.array_equal(kr, ko) and np.array_equal(fr, fo)
            if mode == "fma":
                assert np.array_equal(vr.view(np.uint32), vo.view(np.uint32))
