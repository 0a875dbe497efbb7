"""The edge-collapse decimation as its float64 restatement computes it (tests/_meshcollapse_ref.py; no GPU): on the UV sphere 64 x 32
and the cube of 12 x 12 quads per side, plain and jittered, the run ends exactly at its budget within 64 rounds, leaves a closed oriented
manifold of Euler characteristic 2, and lies at most half as far from the true surface as the mean-placement clustering bisected to the
same budget -- which, on the spheres, is not a manifold at all."""
import numpy as np
import pytest

import _meshcollapse_ref as mc
import _meshquadric_ref as mq

TARGETS = {"sphere": 400, "sphere_jitter": 400, "cube": 300, "cube_jitter": 300}
_RUNS = {}


def _run(name):
    if name not in _RUNS:
        v, f = mq.shape(name)
        _RUNS[name] = mc.collapse(v, f, TARGETS[name])
    return _RUNS[name]


def test_fmix32_is_murmur3s_finaliser_and_a_bijection_on_a_range():
    assert mc.fmix32(np.array([0, 1, 2, 0xffffffff])).tolist() == [0, 0x514e28b7, 0x30f4c306, 0x81f16f39]
    assert len(np.unique(mc.fmix32(np.arange(1 << 16)))) == 1 << 16


@pytest.mark.parametrize("name", mq.SHAPES)
def test_run_ends_at_the_budget_as_a_closed_oriented_manifold(name):
    v, f = mq.shape(name)
    r = _run(name)
    F0, target = len(f), TARGETS[name]
    print(f"{name}: {F0} -> {len(r['faces'])} faces in {r['rounds']} rounds, {r['collapses']} collapses")
    assert not r["stalled"] and r["rounds"] <= 64
    assert len(r["faces"]) == F0 - 2 * ((F0 - target + 1) // 2) == target and r["collapses"] == (F0 - target) // 2
    t = mc.topology(r["verts"], r["faces"])
    assert t["euler"] == 2 and t["open_edges"] == 0 and t["oriented"]
    assert t["V"] == len(v) - r["collapses"]
    vmap = r["vertex_map"]
    assert vmap.shape == (len(v),) and vmap.min() >= 0 and vmap.max() == t["V"] - 1 and len(np.unique(vmap)) == t["V"]


@pytest.mark.parametrize("name", mq.SHAPES)
def test_surface_error_is_at_most_half_the_clusterings(name):
    v, f = mq.shape(name)
    r = _run(name)
    cv, cf, cell = mc.cluster_to(v, f, TARGETS[name])
    qv, qf, _ = mc.cluster_to(v, f, TARGETS[name], placement="quadric")
    ours, mean, quad = (mq.quality(name, *m)["surface"] for m in ((r["verts"], r["faces"]), (cv, cf), (qv, qf)))
    print(f"{name}: surface error collapse {ours:.4g}, clustering at cell {cell:.4g} mean {mean:.4g} ({len(cf)} faces; ratio {ours / mean:.3g}), "
          f"quadric {quad:.4g} (ratio {ours / max(quad, 1e-300):.3g}, not bounded)")
    assert len(cf) <= TARGETS[name]
    assert ours <= 0.5 * mean
    if name.startswith("sphere"):                         # why the feature exists: the clustering of a sphere is not a manifold
        t = mc.topology(cv, cf)
        print(f"{name}: the clustering has {t['open_edges']} edges without two faces, oriented {t['oriented']}")
        assert t["open_edges"] > 0


def test_round_refuses_what_it_must():
    """A tetrahedron (valence), two tetrahedra glued on a face (link), an open strip and a fan on an edge (locked)."""
    import _meshprep_ref as mr
    tet_v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]); tet_f = np.int64([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    r = mc.round(tet_v, tet_f, mc.vertex_quadrics(tet_v, tet_f))
    assert len(r["edges"]) == 6 and not r["candidate"].any() and not r["locked"].any() and (r["keys"] == mc.INT64_MAX).all()
    for v, f in (mr.flat_strip(6), mr.fan_on_edge()):
        r = mc.round(v, f, mc.vertex_quadrics(v, f))
        assert r["locked"][np.unique(f)].all() and not r["selected"].any()
