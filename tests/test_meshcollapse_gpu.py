"""Edge-collapse decimation on the GPU (csrc/mesh_collapse.hip; mesh_prep_ops.collapse_round / collapse_apply; mesh_prep.simplify_collapse)
against the float64 restatement of tests/_meshcollapse_ref.py, round by round and as whole runs.

Tolerances.  Edges, the selection, the applied faces and the map are integers: exact.  A position is a double result rounded once to
float32, so product and restatement may differ by one rounding: 2^-23 max |coordinate|.  The cost is compared as decoded from the key:
float32 rounding, 2^-23 cost, plus 256 2^-53 (x^T |A| x + 2 |b|^T |x| + |c|) for the double evaluation (the kernel contracts products
into fused multiply-adds, the restatement does not; some 20 operations, so 256 roundings of the largest partial sum is a wide
margin, not a fitted one).  Where the two float32 positions of an edge are not the same bits -- the double optimum lay within a solve's
error of a float32 tie -- the restated cost is evaluated at the product's position: the bound is about the cost function, and the
position has its own check.  The candidate sets are compared outside the edges whose tightest restated flip test lies within 1e-9 of
the threshold (at most 1 % of the edges, none on the plain shapes)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import _meshcollapse_ref as mc
import _meshprep_ref as mr
import _meshquadric_ref as mq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX = mc.INT64_MAX
TARGETS = {"sphere": 400, "sphere_jitter": 400, "cube": 300, "cube_jitter": 300}
_RUNS = {}


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _small(name):
    v, f = mq.uv_sphere(32, 16) if name.startswith("sphere") else mq.cube(6)
    return (mr.jitter(v, 7, 0.002) if name.endswith("jitter") else v), f


def _run(name):
    """One whole run of the product per shape (and a second one, for the bits), computed once."""
    from selfreconcode_amd.mesh_prep import simplify_collapse
    if name not in _RUNS:
        v, f = mq.shape(name)
        rep = {}
        mesh = simplify_collapse(_t(v), _t(f), TARGETS[name], report=rep)
        _RUNS[name] = dict(v=v, f=f, mesh=mesh, rep=rep, again=simplify_collapse(_t(v), _t(f), TARGETS[name]))
    return _RUNS[name]


def _cost_of(keys):
    return (keys >> 32).astype(np.int32).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("name", mq.SHAPES)
def test_three_rounds_vs_restatement(name):
    from selfreconcode_amd import mesh_prep_ops as mp
    v, f = _small(name)
    tv, tf = _t(v), _t(f)
    V = len(v)
    Q = mp.vertex_quadrics(tv, tf)
    Qr = mc.vertex_quadrics(v, f)
    n, w, d, ok = mq.face_planes(v.astype(np.float64), f)
    S = np.zeros(V)
    np.add.at(S, f.reshape(-1), np.repeat(w * np.maximum(1., np.abs(d)) ** 2, 3))
    assert (np.abs(Q.cpu().numpy() - Qr) <= 64 * 2. ** -52 * S[:, None]).all()       # (<= 32 faces per vertex, a few roundings per term)
    for rnd in range(3):
        edges, keys, pos, sel = mp.collapse_round(tv, tf, Q)
        hv, hf, hQ = tv.cpu().numpy(), tf.cpu().numpy(), Q.cpu().numpy()
        ref = mc.round(hv, hf, hQ)
        e, k, p, s = edges.cpu().numpy(), keys.cpu().numpy(), pos.cpu().numpy(), sel.cpu().numpy()
        assert np.array_equal(e, ref["edges"]) and k.dtype == np.int64 and s.dtype == bool and (k >= 0).all()
        E, cand = len(e), k != MAX
        near = ref["margin"] <= 1e-9
        assert near.sum() <= 0.01 * E and (near.sum() == 0 or name.endswith("jitter"))
        assert np.array_equal(cand[~near], ref["candidate"][~near]) and cand.sum() > 0
        assert np.array_equal(k[cand] & 0xffffffff, mc.fmix32(np.arange(E))[cand])
        assert (np.abs(p.astype(np.float64) - ref["x"]) <= 2. ** -23 * np.abs(ref["x"]).max()).all()
        same = (p.view(np.int32) == ref["positions"].view(np.int32)).all(1)
        value, scale = mc.cost_terms(ref["quadric"], p.astype(np.float64))
        want = np.where(same, ref["cost"], np.maximum(value, 0.))
        err = np.abs(_cost_of(k) - want)[cand]
        bound = (2. ** -23 * want + 256 * 2. ** -53 * scale)[cand]
        print(f"{name} round {rnd}: {E} edges, {cand.sum()} candidates, {s.sum()} selected, {near.sum()} near the flip threshold, {(~same).sum()} positions "
              f"off by a rounding, cost error / bound at most {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
        assert (err <= bound).all()
        assert np.array_equal(s, mc.select(e, k, V)) and s.sum() > 0                  # the min rule, on the product's own keys
        ends = e[s].reshape(-1)
        assert len(np.unique(ends)) == len(ends)
        nv, nf, nQ, nt = mc.apply(hv, hf, hQ, e, p, s)
        tgt = torch.arange(V, dtype=torch.int64, device=DEV)
        tf = mp.collapse_apply(tv, tf, Q, tgt, edges, pos, sel)
        assert np.array_equal(tf.cpu().numpy(), nf) and len(nf) == len(hf) - 2 * s.sum()
        assert np.array_equal(tv.cpu().numpy().view(np.int32), nv.view(np.int32)) and np.array_equal(tv[edges[sel][:, 0]].cpu().numpy().view(np.int32), p[s].view(np.int32))
        assert np.array_equal(Q.cpu().numpy(), nQ) and np.array_equal(tgt.cpu().numpy(), nt)
    assert mc.topology(v, tf.cpu().numpy())["open_edges"] == 0


def _keys(v, f, flip_cos=0.2):
    from selfreconcode_amd import mesh_prep_ops as mp
    tv, tf = _t(np.float32(v)), _t(np.int64(f))
    edges, keys, pos, sel = mp.collapse_round(tv, tf, mp.vertex_quadrics(tv, tf), flip_cos=flip_cos)
    return edges.cpu().numpy(), keys.cpu().numpy(), pos.cpu().numpy(), sel.cpu().numpy()


def test_refusals_by_valence_and_by_the_link_condition():
    """flip_cos = -1 switches the flip test off (no cosine is below -1), so what is refused here is refused by the topology alone."""
    tet_v = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]; tet_f = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]
    e, k, _, s = _keys(tet_v, tet_f, -1.)
    assert len(e) == 6 and (k == MAX).all() and not s.any()            # link holds (the two other vertices are the opposite ones); val 3 + 3 - 4 < 3
    # two tetrahedra glued on a face (the face itself removed): every edge of the glued triangle has three common neighbours
    bi_v = [[1, 0, 0], [-0.5, 0.9, 0], [-0.5, -0.9, 0], [0, 0, 1], [0, 0, -1]]
    bi_f = [[0, 1, 3], [1, 2, 3], [2, 0, 3], [1, 0, 4], [2, 1, 4], [0, 2, 4]]
    e, k, _, _ = _keys(bi_v, bi_f, -1.)
    waist = (e < 3).all(1)
    assert waist.sum() == 3 and (k[waist] == MAX).all() and np.array_equal(k != MAX, mc.round(np.float32(bi_v), np.int64(bi_f), mc.vertex_quadrics(bi_v, bi_f), flip_cos=-1.)["candidate"])
    # the link condition on its own: rings of three vertices, every valence 6 around ring 2 (vertices 7, 8, 9), whose edges have the third
    # ring vertex as a third common neighbour
    v, f = mq.uv_sphere(3, 6)
    e, k, _, _ = _keys(v, f, -1.)
    ref = mc.round(v, f, mc.vertex_quadrics(v, f), flip_cos=-1.)
    ring = ((e >= 7) & (e <= 9)).all(1)
    val = np.bincount(e.reshape(-1))
    assert ring.sum() == 3 and (val[4:13] == 6).all() and (k[ring] == MAX).all() and np.array_equal(k != MAX, ref["candidate"]) and (k != MAX).sum() > 0


def test_locked_boundary_and_non_manifold_edges():
    from selfreconcode_amd.mesh_prep import simplify_collapse
    for v, f in (mr.flat_strip(6), mr.fan_on_edge()):
        e, k, _, s = _keys(v, f)
        assert (k == MAX).all() and not s.any()
        rep = {}
        tv = _t(np.float32(v))
        mesh = simplify_collapse(tv, _t(f), 2, report=rep)
        assert rep["stalled"] and rep["rounds"] == 1 and rep["collapses"] == 0 and rep["locked_vertices"] == len(v) and rep["candidates_first"] == 0
        assert torch.equal(mesh.verts.view(torch.int32), tv.view(torch.int32)) and np.array_equal(mesh.faces.cpu().numpy(), f)
        assert mesh.vertex_map.tolist() == list(range(len(v)))
    # a grid with an interior: the interior collapses, nothing on the boundary moves
    v, f = mq.flat_grid(9)
    rep = {}
    mesh = simplify_collapse(_t(v), _t(f), 64, report=rep)
    ring = np.nonzero((v[:, 0] == 0) | (v[:, 0] == 8) | (v[:, 1] == 0) | (v[:, 1] == 8))[0]
    vm = mesh.vertex_map.cpu().numpy()
    assert rep["locked_vertices"] == len(ring) == 32 and rep["collapses"] > 0 and mesh.faces.shape[0] == 128 - 2 * rep["collapses"]
    assert np.array_equal(mesh.verts.cpu().numpy()[vm[ring]].view(np.int32), v[ring].view(np.int32)) and len(np.unique(vm[ring])) == 32
    assert (mesh.verts[:, 2] == 0).all()


def test_a_fold_only_the_flip_test_refuses():
    """A height field over the 6 x 6 grid, rough enough that moving some edge's ends to its optimum turns a face by more than acos 0.2:
    such an edge is a candidate at flip_cos = -0.99 (so the topology lets it through) and none at 0.2."""
    v, f = mq.flat_grid(6)
    inner = (v[:, 0] > 0) & (v[:, 0] < 5) & (v[:, 1] > 0) & (v[:, 1] < 5)
    v = v.copy()
    v[inner, 2] += np.random.default_rng(6).uniform(-0.6, 0.6, int(inner.sum())).astype(np.float32)
    Q = mc.vertex_quadrics(v, f)
    loose, tight = mc.round(v, f, Q, flip_cos=-0.99), mc.round(v, f, Q, flip_cos=0.2)
    only = loose["candidate"] & ~tight["candidate"]
    assert only.sum() >= 1 and (tight["margin"] > 1e-3).all() and (loose["margin"] > 1e-3).all()      # (nothing sits on a threshold)
    e0, k0, _, _ = _keys(v, f, -0.99)
    e1, k1, _, s1 = _keys(v, f, 0.2)
    assert np.array_equal(k0 != MAX, loose["candidate"]) and np.array_equal(k1 != MAX, tight["candidate"])
    assert (k0[only] != MAX).all() and (k1[only] == MAX).all() and not s1[only].any()


@pytest.mark.parametrize("name", mq.SHAPES)
def test_whole_run(name):
    from selfreconcode_amd.mesh_prep import simplify_to
    r = _run(name)
    v, f, mesh, rep = r["v"], r["f"], r["mesh"], r["rep"]
    F0, target = len(f), TARGETS[name]
    nv, nf, vm = mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.vertex_map.cpu().numpy()
    print(f"{name}: {F0} -> {len(nf)} faces in {rep['rounds']} rounds; report {rep}")
    assert mesh.cell == 0. and not rep["stalled"] and rep["rounds"] <= 64 and rep["method"] == "collapse"
    assert len(nf) == F0 - 2 * ((F0 - target + 1) // 2) == rep["faces"] and rep["collapses"] == (F0 - len(nf)) // 2 and rep["vertices"] == len(nv)
    assert rep["locked_vertices"] == 0 and rep["candidates_first"] > 0 and rep["candidates_last"] > 0 and rep["zero_area"] == 0
    t = mc.topology(nv, nf)
    assert t["euler"] == 2 and t["open_edges"] == 0 and t["oriented"] and nf.min() == 0 and nf.max() == len(nv) - 1
    # vertex_map: onto the survivors, and a survivor -- the least original index of its class, since a collapse keeps the lower end -- to
    # itself: the survivors keep their ascending original order
    assert vm.shape == (len(v),) and vm.min() == 0 and vm.max() == len(nv) - 1
    first = np.full(len(nv), len(v))
    np.minimum.at(first, vm, np.arange(len(v)))
    assert (np.diff(first) > 0).all() and np.array_equal(vm[first], np.arange(len(nv)))
    untouched = np.bincount(vm, minlength=len(nv))[vm] == 1
    assert np.array_equal(nv[vm[untouched]].view(np.int32), v[untouched].view(np.int32))
    mean = simplify_to(_t(v), _t(f), target, placement="mean")
    ours, theirs = mq.quality(name, nv, nf)["surface"], mq.quality(name, mean.verts.cpu().numpy(), mean.faces.cpu().numpy())["surface"]
    print(f"{name}: surface error {ours:.4g} against the clustering's {theirs:.4g} ({mean.faces.shape[0]} faces): ratio {ours / theirs:.3g}")
    assert ours <= 0.5 * theirs
    again = r["again"]
    assert torch.equal(again.verts.view(torch.int32), mesh.verts.view(torch.int32)) and torch.equal(again.faces, mesh.faces) and torch.equal(again.vertex_map, mesh.vertex_map)


def test_flat_grid_beyond_one_launch_pass():
    """800 x 800 vertices, 1 276 802 faces (the launch grid covers 524 288 threads): to half the faces.  Every quadric is that of the
    plane z = 0, so every cost is exactly 0, every position stays in the plane, and the order is the hash's alone."""
    from selfreconcode_amd import mesh_prep_ops as mp
    from selfreconcode_amd.mesh_prep import simplify_collapse
    n = 800
    v, f = mq.flat_grid(n)
    tv, tf = _t(v), _t(f)
    edges, keys, pos, sel = mp.collapse_round(tv, tf, mp.vertex_quadrics(tv, tf))
    cand = keys != MAX
    interior = ((edges % n > 0) & (edges % n < n - 1) & (edges // n > 0) & (edges // n < n - 1)).all(1)
    assert edges.shape[0] == 3 * (n - 1) ** 2 + 2 * (n - 1) and torch.equal(cand, interior)
    assert ((keys[cand] >> 32) == 0).all() and (pos[:, 2] == 0).all() and int(sel.sum()) > 1000 and not (sel & ~cand).any()
    rep = {}
    F0 = len(f)
    mesh = simplify_collapse(tv, tf, F0 // 2, report=rep)
    print(f"flat grid {n}: {F0} -> {mesh.faces.shape[0]} faces in {rep['rounds']} rounds; {rep}")
    assert mesh.faces.shape[0] == F0 - 2 * ((F0 - F0 // 2 + 1) // 2) and not rep["stalled"] and rep["locked_vertices"] == 4 * (n - 1)
    assert rep["zero_area"] == 0 and (mesh.verts[:, 2] == 0).all()
    ij = torch.arange(n, device=DEV)
    ring = torch.cat([ij, ij + n * (n - 1), ij * n, ij * n + n - 1]).unique()
    assert torch.equal(mesh.verts[mesh.vertex_map[ring]], tv[ring]) and mesh.vertex_map[ring].unique().shape[0] == ring.shape[0]
    p = mesh.verts.double()[mesh.faces]
    area2 = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2]
    assert (area2 > 0).all() and abs(float(area2.sum()) - 2. * (n - 1) ** 2) <= 1e-9 * 2. * (n - 1) ** 2          # still a tiling of the square


def test_stall_budget_and_refusals():
    from selfreconcode_amd.mesh_prep import simplify_collapse, simplify_to
    v, f = mq.shape("cube_jitter")
    tv, tf = _t(v), _t(f)
    rep = {}
    one = simplify_collapse(tv, tf, 300, max_rounds=1, report=rep)
    assert rep["stalled"] and rep["rounds"] == 1 and 0 < rep["collapses"] and one.faces.shape[0] == len(f) - 2 * rep["collapses"] > 300
    t = mc.topology(one.verts.cpu().numpy(), one.faces.cpu().numpy())
    assert t["euler"] == 2 and t["open_edges"] == 0 and t["oriented"]
    rep = {}
    padded = torch.cat([tf, torch.full((3, 3), -1, dtype=torch.int64, device=DEV), tf[:1, [0, 0, 1]]])
    same, ref = simplify_collapse(tv, padded, len(f) + 10, report=rep), simplify_to(tv, tf, len(f) + 10)
    assert same.cell == 0. and torch.equal(same.verts, ref.verts) and torch.equal(same.faces, ref.faces) and torch.equal(same.vertex_map, ref.vertex_map)
    assert rep == dict(method="collapse", rounds=0, collapses=0, stalled=False, locked_vertices=0, candidates_first=0, candidates_last=0, vertices=len(v),
                       faces=len(f), flipped=0, zero_area=0)
    odd = simplify_collapse(tv, tf, 301)                                                # an odd distance to the budget: one pair more
    assert odd.faces.shape[0] == 300
    bad = tv.clone(); bad[5, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        simplify_collapse(bad, tf, 300)
    with pytest.raises(RuntimeError, match="non-GPU"):
        simplify_collapse(tv.cpu(), tf.cpu(), 300)
    with pytest.raises(ValueError, match="outside"):
        simplify_collapse(tv[:100], tf, 300)
    for kw in (dict(reg=0.), dict(reg=float("nan")), dict(flip_cos=1.), dict(flip_cos=-1.5)):
        with pytest.raises(ValueError):
            simplify_collapse(tv, tf, 300, **kw)


def test_collapse_abi_argument_checks():
    """The ten entry points accept the arrays of one round on a tetrahedron, and refuse each of them as a null pointer, each count as 0
    or negative, and each parameter outside its domain, with SR_EINVAL before anything is launched."""
    from selfreconcode_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    P = _lib.ptr
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    v = _t(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])); f = _t(np.int64([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]))
    V, F, E = 4, 4, 6
    slots = torch.sort(f.view(-1), stable=True)[1].contiguous(); soff = torch.arange(0, 3 * F + 1, 3, device=DEV)
    Q = torch.zeros(V, 10, dtype=torch.float64, device=DEV); hkey = torch.zeros(3 * F, dtype=i64, device=DEV)
    ukey = _t(np.int64([1, 2, 3, 6, 7, 11])); offs = torch.arange(0, 2 * E + 1, 2, device=DEV)
    edges = torch.zeros(E, 2, dtype=i64, device=DEV); opp = torch.zeros(E, 2, dtype=i64, device=DEV); count = torch.zeros(E, dtype=i32, device=DEV)
    locked = torch.ones(V, dtype=i32, device=DEV); directed = torch.zeros(2 * E, dtype=i64, device=DEV)
    pos = torch.zeros(E, 3, device=DEV); key = torch.zeros(E, dtype=i64, device=DEV); m1 = torch.zeros(V, dtype=i64, device=DEV); m2 = torch.zeros(V, dtype=i64, device=DEV)
    sel = torch.ones(E, dtype=u8, device=DEV); record = torch.ones(2, dtype=i64, device=DEV)
    none = torch.zeros(E, dtype=u8, device=DEV); v2 = v.clone(); Q2 = Q.clone(); target = torch.arange(V, device=DEV)
    out = torch.zeros(F, 3, dtype=i64, device=DEV); keep = torch.zeros(F, dtype=u8, device=DEV)
    nxt = torch.zeros(V, dtype=i64, device=DEV); changed = torch.ones(1, dtype=i32, device=DEV)
    _lib.call("sr_collapse_edge_keys", P(f), F, V, P(hkey), s)
    skey, perm = torch.sort(hkey, stable=True)
    assert torch.equal(torch.unique_consecutive(skey), ukey)
    _lib.call("sr_collapse_edge_heads", P(ukey), P(offs), E, P(perm), P(f), F, V, P(edges), P(count), P(opp), P(locked), P(directed), s)
    nbr = torch.sort(directed)[0]; noff = torch.arange(0, 2 * E + 1, 3, device=DEV)
    calls = {
        "sr_collapse_vertex_quadrics": dict(v=P(v), V=V, f=P(f), F=F, slots=P(slots), soff=P(soff), Q=P(Q)),
        "sr_collapse_edge_keys": dict(f=P(f), F=F, V=V, key=P(hkey)),
        "sr_collapse_edge_heads": dict(ukey=P(ukey), offs=P(offs), E=E, perm=P(perm), f=P(f), F=F, V=V, edges=P(edges), count=P(count), opp=P(opp), locked=P(locked),
                                       directed=P(directed)),
        "sr_collapse_candidates": dict(v=P(v), V=V, f=P(f), F=F, Q=P(Q), slots=P(slots), soff=P(soff), nbr=P(nbr), noff=P(noff), edges=P(edges), count=P(count),
                                       opp=P(opp), locked=P(locked), E=E, reg=1e-3, flip_cos=0.2, pos=P(pos), key=P(key)),
        "sr_collapse_min1": dict(edges=P(edges), key=P(key), E=E, V=V, m1=P(m1)),
        "sr_collapse_min2": dict(edges=P(edges), E=E, V=V, m1=P(m1), m2=P(m2)),
        "sr_collapse_select": dict(edges=P(edges), key=P(key), E=E, V=V, m2=P(m2), sel=P(sel), record=P(record)),
        "sr_collapse_apply_vertices": dict(edges=P(edges), pos=P(pos), sel=P(none), E=E, v=P(v2), V=V, Q=P(Q2), target=P(target)),
        "sr_collapse_apply_faces": dict(f=P(f), F=F, target=P(target), V=V, out=P(out), keep=P(keep)),
        "sr_collapse_map_jump": dict(parent=P(target), V=V, next=P(nxt), changed=P(changed)),
    }
    big = dict(V=(1 << 31) + 1), dict(F=(1 << 30) + 1)
    extra = {"sr_collapse_vertex_quadrics": [dict(V=-1), dict(F=-1), *big], "sr_collapse_edge_keys": [dict(F=-1), dict(V=-1), *big],
             "sr_collapse_edge_heads": [dict(E=-1), dict(F=-1), dict(V=-1), dict(E=3 * F + 1), *big],
             "sr_collapse_candidates": [dict(V=-1), dict(F=-1), dict(E=-1), dict(E=3 * F + 1), dict(reg=-1e-3), dict(reg=float("nan")), dict(reg=float("inf")),
                                        dict(flip_cos=1.), dict(flip_cos=-1.5), dict(flip_cos=float("nan")), *big],
             "sr_collapse_min1": [dict(E=-1), dict(V=-1)], "sr_collapse_min2": [dict(E=-1), dict(V=-1), dict(m2=P(m1))],
             "sr_collapse_select": [dict(E=-1), dict(V=-1)], "sr_collapse_apply_vertices": [dict(E=-1), dict(V=-1)],
             "sr_collapse_apply_faces": [dict(F=-1), dict(V=-1)], "sr_collapse_map_jump": [dict(V=-1), dict(next=P(target))]}
    n = 0
    for name, args in calls.items():
        _lib.call(name, *args.values(), s)                                                           # the arguments as they are: accepted
        torch.cuda.synchronize()
        for change in [{k: 0} for k in args if k != "flip_cos"] + extra[name]:                       # (flip_cos = 0 is a valid threshold)
            with pytest.raises(_lib.SrError, match="SR_EINVAL"):
                _lib.call(name, *{**args, **change}.values(), s)
                pytest.fail(f"{name} accepted {change}")
            n += 1
    torch.cuda.synchronize()
    assert n == (7 + 4) + (4 + 4) + (12 + 6) + (17 + 12) + (5 + 2) + (5 + 3) + (7 + 2) + (8 + 2) + (6 + 2) + (4 + 2)
    # what the accepted calls left: a tetrahedron has six edges of two faces each, nothing locked, no candidate (valence), nothing selected
    assert edges.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and count.tolist() == [2] * 6 and locked.tolist() == [0] * 4
    assert sorted(opp[0].tolist()) == [2, 3] and (key == MAX).all() and (m1 == MAX).all() and (m2 == MAX).all() and sel.tolist() == [0] * 6
    assert record.tolist() == [0, 0] and torch.equal(v2, v) and torch.equal(out, f) and keep.tolist() == [1] * 4 and int(changed) == 0
    assert torch.equal(nxt, target) and np.abs(Q.cpu().numpy() - mc.vertex_quadrics(v.cpu().numpy(), f.cpu().numpy())).max() <= 1e-14


def test_prepare_template_collapse_into_export_texture(tmp_path):
    import _texture_ref as tr
    from selfreconcode_amd.mesh_io import read_obj_uv
    from selfreconcode_amd.mesh_prep import prepare_template, simplify_quality
    from selfreconcode_amd.posed import FULL_RATIO
    from selfreconcode_amd.synthetic import build_synthetic_scene
    from selfreconcode_amd.texture import export_texture, texture_frames
    H = W = 96
    R = 256
    torch.manual_seed(0)
    net, ds, _ = build_synthetic_scene(device=DEV, frame_num=40, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)], lbs_volume_shape=(17, 57, 33),
                                       consistent_masks=False)
    fids = texture_frames(ds.frame_num, 6)
    views = [(int(f), tr.smooth_image(H, W, 0.3 * k), ds.batch(torch.tensor([int(f)], device=DEV))['mask'][0] > 0.5) for k, f in enumerate(fids)]
    TmpVs, Tmpfs = net.discretizeSDF(FULL_RATIO, None, 0.)
    root, rep = str(tmp_path / "collapse"), {}
    prep = prepare_template(net, root, target_faces=600, resolution=R, TmpVs=TmpVs, Tmpfs=Tmpfs, method="collapse", report=rep)
    before = mc.topology(TmpVs.detach().cpu().numpy(), mc.clean(Tmpfs.cpu().numpy()))
    after = mc.topology(prep.mesh.verts.cpu().numpy(), prep.mesh.faces.cpu().numpy())
    print(f"template {before} -> {after}; report {rep}")
    assert rep["method"] == "collapse" and rep["faces"] == prep.mesh.faces.shape[0] and rep["zero_area"] == 0
    assert rep["stalled"] or prep.mesh.faces.shape[0] in (600, 599)
    referenced = len(np.unique(mc.clean(Tmpfs.cpu().numpy())))                             # (a collapse removes one vertex, three edges, two faces)
    assert after["open_edges"] <= before["open_edges"] and after["oriented"] == before["oriented"]
    assert after["euler"] == before["euler"] - before["V"] + referenced
    v, f, vt, ft = read_obj_uv(prep.obj_path)
    assert np.array_equal(v, prep.mesh.verts.cpu().numpy()) and np.array_equal(f, prep.mesh.faces.cpu().numpy())
    q = simplify_quality(prep.mesh, TmpVs.detach(), Tmpfs, samples=20000)
    mean = prepare_template(net, str(tmp_path / "mean"), target_faces=600, resolution=R, TmpVs=TmpVs, Tmpfs=Tmpfs)
    m = simplify_quality(mean.mesh, TmpVs.detach(), Tmpfs, samples=20000)
    print(f"volume ratio collapse {q['volume_ratio']:.5f}, clustering {m['volume_ratio']:.5f}; source -> simplified mean {q['source_to_simplified']['mean']:.4g}, "
          f"{m['source_to_simplified']['mean']:.4g}; charts {prep.atlas.labels.shape[0]} / {mean.atlas.labels.shape[0]}, overlap {prep.atlas.overlap_texels} / {mean.atlas.overlap_texels}")
    assert np.isfinite(q["volume_ratio"]) and abs(1. - q["volume_ratio"]) < abs(1. - m["volume_ratio"])
    baked = export_texture(net, prep.obj_path, views, os.path.join(root, "template"), resolution=R, check_num=2)
    assert baked.tex_mask.any() and baked.mask_final.any() and not (baked.mask_final & ~baked.tex_mask).any()
    for kw, what in ((dict(method="greedy"), "method"), (dict(method="collapse", placement="quadric"), "placement")):
        with pytest.raises(ValueError, match=what):
            prepare_template(net, str(tmp_path / "bad"), TmpVs=TmpVs, Tmpfs=Tmpfs, **kw)
    assert not os.path.exists(str(tmp_path / "bad"))


def _texture_command(tmp_path_factory, suffix, extra):
    """The texture command on a copy of the folder a training run left (tests/_train_scene.py; the session's shared result folder is only
    read) -> (the template folder, what it said with the folder's path taken out)."""
    import _train_scene as ts
    from selfreconcode_amd import texture
    from test_texture_cli_gpu import ARGS
    capture, first = ts.folder(tmp_path_factory)
    rec_root = os.path.join(os.path.dirname(first.save_root), os.path.basename(first.save_root) + suffix)
    assert not os.path.exists(rec_root)
    shutil.copytree(first.save_root, rec_root, ignore=shutil.ignore_patterns('template', 'textured', 'turntable'))
    said = []
    assert texture.main(ARGS + ['--rec-root', rec_root] + extra, out=lambda *a, **k: said.append(' '.join(str(x) for x in a)), resolutions=ts.PYRAMID) == 0
    return os.path.join(rec_root, 'template'), [x.replace(rec_root, '<root>') for x in said]


def test_texture_command_with_collapse_and_report(tmp_path_factory):
    """`python -m selfreconcode_amd.texture --simplify collapse --simplify-report`: the usual files plus template/simplify.json with the
    collapse report; together with --placement quadric it is a usage error, before anything is loaded."""
    from selfreconcode_amd import texture
    from test_texture_cli_gpu import ARGS, WRITTEN
    with pytest.raises(SystemExit):
        texture.main(ARGS + ['--rec-root', 'nowhere', '--simplify', 'collapse', '--placement', 'quadric'])
    folder, said = _texture_command(tmp_path_factory, '_collapse', ['--simplify', 'collapse', '--simplify-report'])
    assert sorted(os.listdir(folder)) == sorted(WRITTEN + ['simplify.json'])
    lines = [x for x in said if x.startswith('simplify:')]
    assert len(lines) == 1 and 'method collapse' in lines[0] and 'simplify.json' in lines[0]
    with open(os.path.join(folder, 'simplify.json')) as fh:
        rep = json.load(fh)
    assert set(rep) == {'method', 'rounds', 'collapses', 'stalled', 'locked_vertices', 'candidates_first', 'candidates_last', 'vertices', 'faces', 'flipped',
                        'zero_area', 'quality'}
    assert rep['method'] == 'collapse' and rep['rounds'] > 0 and rep['collapses'] > 0 and rep['zero_area'] == 0 and (rep['faces'] <= 400 or rep['stalled'])
    assert np.isfinite(rep['quality']['volume_ratio']) and np.isfinite(rep['quality']['source_to_simplified']['mean'])
    assert sum(x.startswith('template:') for x in said) == 1 and sum('wrote' in x and 'uvmap.obj' in x for x in said) == 1


def test_texture_command_default_is_the_clustering_as_before(tmp_path_factory):
    """The command as it always was and the command with the defaults spelled out write the same bytes and say the same."""
    from test_texture_cli_gpu import WRITTEN, _snapshot
    plain, said_plain = _texture_command(tmp_path_factory, '_plain', [])
    spelled, said_spelled = _texture_command(tmp_path_factory, '_spelled', ['--simplify', 'cluster', '--placement', 'mean'])
    assert sorted(os.listdir(plain)) == WRITTEN and _snapshot(plain) == _snapshot(spelled) and said_plain == said_spelled
    assert not any(x.startswith('simplify:') for x in said_plain)
