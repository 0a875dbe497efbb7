"""The ICP alignment on the GPU (csrc/icp.hip, align.py, evaluate): sr_icp_accumulate launch by launch against double
sums built from closest_point of the same points, sr_icp_solve alone against the restatement's solve, then icp_align, surface_metrics
and the command against the float64 restatement of tests/_icp_ref.py and the known transform.

Bounds.  Sums: S 2^-53 sum |term|, the bound of a sum of S rounded terms in any order -- the terms themselves are formed in the stated
operation order, without contraction, on both sides, so a sum of one term is exact.  Solve: max(4 E, 2^-40), E the difference between
the restatement's Cholesky and numpy.linalg.lstsq on the same scaled system (the float64 noise of that system).  End to end: max(4 E32,
8 2^-23 scale), E32 the restatement with a float32 closest-point search against the float64 one, scale the largest coordinate (DESIGN
3.18's bound).  Every comparison prints measured / bound."""
import json
import os

import numpy as np
import pytest
import torch

import _icp_ref as ir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2. ** -23
U = 2. ** -53
_CACHE = {}


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _case(name, n=16):
    if ("case", name, n) not in _CACHE:
        _CACHE[("case", name, n)] = ir.case(name, n)
    return _CACHE[("case", name, n)]


def _index():
    """The MeshIndex of the n = 16 shape (3072 faces) and its frame."""
    from selfreconcode_amd import align, surfdist_ops as sd
    if "index" not in _CACHE:
        _, gt, _ = _case("rigid")
        index = sd.MeshIndex.build(_t(gt[0]), _t(gt[1]))
        assert index.faces.shape[0] == 3072
        _CACHE["index"] = (index, align.frame_of(index))
    return _CACHE["index"]


def _reference(name):
    """The restatement's float64 result, E32 and the bound of a named case: computed once."""
    if ("ref", name) not in _CACHE:
        pred, gt, answer = _case(name)
        r64 = ir.icp(pred, gt, 2003, iters=12, scale=name == "similarity")
        r32 = ir.icp(pred, gt, 2003, iters=12, scale=name == "similarity", dtype=np.float32)
        e32 = float(np.abs(r64["matrix"] - r32["matrix"]).max())
        scale = max(float(np.abs(pred[0]).max()), float(np.abs(gt[0]).max()))
        _CACHE[("ref", name)] = (r64, e32, scale, max(4. * e32, 8. * EPS * scale))
    return _CACHE[("ref", name)]


def _state(matrix, done=0.):
    from selfreconcode_amd import align
    s = np.zeros(align.STATE)
    s[:9], s[9:12], s[align.DONE] = matrix[:3, :3].reshape(9), matrix[:3, 3], done
    return _t(s)


def _transform(state, p):
    """q = fl32(((M0 px + M1 py) + M2 pz) + t) per row in double, op by op."""
    p = p.double()
    return torch.stack([((state[3 * i] * p[:, 0] + state[3 * i + 1] * p[:, 1]) + state[3 * i + 2] * p[:, 2]) + state[9 + i] for i in range(3)], 1).float()


def _sums(q, index, frame, max_dist):
    """(sums [38], sums of |term| [38], dist [S]) in double from closest_point(q): the terms in the stated operation order."""
    from selfreconcode_amd import surfdist_ops as sd
    (ox, oy, oz), rho = frame
    dist, face, closest = sd.closest_point(q, index)
    kept = torch.isfinite(q).all(1) & (dist <= max_dist)
    qk, ck, dk = q[kept].double(), closest[kept].double(), dist[kept].double()
    tri = index.tri[face[kept]].double()
    u, v = tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3]
    n = [u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]]
    length = torch.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    n = [torch.where(length > 0, c / length, torch.zeros_like(c)) for c in n]
    x = [(qk[:, 0] - ox) / rho, (qk[:, 1] - oy) / rho, (qk[:, 2] - oz) / rho]
    e = [qk[:, i] - ck[:, i] for i in range(3)]
    w = [x[1] * n[2] - x[2] * n[1], x[2] * n[0] - x[0] * n[2], x[0] * n[1] - x[1] * n[0], n[0], n[1], n[2], (n[0] * x[0] + n[1] * x[1]) + n[2] * x[2],
         ((n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]) / rho]
    terms = [w[j] * w[l] for j in range(8) for l in range(j, 8)] + [torch.ones_like(dk), dk * dk]
    return torch.stack([t.sum() for t in terms]).cpu().numpy(), torch.stack([t.abs().sum() for t in terms]).cpu().numpy(), dist


def _start(name="rigid"):
    """A state a little off the answer of the case, so that every distance is positive and every unknown has a gradient."""
    _, _, answer = _case(name)
    m = ir.truth_matrix(answer)
    m[:3, :3] = ir.exp_rotation([0.02, -0.015, 0.01]) @ m[:3, :3]
    m[:3, 3] += [0.004, 0.003, -0.005]
    return m


def _samples(S):
    from selfreconcode_amd import surfdist_ops as sd
    pred, _, _ = _case("rigid")
    return sd.sample_surface(_t(pred[0]), _t(pred[1]), S, 5)[0]


# ------------------------------------------------------------------------------------------------------------ sr_icp_accumulate
@pytest.mark.parametrize("S", [1, 1031, 1024 * 256 + 257])
def test_accumulate_one_launch(S):
    """One lane; partial waves in five blocks; one full grid of the capped block count plus 257 samples in the stride loop."""
    from selfreconcode_amd import align
    index, frame = _index()
    p, state = _samples(S), _state(_start())
    assert align.blocks_of(S) == (1 if S == 1 else 5 if S == 1031 else align.MAX_BLOCKS)
    partial = torch.full((align.blocks_of(S), align.COLS), 7., dtype=torch.float64, device=DEV)
    align.accumulate(p, index, state, frame, float("inf"), partial)
    again = torch.full_like(partial, -3.)
    align.accumulate(p, index, state, frame, float("inf"), again)
    assert torch.equal(partial.view(torch.int64), again.view(torch.int64))               # two runs, identical bits
    assert bool((partial[:, 38:] == 0).all())
    got = partial.sum(0).cpu().numpy()
    want, mass, dist = _sums(_transform(state, p), index, frame, float("inf"))
    bound = S * U * mass
    ratio = float(np.max(np.abs(got[:38] - want) / np.where(bound > 0, bound, 1.)))
    print(f"accumulate S {S}: kept {got[36]:.0f} of {S}, largest |sum - reference| / (S 2^-53 sum|term|) = {ratio:.3g} (bound 1), "
          f"rms d {np.sqrt(got[37] / S):.3g}")
    assert got[36] == want[36] == S
    assert (np.abs(got[:38] - want) <= bound).all()
    if S == 1:
        assert np.array_equal(got[:38], want)                                             # one term: the same bits
    if S == 1031:
        # max_dist equal to one of the distances: <=, so that sample stays
        md = float(dist.sort()[0][S // 2])
        align.accumulate(p, index, state, frame, md, partial)
        got = partial.sum(0).cpu().numpy()
        want, mass, _ = _sums(_transform(state, p), index, frame, md)
        assert got[36] == float((dist <= md).sum()) == want[36] and 0 < got[36] < S and (np.abs(got[:38] - want) <= S * U * mass).all()
        print(f"accumulate S {S}: max_dist {md:.6g} keeps {got[36]:.0f}")
        # samples that map to NaN or Inf are not kept, and the sums stay finite
        bad = p.clone()
        bad[[0, 63, 64, 500, 1030]] = torch.tensor([[float("nan"), 0., 0.], [0., float("inf"), 0.], [0., 0., -float("inf")], [3.3e38, 3.3e38, 3.3e38],
                                                      [float("nan")] * 3], device=DEV)
        align.accumulate(bad, index, state, frame, float("inf"), partial)
        got = partial.sum(0).cpu().numpy()
        q = _transform(state, bad)
        assert int((~torch.isfinite(q).all(1)).sum()) == 5
        want, mass, _ = _sums(q, index, frame, float("inf"))
        assert np.isfinite(got).all() and got[36] == S - 5 == want[36] and (np.abs(got[:38] - want) <= S * U * mass).all()


def test_done_flag_freezes_both_launches():
    from selfreconcode_amd import align
    index, frame = _index()
    p, state = _samples(1031), _state(_start(), done=1.)
    before = state.clone()
    partial = torch.full((align.blocks_of(1031), align.COLS), 7., dtype=torch.float64, device=DEV)
    history = torch.full((3, align.HISTORY), 5., dtype=torch.float64, device=DEV)
    align.accumulate(p, index, state, frame, float("inf"), partial)
    assert bool((partial == 7.).all())                                                   # nothing written
    align.solve(partial, frame, True, EPS, 0, 3, state, history)
    align.solve(partial, frame, True, EPS, 1, 3, state, history)
    assert torch.equal(state.view(torch.int64), before.view(torch.int64))
    assert history[0].tolist() == [0., 0., 0., 0., 0., 1.] and history[1].tolist() == history[0].tolist() and history[2].tolist() == [5.] * 6
    align.accumulate(p, index, state, frame, float("inf"), partial, measure=True)        # the measuring launch ignores the flag
    assert float(partial[:, 36].sum()) == 1031.


# ------------------------------------------------------------------------------------------------------------ sr_icp_solve
def _partial_of(G, count, d2, blocks=3):
    """partial [blocks, 40] whose ascending column sums are exactly the upper triangle of G, count and d2: a float32 head, the rest,
    zeros."""
    cols = np.float64([G[j, l] for j in range(8) for l in range(j, 8)] + [count, d2, 0., 0.])
    head = cols.astype(np.float32).astype(np.float64)
    rows = np.zeros((blocks, 40))
    rows[0], rows[1] = head, cols - head
    assert np.array_equal((rows[0] + rows[1]) + rows[2], cols)
    return _t(rows)


def _host_system(name, n, S):
    pred, gt, _ = _case(name, n) if isinstance(name, str) else (name[0], name[1], None)
    q = ir.samples_of(pred, S, 0)
    d, f, c = ir.sr.closest(q, gt[0], gt[1])
    o, rho = ir.frame(gt[0])
    W = ir.rows(q.astype(np.float64), c, ir.sr.face_normals(gt[0], gt[1])[f], o, rho)
    return W.T @ W, float(S), float((d * d).sum()), ((float(o[0]), float(o[1]), float(o[2])), float(rho))


@pytest.mark.parametrize("scale", [False, True])
def test_solve_against_the_restatement(scale):
    from selfreconcode_amd import align
    G, count, d2, frame = _host_system("similarity", 8, 501)
    o, rho = np.float64(frame[0]), frame[1]
    xi, rank = ir.solve(G, count, scale)
    E = float(np.abs(xi - ir.solve_lstsq(G, count, scale)).max())
    bound = max(4. * E, 2. ** -40)
    start = np.eye(4)
    start[:3, 3] = o                                                                      # M = I, t = o: the state after is the update itself
    state, history = _state(start), torch.zeros((2, align.HISTORY), dtype=torch.float64, device=DEV)
    align.solve(_partial_of(G, count, d2), frame, scale, EPS, 0, 2, state, history)
    s, h = state.cpu().numpy(), history.cpu().numpy()
    M, t = ir.update(np.eye(3), o, xi, o, rho)
    err_m, err_t = float(np.abs(s[:9].reshape(3, 3) - M).max()), float(np.abs((s[9:12] - o) / rho - xi[3:6]).max())
    print(f"solve scale {scale}: |M - restatement| {err_m:.3g}, |tau - restatement| {err_t:.3g}; bound {bound:.3g} (E {E:.3g}), max|xi| {np.abs(xi).max():.3g}")
    assert err_m <= bound and err_t <= bound
    assert h[0, 0] == count and h[0, 3] == rank == (7 if scale else 6) and h[0, 5] == 0. and s[align.DONE] == 0. and s[align.DONE + 1] == 1.
    assert abs(h[0, 1] - np.sqrt(d2 / count)) <= 4 * U * h[0, 1] and abs(h[0, 2] - np.abs(xi).max()) <= bound
    assert abs(h[0, 4] - (1. + xi[6])) <= bound and (scale or abs(h[0, 4] - 1.) <= 8 * 2. ** -52) and (h[1] == 0).all()
    # an update below tol sets the flag: the same system with a huge tol
    state = _state(start)
    align.solve(_partial_of(G, count, d2), frame, scale, 1., 0, 2, state, history)
    assert float(state[align.DONE]) == 1. and float(history[0, 5]) == 1.


def test_solve_flat_target_drops_three_unknowns():
    from selfreconcode_amd import align
    pred, gt = ir.flat_pair(0.05)
    G, count, d2, frame = _host_system((pred, gt), None, 257)
    o, rho = np.float64(frame[0]), frame[1]
    start = np.eye(4)
    start[:3, 3] = o
    for scale in (False, True):
        state, history = _state(start), torch.zeros((1, align.HISTORY), dtype=torch.float64, device=DEV)
        align.solve(_partial_of(G, count, d2), frame, scale, EPS, 0, 1, state, history)
        s, h = state.cpu().numpy(), history.cpu().numpy()
        M = s[:9].reshape(3, 3)
        assert h[0, 3] == 3. and np.isfinite(s).all() and np.isfinite(h).all()
        assert s[9] == o[0] and s[10] == o[1]                                             # tau_x = tau_y = 0 exactly
        assert M[1, 0] == M[0, 1]                                                         # omega_z = 0 exactly: no rotation about the normal
        assert h[0, 4] == 1. if not scale else abs(h[0, 4] - 1.) < 1e-15                  # sigma = 0
        assert abs((s[11] - o[2]) + 0.05) < 1e-7
    empty = _t(np.zeros((2, 40)))                                                         # no pairs: nothing moves, rank 0, done
    state, history = _state(start), torch.zeros((1, align.HISTORY), dtype=torch.float64, device=DEV)
    align.solve(empty, frame, True, EPS, 0, 1, state, history)
    assert np.array_equal(state.cpu().numpy()[:12], _state(start).cpu().numpy()[:12]) and history[0].tolist() == [0., 0., 0., 0., 1., 1.]


def test_composition_stays_a_similarity():
    """30 updates by the same system (tol 0: never done): M M^T = s^2 I to 64 2^-52."""
    from selfreconcode_amd import align
    G, count, d2, frame = _host_system("similarity", 8, 501)
    partial = _partial_of(G, count, d2)
    state, history = _state(np.eye(4)), torch.zeros((30, align.HISTORY), dtype=torch.float64, device=DEV)
    for it in range(30):
        align.solve(partial, frame, True, 0., it, 30, state, history)
    s, h = state.cpu().numpy(), history.cpu().numpy()
    M = s[:9].reshape(3, 3)
    s2 = (M * M).sum() / 3.
    err = float(np.abs(M @ M.T / s2 - np.eye(3)).max())
    print(f"composition: |M M^T / s^2 - I| {err / 2. ** -52:.3g} 2^-52 after 30 updates (bound 64), s {np.sqrt(s2):.6g}, max|xi| {h[0, 2]:.3g}")
    assert err <= 64 * 2. ** -52 and (h[:, 5] == 0).all() and s[align.DONE + 1] == 30. and np.linalg.det(M) > 0 and h[0, 2] > 1e-3
    assert abs(h[29, 4] - np.sqrt(s2)) <= 4 * U * h[29, 4]


def test_entries_refuse_bad_arguments():
    from selfreconcode_amd import _lib, align
    index, frame = _index()
    p, state = _samples(300), _state(np.eye(4))
    partial = torch.zeros((2, align.COLS), dtype=torch.float64, device=DEV)
    history = torch.zeros((2, align.HISTORY), dtype=torch.float64, device=DEV)
    n = index.n

    def acc(points=p, S=300, tri=index.tri, st=state, rho=frame[1], max_dist=1., blocks=2):
        _lib.launch("sr_icp_accumulate", p, points, S, tri, 3072, index.lo, index.cell, n[0], n[1], n[2], index.cell_start, index.cell_faces, index.pairs,
                    st, 0., 0., 0., rho, max_dist, 0, partial, blocks)

    acc()
    for bad in (dict(points=None), dict(S=0), dict(tri=index.tri.view(-1)[1:]), dict(st=None), dict(rho=0.), dict(max_dist=float("nan")), dict(blocks=1)):
        with pytest.raises(_lib.SrError):
            acc(**bad)
    for it, iters in ((0, 0), (2, 2), (-1, 2)):
        with pytest.raises(_lib.SrError):
            _lib.launch("sr_icp_solve", partial, partial, 2, 0., 0., 0., 1., 0, EPS, it, iters, state, history)
    with pytest.raises(_lib.SrError):
        _lib.launch("sr_icp_solve", partial, None, 2, 0., 0., 0., 1., 0, EPS, 0, 2, state, history)


# ------------------------------------------------------------------------------------------------------------ icp_align
@pytest.mark.parametrize("name", ["rigid", "similarity"])
def test_icp_align_end_to_end(name):
    from selfreconcode_amd.align import icp_align
    pred, gt, answer = _case(name)
    r64, e32, scale, bound = _reference(name)
    dp, dg = (_t(pred[0]), _t(pred[1])), (_t(gt[0]), _t(gt[1]))
    got = icp_align(dp, dg, samples=2003, iters=12, scale=name == "similarity")
    err_ref = float(np.abs(got.matrix - r64["matrix"]).max())
    err_truth = float(np.abs(got.matrix - ir.truth_matrix(answer)).max())
    print(f"icp_align {name}: {got.iterations} iterations (restatement {r64['iterations']}), |matrix - restatement| {err_ref:.3g}, |matrix - truth| "
          f"{err_truth:.3g}; bound {bound:.3g} (E32 {e32:.3g}); rms {got.rms_before:.3g} -> {got.rms_after:.3g}, rank {got.rank}")
    assert err_ref <= bound and err_truth <= bound
    assert got.converged and got.iterations <= 12 and got.rank == (7 if name == "similarity" else 6) and got.pairs == 2003
    assert got.matrix.dtype == np.float64 and got.history.shape == (12, 6) and np.array_equal(got.matrix[3], [0., 0., 0., 1.])
    assert abs(got.scale - answer[0]) <= bound and np.abs(got.rotation - answer[1]).max() <= bound and np.abs(got.translation - answer[2]).max() <= bound
    assert (name == "similarity") == (got.scale != 1.) or abs(got.scale - 1.) <= 64 * 2. ** -52
    assert got.rms_after < 1e-3 * got.rms_before and got.rms_before == got.history[0, 1]
    assert (got.history[got.iterations:, 5] == 1).all() and (got.history[:got.iterations - 1, 5] == 0).all()
    # the freeze: more launches change no bit; two calls are identical
    more = icp_align(dp, dg, samples=2003, iters=30, scale=name == "similarity")
    exact = icp_align(dp, dg, samples=2003, iters=got.iterations, scale=name == "similarity")
    assert np.array_equal(more.matrix, got.matrix) and np.array_equal(exact.matrix, got.matrix) and more.iterations == exact.iterations == got.iterations
    assert exact.converged and more.rms_after == got.rms_after
    again = icp_align(dp, dg, samples=2003, iters=12, scale=name == "similarity")
    assert np.array_equal(again.matrix, got.matrix) and np.array_equal(again.history, got.history) and again.rms_after == got.rms_after
    # apply: the double product, rounded once
    want = (pred[0].astype(np.float64) @ got.matrix[:3, :3].T + got.matrix[:3, 3])
    out = got.apply(dp[0])
    assert out.dtype == torch.float32 and float(np.abs(out.cpu().numpy() - want).max()) <= EPS * scale
    # an init matrix near the answer, and no init at all (the offset is small enough for ICP to find its way)
    start = ir.truth_matrix(answer)
    start[:3, 3] += 0.01
    for init in (start, "none"):
        other = icp_align(dp, dg, samples=2003, iters=12, scale=name == "similarity", init=init)
        assert other.converged and np.abs(other.matrix - ir.truth_matrix(answer)).max() <= bound
    with pytest.raises(ValueError):
        icp_align(dp, dg, samples=2003, init="pca")
    with pytest.raises(ValueError):
        icp_align(dp, dg, samples=0)


# ------------------------------------------------------------------------------------------------------------ metrics, command
def test_surface_metrics_with_alignment():
    from selfreconcode_amd.evaluate import surface_metrics, vertex_to_surface
    pred, gt, answer = _case("similarity")
    _, _, scale, bound = _reference("similarity")
    dp, dg = (_t(pred[0]), _t(pred[1])), (_t(gt[0]), _t(gt[1]))
    there = (pred[0].astype(np.float64) @ (answer[0] * answer[1]).T + answer[2]).astype(np.float32)      # pred in gt's coordinates
    want = surface_metrics((_t(there), dp[1]), dg, samples=20011, seed=3)
    opts = {"samples": 2003, "iters": 12}
    got = surface_metrics(dp, dg, samples=20011, seed=3, align="similarity", align_opts=opts)
    plain = surface_metrics(dp, dg, samples=20011, seed=3)
    assert "alignment" not in plain and "alignment" not in want and plain == surface_metrics(dp, dg, samples=20011, seed=3)
    assert plain["chamfer"] > 100 * want["chamfer"]                                      # unaligned, the number measures the offset
    a = got["alignment"]
    assert set(a) == {"matrix", "scale", "iterations", "converged", "rank", "rms_before", "rms_after"} and a["converged"] and a["rank"] == 7
    assert np.abs(np.float64(a["matrix"]) - ir.truth_matrix(answer)).max() <= bound
    for label, x, y in [("chamfer", got["chamfer"], want["chamfer"]), ("p2s", got["p2s"], want["p2s"]),
                        ("pred_to_gt mean", got["pred_to_gt"]["mean"], want["pred_to_gt"]["mean"]),
                        ("gt_to_pred mean", got["gt_to_pred"]["mean"], want["gt_to_pred"]["mean"])]:
        print(f"surface_metrics aligned {label}: {x:.9g} vs {y:.9g} in gt's coordinates (bound {bound:.3g})")
        assert abs(x - y) <= bound
    json.dumps(got)
    rigid = surface_metrics(dp, dg, samples=20011, seed=3, align="rigid", align_opts=opts)   # the scale stays: better than nothing, not right
    assert rigid["alignment"]["scale"] == 1. or abs(rigid["alignment"]["scale"] - 1.) <= 64 * 2. ** -52
    assert want["chamfer"] < rigid["chamfer"] < plain["chamfer"]
    with pytest.raises(ValueError):
        surface_metrics(dp, dg, samples=100, align="affine")
    d = vertex_to_surface(dp[0], dg, align="similarity", align_opts=opts, faces=dp[1]).cpu().numpy()
    assert d.shape == (len(pred[0]),) and float(d.max()) <= bound                          # the vertices land on their own surface
    with pytest.raises(ValueError):
        vertex_to_surface(dp[0], dg, align="similarity")


def _write_folder(tmp_path):
    from selfreconcode_amd.mesh_io import write_ply
    pred, gt, answer = _case("rigid", 8)
    rec, gtd = tmp_path / "result", tmp_path / "gt"
    os.makedirs(rec / "meshs")
    os.makedirs(gtd)
    write_ply(str(rec / "tmp.ply"), pred[0], pred[1])
    for fid, grow in ((0, 1.), (7, 1.), (12, 1.01)):
        np.save(str(rec / "meshs" / ("%d.npy" % fid)), (pred[0] * np.float32(grow)).astype(np.float32))
    for fid in (0, 12):
        write_ply(str(gtd / ("%d.ply" % fid)), gt[0], gt[1])
    return rec, gtd, answer


def test_command_with_alignment(tmp_path):
    from selfreconcode_amd import evaluate
    from selfreconcode_amd.mesh_io import write_ply
    pred, gt, answer = _case("similarity", 8)
    scale = float(np.abs(gt[0]).max())
    a, b, out = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "m.json")
    write_ply(a, pred[0], pred[1])
    write_ply(b, gt[0], gt[1])
    lines = []
    got = evaluate.main(["--pred", a, "--gt", b, "--samples", "5003", "--align", "similarity", "--align-samples", "2003", "--align-iters", "12",
                         "--out", out], out=lines.append)
    assert len(lines) == 1 and json.loads(lines[0]) == got == json.load(open(out))
    m = np.float64(got["alignment"]["matrix"])
    assert m.shape == (4, 4) and got["alignment"]["converged"] and np.abs(m - ir.truth_matrix(answer)).max() <= 8 * EPS * scale
    assert got["chamfer"] < 8 * EPS * scale
    # folder mode: per frame, shared, and --align none against no flag at all
    rec, gtd, answer = _write_folder(tmp_path)
    base = ["--rec-root", str(rec), "--gt-root", str(gtd), "--samples", "3001"]
    plain = evaluate.main(base, out=lines.append)
    files = [open(rec / "geometry_errors.txt", "rb").read(), open(rec / "geometry_errors.json", "rb").read()]
    lines_none = []
    none = evaluate.main(base + ["--align", "none"], out=lines_none.append)
    assert none == plain and files == [open(rec / "geometry_errors.txt", "rb").read(), open(rec / "geometry_errors.json", "rb").read()]
    assert "alignment" not in plain["frames"]["0"] and lines_none == lines[1:]
    opts = ["--align", "rigid", "--align-samples", "2003", "--align-iters", "12"]
    per = evaluate.main(base + opts, out=lines.append)
    assert list(per["frames"]) == ["0", "12"] and per["skipped"] == ["7"] and json.load(open(rec / "geometry_errors.json")) == per
    m0, m12 = np.float64(per["frames"]["0"]["alignment"]["matrix"]), np.float64(per["frames"]["12"]["alignment"]["matrix"])
    assert np.abs(m0 - ir.truth_matrix(answer)).max() <= 8 * EPS * scale and not np.array_equal(m0, m12)
    assert per["frames"]["0"]["chamfer"] < 8 * EPS * scale < per["frames"]["12"]["chamfer"] < plain["frames"]["12"]["chamfer"]
    txt = open(rec / "geometry_errors.txt").read().splitlines()
    assert len(txt) == 5 and txt[0] == "      chamfer p2s" and txt[1].startswith("   0: ") and txt[3].startswith("chamfer mean: ")
    shared = evaluate.main(base + opts + ["--align-shared"], out=lines.append)
    s0, s12 = np.float64(shared["frames"]["0"]["alignment"]["matrix"]), np.float64(shared["frames"]["12"]["alignment"]["matrix"])
    assert np.array_equal(s0, m0) and np.array_equal(s12, m0)                             # the first compared frame's transform, for all
    assert shared["frames"]["0"]["chamfer"] == per["frames"]["0"]["chamfer"] and shared["frames"]["12"]["chamfer"] != per["frames"]["12"]["chamfer"]
