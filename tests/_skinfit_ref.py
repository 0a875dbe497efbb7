"""The skin fit restated in float64 numpy, for tests/test_gltf_cpu.py and tests/test_skinfit_gpu.py: the normal
matrices H = sum_t D^T D, the cardinality-constrained simplex QP by enumeration of supports -- each support's equality-constrained
minimiser from its KKT system with numpy's LU solve, not by Cholesky as the kernel does --, the KKT residuals that witness optimality
without any enumeration, and a brute force that is organised differently (every support of exactly K candidates, the full simplex QP on
each).  Nothing here imports the package."""
import itertools

import numpy as np

TRI = 36
LAMBDA_FLOOR = 1e-24


def tri(k, l):
    return k * (k + 1) // 2 + l


def residual_rows(q, y, A, trans, cands):
    """D [T,V,C,3]: d_tk = A[t, cands[v,k]] [q; 1] - (y - trans); A [T,24,12]."""
    T, V = q.shape[:2]
    A = np.asarray(A, np.float64).reshape(T, 24, 3, 4)
    q, y, trans = np.asarray(q, np.float64), np.asarray(y, np.float64), np.asarray(trans, np.float64)
    Ac = A[np.arange(T)[:, None, None], np.asarray(cands)[None, :, :]]                     # [T,V,C,3,4]
    Aq = (Ac[..., :3] * q[:, :, None, None, :]).sum(-1) + Ac[..., 3]
    return Aq - (y - trans[:, None, :])[:, :, None, :]


def accumulate_ref(q, y, A, trans, cands):
    """(H [36,V] float64, S2 [V]): the normal matrices, and S2 = sum_t (max_k |A q| + |y - trans|)^2, the scale of the bound on H."""
    T, V = q.shape[:2]
    C = cands.shape[1]
    D = residual_rows(q, y, A, trans, cands)
    G = np.einsum('tvkx,tvlx->klv', D, D)
    H = np.zeros((TRI, V))
    for k in range(C):
        for l in range(k + 1):
            H[tri(k, l)] = G[k, l]
    target = np.asarray(y, np.float64) - np.asarray(trans, np.float64)[:, None, :]
    Aq = D + target[:, :, None, :]
    S2 = ((np.linalg.norm(Aq, axis=-1).max(-1) + np.linalg.norm(target, axis=-1)) ** 2).sum(0)
    return H, S2


def full_matrix(H, C):
    M = np.zeros((H.shape[1], C, C))
    for k in range(C):
        for l in range(k + 1):
            M[:, k, l] = M[:, l, k] = H[tri(k, l)]
    return M


def lambda_of(H, C, reg, floor=LAMBDA_FLOOR):
    return reg * sum(H[tri(k, k)] for k in range(C)) / C + floor


def objective_of(M, xbar, lam, x):
    """x^T M x + lam |x - xbar|^2 per vertex: M [V,C,C], xbar / x [V,C], lam [V]."""
    return np.einsum('vk,vkl,vl->v', x, M, x) + lam * ((x - xbar) ** 2).sum(1)


def solve_ref(H, xbar, K, reg=1e-6, floor=LAMBDA_FLOOR, lam=None):
    """The enumeration: H [36,V], xbar [V,C] -> {'x' [V,C], 'objective', 'second' (the lowest objective of another accepted support, inf
    without one), 'mask', 'lambda'}.  Ties: the smaller support, then the lower mask."""
    V, C = xbar.shape
    M = full_matrix(H, C)
    lam = lambda_of(H, C, reg, floor) if lam is None else np.broadcast_to(np.asarray(lam, np.float64), (V,))
    best = np.full(V, np.inf)
    second = np.full(V, np.inf)
    best_x = np.zeros((V, C))
    best_mask = np.zeros(V, np.int64)
    best_count = np.zeros(V, np.int64)
    for m in range(1, 1 << C):
        S = [k for k in range(C) if (m >> k) & 1]
        n = len(S)
        if n > K:
            continue
        kkt = np.zeros((V, n + 1, n + 1))
        kkt[:, :n, :n] = 2. * (M[:, S][:, :, S] + lam[:, None, None] * np.eye(n))
        kkt[:, :n, n] = kkt[:, n, :n] = 1.
        rhs = np.concatenate([2. * lam[:, None] * xbar[:, S], np.ones((V, 1))], 1)
        with np.errstate(all='ignore'):
            xs = np.linalg.solve(kkt, rhs[..., None])[:, :n, 0]
        x = np.zeros((V, C))
        x[:, S] = xs
        obj = objective_of(M, xbar, lam, x)
        ok = ~(xs < 0.).any(1) & np.isfinite(obj)
        take = ok & ((obj < best) | ((obj == best) & (n < best_count)))
        second = np.where(take, best, np.where(ok, np.minimum(second, obj), second))
        best = np.where(take, obj, best)
        best_x[take] = x[take]
        best_mask[take] = m
        best_count[take] = n
    return {'x': best_x, 'objective': best, 'second': second, 'mask': best_mask, 'lambda': lam}


def kkt_residuals(M, xbar, lam, x, tol=1e-12):
    """For the simplex QP min x^T M x + lam |x - xbar|^2, x >= 0, sum x = 1, per vertex (spread, slack): the spread of the gradient
    over the support (0 at an optimum: one multiplier for the equality) and the smallest gradient off the support minus the
    support's mean (>= 0 at an optimum: the multipliers of x >= 0); a vertex whose support is everything has slack +inf."""
    g = 2. * np.einsum('vkl,vl->vk', M, x) + 2. * lam[:, None] * (x - xbar)
    on = x > tol
    mean = np.where(on, g, 0.).sum(1) / on.sum(1)
    spread = np.where(on, np.abs(g - mean[:, None]), 0.).max(1)
    slack = np.where(on, np.inf, g - mean[:, None]).min(1)
    return spread, slack


def brute_force(H, xbar, K, reg=1e-6, floor=LAMBDA_FLOOR):
    """The optimum with at most K non-zeros, organised the other way round: over every support of exactly K candidates the full
    simplex QP of that face (solve_ref of the K x K sub-problem with K' = K and the full problem's lambda), the lowest kept ->
    (x [V,C], objective [V])."""
    V, C = xbar.shape
    M = full_matrix(H, C)
    lam = lambda_of(H, C, reg, floor)
    best = np.full(V, np.inf)
    best_x = np.zeros((V, C))
    for S in itertools.combinations(range(C), K):
        S = list(S)
        sub = np.zeros((TRI, V))
        for a in range(K):
            for b in range(a + 1):
                sub[tri(a, b)] = M[:, S[a], S[b]]
        face = solve_ref(sub, xbar[:, S], K, lam=lam)
        x = np.zeros((V, C))
        x[:, S] = face['x']
        obj = objective_of(M, xbar, lam, x)
        take = obj < best
        best = np.where(take, obj, best)
        best_x[take] = x[take]
    return best_x, best


def _rotations(aa):
    angle = np.linalg.norm(aa, axis=-1, keepdims=True)
    x, y, z = np.moveaxis(aa / np.where(angle > 0., angle, 1.), -1, 0)
    zero = np.zeros_like(x)
    Kx = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(aa.shape[:-1] + (3, 3))
    return np.eye(3) + np.sin(angle)[..., None] * Kx + (1. - np.cos(angle))[..., None] * (Kx @ Kx)


def random_problem(seed, V, T, C, noise=0.02):
    """A batch as the skin fit sees one, in float32: q [T,V,3], transforms A [T,24,12] (rotations by about a radian with offsets),
    trans [T,3], distinct candidates cands [V,C], y = a blend of the candidates' transforms of q by weights that change a little from
    frame to frame (+ trans), and a prior xbar [V,C] near the blend's mean."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1., 1., (T, V, 3)).astype(np.float32)
    A = np.concatenate([_rotations(rng.normal(0., 0.6, (T, 24, 3))), rng.uniform(-0.3, 0.3, (T, 24, 3, 1))], -1).astype(np.float32)
    trans = rng.uniform(-0.5, 0.5, (T, 3)).astype(np.float32)
    cands = np.stack([rng.permutation(24)[:C] for _ in range(V)]).astype(np.int32)
    base = rng.uniform(0., 1., (V, C)) ** 3
    base /= base.sum(1, keepdims=True)
    w = np.abs(base[None] + noise * rng.normal(size=(T, V, C)) * base[None])
    w /= w.sum(-1, keepdims=True)
    Ac = A.astype(np.float64)[np.arange(T)[:, None, None], cands[None]]
    Aq = (Ac[..., :3] * q.astype(np.float64)[:, :, None, None, :]).sum(-1) + Ac[..., 3]
    y = ((w[..., None] * Aq).sum(2) + trans[:, None, :]).astype(np.float32)
    xbar = np.abs(base * (1. + 0.1 * rng.normal(size=(V, C))))
    return {'q': q, 'y': y, 'A': A.reshape(T, 24, 12), 'trans': trans, 'cands': cands, 'xbar': xbar / xbar.sum(1, keepdims=True)}


def h_bound(T, S2):
    """|dH_ij| <= (T + 64) 2^-52 S2: the accumulated rounding of T double sums of ~30-operation terms of size <= S2's."""
    return (T + 64) * 2. ** -52 * S2


def near_ties(out, delta):
    """The vertices whose best and second-best supports are closer than an error `delta` [V] on H carries through the objective
    (|x^T dH x| <= max |dH_ij| for x on the simplex, once for each of the two) plus the solvers' own 1e-9 of the objective."""
    return out['second'] - out['objective'] <= 2. * delta + 1e-9 * np.abs(out['objective'])


SOLVE_CASES = [(257, 7, 8, 4, 31), (257, 7, 8, 8, 32), (65, 2, 3, 2, 33), (64, 17, 5, 1, 34)]      # (V, T, C, K, seed) of the GPU solve test
NEAR_TIE_CAP = 0.02


def top_k(xbar, K):
    """The K largest xbar per vertex (stable: a tie to the lower candidate), renormalised -> (x [V,C], chosen [V,C] bool)."""
    order = np.argsort(-xbar, axis=1, kind='stable')[:, :K]
    chosen = np.zeros(xbar.shape, bool)
    np.put_along_axis(chosen, order, True, 1)
    x = np.where(chosen, xbar, 0.)
    return x / x.sum(1, keepdims=True), chosen
