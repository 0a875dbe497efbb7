"""Restatement of the silhouette term of smpl_fit.py that shares no code with csrc/silfit.hip:

  edt_brute / edt_two_pass   the exact squared Euclidean distance transform in numpy (all pairs; columns then rows)
  contour / sample_indices / contour_samples   the contour rule and the sampler
  match / energy             the two terms in torch CPU operators, float64 by default (float32 on request: the same formulas in the
                             kernels' precision, which is how the tests measure their bounds on code that is not under test); the
                             gradients come from autograd; the matches are an INPUT of energy, so that a near-tie cannot decide a
                             gradient comparison
  scene / keypoint_fit / silhouette_fit   tests/_smplfit_scene.py's scene with disc masks of radius 6 round the true projected vertices on
                             a 688 x 544 canvas and the four arm keypoints at confidence 0; the keypoint-only fit (float64) and the
                             silhouette rounds restated from it (Adam written out)
"""
import functools

import numpy as np
import torch

import _smplfit_scene as base
import _smplgrad_ref as gtwin

EMPTY = 1 << 30
F64 = torch.float64
H, W = 688, 544                       # non-square, the width no multiple of 64
DISC = 6
ARMS = (6, 7, 10, 11)                 # cocoplus R wrist, R elbow, L elbow, L wrist
SIGMA, MARGIN, SAMPLES = 20., 6., 512
# (iterations, lr, l_theta, l_beta, l_s, l_in, l_cov): the priors and the step of the scene's last keypoint round; l_in, l_cov: the
# package's documented defaults
SIL_STAGES = ((80, 0.004, 0.1, 0.1, 1., 10., 25.),)


# ---------------------------------------------------------------------------------------------- distance transform
def edt_brute(mask):
    """[H,W] int64: squared distance of every pixel to the nearest non-zero pixel of mask [H,W], by all pairs; EMPTY without one."""
    mask = np.asarray(mask) != 0
    ys, xs = np.nonzero(mask)
    h, w = mask.shape
    if ys.size == 0:
        return np.full((h, w), EMPTY, np.int64)
    Y, X = np.mgrid[0:h, 0:w]
    out = np.empty((h, w), np.int64)
    for y0 in range(0, h, 16):
        out[y0:y0 + 16] = ((Y[y0:y0 + 16, :, None] - ys) ** 2 + (X[y0:y0 + 16, :, None] - xs) ** 2).min(-1)
    return out


def edt_two_pass(masks):
    """[F,H,W] int64 of masks [F,H,W]: the distance along the column by two sweeps, then per row the minimum over the columns of
    (x - x')^2 + g^2(x'), taken offset by offset until the offset's square reaches every value."""
    m = np.asarray(masks) != 0
    f, h, w = m.shape
    big = 1 << 15                                        # its square is EMPTY
    g = np.full((f, h, w), big, np.int64)
    d = np.full((f, w), big, np.int64)
    for y in range(h):
        d = np.where(m[:, y], 0, np.minimum(d + 1, big))
        g[:, y] = d
    d = np.full((f, w), big, np.int64)
    for y in range(h - 1, -1, -1):
        d = np.where(m[:, y], 0, np.minimum(d + 1, big))
        g[:, y] = np.minimum(g[:, y], d)
    g2 = g * g
    best = g2.copy()
    for k in range(1, w):
        if k * k >= best.max():
            break
        best[:, :, k:] = np.minimum(best[:, :, k:], g2[:, :, :-k] + k * k)
        best[:, :, :-k] = np.minimum(best[:, :, :-k], g2[:, :, k:] + k * k)
    return best


# ---------------------------------------------------------------------------------------------- contour and sampler
def contour(masks):
    """[F,H,W] bool: mask pixels with a 4-neighbour inside the image that is background."""
    m = np.asarray(masks) != 0
    c = np.zeros_like(m)
    c[:, :, 1:] |= m[:, :, 1:] & ~m[:, :, :-1]
    c[:, :, :-1] |= m[:, :, :-1] & ~m[:, :, 1:]
    c[:, 1:] |= m[:, 1:] & ~m[:, :-1]
    c[:, :-1] |= m[:, :-1] & ~m[:, 1:]
    return c


def sample_indices(n, S):
    """The ranks, in row-major contour order, of the samples of a frame with n contour pixels."""
    if n <= S:
        return list(range(n))
    return [(i * n) // S for i in range(S)]             # (python integers: no overflow)


def contour_samples(masks, S):
    """(samples [F,S,2] int32 = (x, y), zero past min(n, S); counts [F] int32 = n)."""
    c = contour(masks)
    f = c.shape[0]
    samples, counts = np.zeros((f, S, 2), np.int32), np.zeros(f, np.int32)
    for t in range(f):
        ys, xs = np.nonzero(c[t])                        # row-major
        idx = sample_indices(len(ys), S)
        samples[t, :len(idx), 0], samples[t, :len(idx), 1] = xs[idx], ys[idx]
        counts[t] = len(ys)
    return samples, counts


# ---------------------------------------------------------------------------------------------- the energy
def _t(a, dtype):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).to(dtype)


def project(points, camera, dtype=F64):
    """(xy [F,V,2], front [F,V]): front = in front of the camera with a finite pixel position; the others are masked BEFORE the
    division, so that no NaN reaches a gradient (their xy is the principal point, which nothing reads)."""
    pc = points.matmul(_t(camera['R'], dtype)) + _t(camera['T'], dtype)
    ok = torch.isfinite(pc).all(-1) & (pc[..., 2].detach() > 0)
    pc = torch.where(ok.unsqueeze(-1), pc, torch.tensor([0., 0., 1.], dtype=dtype).expand_as(pc))
    x = camera['cx'] - camera['fx'] * pc[..., 0] / pc[..., 2]
    y = camera['cy'] - camera['fy'] * pc[..., 1] / pc[..., 2]
    xy = torch.stack([x, y], -1)
    return xy, ok & torch.isfinite(xy.detach()).all(-1)


def match(points, samples, counts, camera, dtype=F64):
    """(matches [F,S] int64, -1 without a vertex in front or past min(n, S); distance [F,S] to the matched vertex): the nearest
    projected vertex in front of the camera, the first of equal ones."""
    with torch.no_grad():
        xy, front = project(points, camera, dtype)
        c = _t(samples, dtype)
        d2 = ((c[:, :, None, :] - xy[:, None, :, :]) ** 2).sum(-1)
        d2 = torch.where(front[:, None, :], d2, torch.full_like(d2, float('inf'))).numpy()
        arg = d2.argmin(-1)                              # numpy: the first minimum
        dist = np.sqrt(np.take_along_axis(d2, arg[..., None], -1)[..., 0])
        S = c.shape[1]
        used = (np.arange(S)[None] < np.minimum(np.asarray(counts), S)[:, None]) & np.isfinite(dist)
    return np.where(used, arg, -1), np.where(used, dist, np.inf)


def distances_to(points, samples, vertex, camera, dtype=F64):
    """[F,S]: the pixel distance of every sample to the projection of vertex[t,s] (inf where that is -1 or not in front)."""
    with torch.no_grad():
        xy, front = project(points, camera, dtype)
        v = torch.from_numpy(np.maximum(vertex, 0)).long()
        hit = torch.gather(xy, 1, v.unsqueeze(-1).expand(-1, -1, 2))
        ok = torch.gather(front, 1, v) & torch.from_numpy(vertex >= 0)
        d = (hit - _t(samples, dtype)).norm(dim=-1)
    return torch.where(ok, d, torch.full_like(d, float('inf'))).numpy()


def rho(r2, sigma):
    return sigma ** 2 * r2 / (sigma ** 2 + r2)


def cells(xy, h, w):
    x0 = xy[..., 0].detach().floor().clamp(0, w - 2).long()
    y0 = xy[..., 1].detach().floor().clamp(0, h - 2).long()
    return x0, y0


def energy(points, d2, samples, counts, matches, camera, sigma, margin, dtype=F64):
    """(e_in [F], e_cov [F], outside [F]) in `dtype`; differentiable in points [F,V,3]; d2 [F,H,W] integers, matches [F,S] (match)."""
    d2 = np.asarray(d2)
    f, h, w = d2.shape
    V = points.shape[1]
    xy, front = project(points, camera, dtype)
    x, y = xy[..., 0], xy[..., 1]
    inside = front & (x.detach() >= 0) & (x.detach() <= w - 1) & (y.detach() >= 0) & (y.detach() <= h - 1)
    outside = (~inside).sum(1)
    live = inside & torch.from_numpy(d2[:, 0, 0] != EMPTY).view(f, 1)
    xs = torch.where(live, x, torch.zeros_like(x))
    ys = torch.where(live, y, torch.zeros_like(y))
    x0, y0 = cells(torch.stack([xs, ys], -1), h, w)
    fx, fy = xs - x0, ys - y0
    root = torch.from_numpy(d2.astype(np.float64)).to(dtype).sqrt().view(f, h * w)
    tap = lambda dy, dx: torch.gather(root, 1, (y0 + dy) * w + x0 + dx)          # noqa: E731
    top = tap(0, 0) + fx * (tap(0, 1) - tap(0, 0))
    bot = tap(1, 0) + fx * (tap(1, 1) - tap(1, 0))
    d = top + fy * (bot - top)
    e_in = torch.where(live, rho(d * d, sigma), torch.zeros_like(d)).sum(1) / V
    # coverage: the match is an input and is held fixed
    m = torch.from_numpy(np.asarray(matches)).long()
    S = m.shape[1]
    n = np.minimum(np.asarray(counts), S)
    used = (m >= 0) & (torch.arange(S).view(1, S) < torch.from_numpy(n).view(f, 1))
    hit = torch.gather(xy, 1, m.clamp(min=0).unsqueeze(-1).expand(f, S, 2))
    q2 = ((hit - _t(samples, dtype)) ** 2).sum(-1)
    active = used & (q2.detach().sqrt() > margin)
    r = torch.where(active, torch.where(active, q2, torch.ones_like(q2)).sqrt() - margin, torch.zeros_like(q2))
    e_cov = torch.where(active, rho(r * r, sigma), torch.zeros_like(r)).sum(1) / torch.from_numpy(np.maximum(n, 1)).to(dtype)
    return e_in, e_cov, outside


def energy_and_gradient(points, d2, samples, counts, matches, camera, sigma, margin, dtype=F64):
    """numpy: e_in [F], e_cov [F], outside [F], g_in [F,V,3], g_cov [F,V,3] (the gradients of sum_t e_in[t] and of sum_t e_cov[t])."""
    p = _t(points, dtype).clone().requires_grad_(True)
    e_in, e_cov, outside = energy(p, d2, samples, counts, matches, camera, sigma, margin, dtype)
    g_in, = torch.autograd.grad(e_in.sum(), p, retain_graph=True, allow_unused=True)
    g_cov, = torch.autograd.grad(e_cov.sum(), p, allow_unused=True)
    z = torch.zeros_like(p)
    return (e_in.detach().numpy(), e_cov.detach().numpy(), outside.numpy(), (z if g_in is None else g_in).numpy(), (z if g_cov is None else g_cov).numpy())


# ---------------------------------------------------------------------------------------------- the scene
def _state(poses, shape, trans, dtype=F64):
    poses = _t(np.asarray(poses, np.float64), dtype)
    return {'root': poses[:, 0].clone(), 'body': poses[:, 1:].clone(), 'trans': _t(np.asarray(trans, np.float64), dtype).clone(),
            'beta': _t(np.asarray(shape, np.float64), dtype).view(1, -1).clone()}


def world_vertices(state, dtype=F64):
    m = gtwin.Model(base.model(), dtype=dtype)
    f = state['root'].shape[0]
    theta = torch.cat([state['root'].view(f, 1, 3), state['body']], 1)
    out = gtwin.forward(m, state['beta'].expand(f, -1), theta)
    return out["verts"] + state['trans'].view(f, 1, 3), out["joints"] + state['trans'].view(f, 1, 3)


@functools.lru_cache(maxsize=None)
def scene():
    """The scene of tests/_smplfit_scene.py, imported as it is, plus: `masks` [F,688,544] uint8, the union of discs of radius 6 round
    the true projected vertices; `keypoints` with the four arm joints at confidence 0; `xy_true` [F,V,2]; the float64 field."""
    s = dict(base.scene())
    truth = _state(s["poses"], s["beta"], s["trans"])
    with torch.no_grad():
        xy, front = project(world_vertices(truth)[0], s["camera"])
    xy = xy.numpy()
    assert bool(front.all()) and xy[..., 0].min() >= DISC and xy[..., 0].max() <= W - 1 - DISC and xy[..., 1].min() >= DISC and xy[..., 1].max() <= H - 1 - DISC
    masks = np.zeros((base.F, H, W), np.uint8)
    for t in range(base.F):
        for a, b in xy[t]:
            x0, y0 = int(np.floor(a)) - DISC, int(np.floor(b)) - DISC
            yy, xx = np.mgrid[y0:y0 + 2 * DISC + 2, x0:x0 + 2 * DISC + 2]
            masks[t, y0:y0 + 2 * DISC + 2, x0:x0 + 2 * DISC + 2] |= ((xx - a) ** 2 + (yy - b) ** 2 <= DISC * DISC).astype(np.uint8)
    kp = s["keypoints"].copy()
    kp[:, list(ARMS), 2] = 0.0
    samples, counts = contour_samples(masks, SAMPLES)
    s.update({"masks": masks, "keypoints": kp, "xy_true": xy, "d2": edt_two_pass(masks), "samples": samples, "counts": counts, "truth": truth})
    return s


def vertex_error(state):
    """The mean 2-D distance, in pixels, between the state's projected vertices and the true ones (float64)."""
    s = scene()
    st = {k: v.detach().to(F64) for k, v in state.items()}
    with torch.no_grad():
        xy, _ = project(world_vertices(st)[0], s["camera"])
    return float(np.linalg.norm(xy.numpy() - s["xy_true"], axis=-1).mean())


@functools.lru_cache(maxsize=None)
def keypoint_fit():
    """The keypoint-only fit with the arms blind (float64, tests/_smplgrad_ref.py::fit_sequence): where the silhouette rounds start."""
    s = scene()
    out = gtwin.fit_sequence(base.model(), s["keypoints"], s["camera"], base.STAGES)
    return {"poses": out["poses"], "shape": out["shape"], "trans": out["trans"]}


def _keypoint_energy(joints, kp, camera, sigma, dtype):
    xy, front = project(joints, camera, dtype)
    kp = _t(kp, dtype)
    use = front & torch.isfinite(kp).all(-1) & (kp[..., 2] != 0)
    tgt = torch.where(use.unsqueeze(-1), kp, torch.zeros_like(kp))
    r2 = ((xy - tgt[..., :2]) ** 2).sum(-1)
    return torch.where(use, tgt[..., 2] ** 2 * rho(r2, sigma), torch.zeros_like(r2)).sum()


@functools.lru_cache(maxsize=None)
def silhouette_fit(dtype=F64, stages=SIL_STAGES):
    """The silhouette rounds of smpl_fit.fit_sequence restated in `dtype` on the CPU, from keypoint_fit(): the state at the end (tensors)
    and the energy of every iteration."""
    s = scene()
    cam, kp = s["camera"], s["keypoints"]
    start = keypoint_fit()
    st = _state(start["poses"], start["shape"], start["trans"], dtype)
    names = ['root', 'body', 'trans', 'beta']
    history = []
    for iters, lr, l_theta, l_beta, l_s, l_in, l_cov in stages:
        cur = {k: v.detach().clone().requires_grad_(True) for k, v in st.items()}
        mom = {k: (torch.zeros_like(cur[k]), torch.zeros_like(cur[k])) for k in names}
        for it in range(1, iters + 1):
            verts, joints = world_vertices(cur, dtype)
            E = _keypoint_energy(joints, kp, cam, 100., dtype)
            E = E + l_theta * (cur['body'] ** 2).sum() + l_beta * (cur['beta'] ** 2).sum() + l_s * ((joints[1:] - joints[:-1]) ** 2).sum()
            matches, _ = match(verts.detach(), s["samples"], s["counts"], cam, dtype)
            e_in, e_cov, _ = energy(verts, s["d2"], s["samples"], s["counts"], matches, cam, SIGMA, MARGIN, dtype)
            E = E + l_in * e_in.sum() + l_cov * e_cov.sum()
            history.append(float(E.detach()))
            grads = torch.autograd.grad(E, [cur[k] for k in names])
            with torch.no_grad():
                for k, g in zip(names, grads):
                    m1, m2 = mom[k]
                    m1.mul_(0.9).add_(g, alpha=0.1)
                    m2.mul_(0.999).addcmul_(g, g, value=0.001)
                    cur[k] -= lr * (m1 / (1 - 0.9 ** it)) / (m2.sqrt() / np.sqrt(1 - 0.999 ** it) + 1e-8)
        st = {k: v.detach() for k, v in cur.items()}
    return st, np.array(history)
