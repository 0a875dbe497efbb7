"""Float64 references and seeded cases for the fused LBS kernels and the kinematic chain (tests/test_lbs_ref_cpu.py checks this
file against finite differences and closed forms, tests/test_lbs_paths_gpu.py holds csrc/lbs.hip to it).  Host only: numpy and
torch on the CPU.

The references are oracle.torch_oracle's lbs_forward / lbs_transforms / compute_jacobian evaluated in double.  lbs_forward builds the
posed transforms from the poses itself; the kernels take the transforms, and their Abar is the cotangent of the transforms, so
`lbs_from_transforms` runs lbs_forward with the transforms given (test_lbs_ref_cpu pins that this is the same function).
"""
import contextlib
from types import SimpleNamespace

import numpy as np
import torch

from oracle import fixtures as fx
from oracle import torch_oracle as orc

VOL_DHW = (9, 13, 11)
FRAC_LO, FRAC_HI = 0.05, 0.95          # guaranteed range of an interior point's cell fraction (as the float32 kernel computes it)
OUT_MARGIN = 1e-2                      # an outside point lies at least this share of the box extent beyond a face


def apose():
    """The A-pose the skinner is built with in the GPU tests (utils.smpl_tmp_Apose(1)), restated here to stay host only."""
    pose = np.zeros((24, 3), np.float32)
    a, b = 7. / 180. * np.pi, 55. / 180. * np.pi
    pose[1, 2], pose[2, 2], pose[16, 2], pose[17, 2] = a, -a, -b, b
    return torch.from_numpy(pose)


def constants(init_pose=None):
    """The skinner's constants in double.  init_pose [24,4,4]: the GPU tests pass the LBSkinner's own float32 buffer, so that both
    sides use the same numbers; without it, the oracle's inverse rest chain of the A-pose."""
    Js = fx.synthetic_joints().double()
    if init_pose is None:
        init_pose = orc.make_init_pose_inverse(apose().double(), Js)
    return SimpleNamespace(ws=fx.synthetic_lbs_volume(VOL_DHW).double(), b_min=torch.tensor(fx.LBS_BMIN).float().double(),
                           b_max=torch.tensor(fx.LBS_BMAX).float().double(), Js=Js, init_pose=init_pose.double().view(24, 4, 4))


# ------------------------------------------------------------------------------------------------ float64 references
@contextlib.contextmanager
def _given_transforms(A):
    old = orc.lbs_transforms
    orc.lbs_transforms = lambda *a, **k: (A, None)
    try:
        yield
    finally:
        orc.lbs_transforms = old


def lbs_from_transforms(ps, A, trans, K, batch_inds=None, tps=None):
    """orc.lbs_forward with the posed transforms A [N,24,4,4] given instead of derived from poses.  ps [P,3] with batch_inds or
    [N,V,3] without."""
    with _given_transforms(A):
        return orc.lbs_forward(ps, A.new_zeros(A.shape[0], 24, 3), trans, K.ws, K.b_min, K.b_max, K.Js, K.init_pose, batch_inds=batch_inds, tps=tps)


def transforms(poses, K):
    """A [N,24,4,4] of the oracle's chain."""
    return orc.lbs_transforms(poses.double(), K.Js, K.init_pose)[0]


def lbs_reference(p, A, trans, bi, K, wy=None, wJ=None, tps=None):
    """y, J = dy/dp and the gradients of <wy,y> + <wJ,J> with respect to the points (pbar [P,3]), the posed transforms (Abar
    [N,24,12]: the top three rows, as the kernels emit them) and the translations (transbar [N,3]).  wJ None: first order only (the
    sr_lbs_bwd contract); wy None with wJ: a cotangent on J alone.  With tps the weights are looked up there and only y is returned."""
    p = p.double().clone().requires_grad_(True)
    A = A.double().clone().requires_grad_(True)
    t = trans.double().clone().requires_grad_(True)
    if tps is not None:
        return SimpleNamespace(y=lbs_from_transforms(p, A, t, K, bi, tps.double()).detach())
    y = lbs_from_transforms(p, A, t, K, bi)
    out = SimpleNamespace(y=y.detach())
    if wy is None and wJ is None:
        out.J = orc.compute_jacobian(p, y, False, False).detach()
        return out
    J = orc.compute_jacobian(p, y, True, wJ is not None)
    out.J = J.detach()
    s = 0.
    if wy is not None:
        s = s + (y * wy.double()).sum()
    if wJ is not None:
        s = s + (J * wJ.double()).sum()
    gp, gA, gt = torch.autograd.grad(s, [p, A, t], allow_unused=True)
    out.pbar = gp
    out.Abar = gA[:, :, :3, :].reshape(A.shape[0], 24, 12)
    out.transbar = torch.zeros_like(t) if gt is None else gt
    return out


def lbs_pose_reference(p, poses, trans, bi, K, wy, wJ=None):
    """The same scalar differentiated down to the poses, through the oracle's own chain: (pbar, posebar, transbar)."""
    p = p.double().clone().requires_grad_(True); po = poses.double().clone().requires_grad_(True); t = trans.double().clone().requires_grad_(True)
    y = orc.lbs_forward(p, po, t, K.ws, K.b_min, K.b_max, K.Js, K.init_pose, batch_inds=bi)
    s = (y * wy.double()).sum()
    if wJ is not None:
        s = s + (orc.compute_jacobian(p, y, True, True) * wJ.double()).sum()
    return torch.autograd.grad(s, [p, po, t])


def chain_reference(poses, K, wA=None, wG=None):
    """G (posed chain), A = G init_pose and posebar of <wA,A> + <wG,G>.  The oracle returns A and the posed joints only; the full G
    is A times the inverse of init_pose (a rigid transform per joint), and its translation column is the oracle's joints."""
    po = poses.double().clone().requires_grad_(True)
    A, newJ = orc.lbs_transforms(po, K.Js, K.init_pose)
    G = A @ torch.linalg.inv(K.init_pose).view(1, 24, 4, 4)
    out = SimpleNamespace(G=G.detach(), A=A.detach(), newJ=newJ.detach())
    if wA is not None or wG is not None:
        s = 0.
        if wA is not None:
            s = s + (A * wA.double()).sum()
        if wG is not None:
            s = s + (G * wG.double()).sum()
        out.posebar = torch.autograd.grad(s, po)[0]
    return out


def chain_poses(B, seed=61):
    """[B,24,3]: moderate rotations, with the cases the dual-number Rodrigues has to survive planted in fixed places: exact-zero
    joints, a whole zero pose, rotations of magnitude 1e-4 and rotations near pi."""
    poses = fx.det_tensor((B, 24, 3), seed, 0.4)
    poses[0, 3] = 0.0                                                   # exact zero: the +1e-8 path
    poses[0, 7] = torch.tensor([6e-5, -7e-5, 4e-5])                      # |theta| ~ 1e-4
    poses[0, 11] = 3.1 * torch.nn.functional.normalize(torch.tensor([1.8, -2.0, 1.6]), dim=0)       # |theta| = 3.1: near pi
    for b in range(B):
        poses[b, (5 * b + 2) % 24] = 0.0
        poses[b, (7 * b + 9) % 24] *= 1e-4 / 0.4
    if B > 2:
        poses[B // 2] = 0.0                                             # a whole zero pose
        poses[B - 1, 0] = 3.13 * torch.nn.functional.normalize(torch.tensor([-2.2, 1.9, 1.1]), dim=0)
    return poses


# ------------------------------------------------------------------------------------------------ seeded cases
def _sizes():
    D, H, W = VOL_DHW
    return np.array([W, H, D])


def unnormalised_f32(p):
    """The sampler coordinate of csrc/lbs_device.h make_axis before clipping, in its float32 arithmetic: p [P,3] float32 -> [P,3]."""
    p = np.asarray(p, np.float32)
    bmin, bmax = np.asarray(fx.LBS_BMIN, np.float32), np.asarray(fx.LBS_BMAX, np.float32)
    n = np.float32(2.) * (p - bmin) / (bmax - bmin) - np.float32(1.)
    t = (n + np.float32(1.)) * _sizes().astype(np.float32)
    return ((t.astype(np.float64) - 1.0) / 2.0).astype(np.float32)


def _from_unnormalised(t):
    bmin, bmax = np.asarray(fx.LBS_BMIN, np.float64), np.asarray(fx.LBS_BMAX, np.float64)
    return bmin + (2.0 * t + 1.0) / _sizes() * (bmax - bmin) / 2.0


def interior_points(P, seed):
    """Placed cell by cell (every cell of the volume in turn, from a seeded start), at a seeded fraction in [0.1, 0.9] per axis."""
    S = _sizes()
    ncell = int(np.prod(S - 1))
    cell = (np.arange(P, dtype=np.int64) * 389 + seed * 131) % ncell
    c = np.stack([cell % (S[0] - 1), (cell // (S[0] - 1)) % (S[1] - 1), cell // ((S[0] - 1) * (S[1] - 1))], 1)
    frac = 0.5 + 0.4 * fx.det_array((P, 3), seed, 1.0, np.float64)
    p = _from_unnormalised(c + frac).astype(np.float32)
    t = unnormalised_f32(p)
    f = t - np.floor(t)
    assert (np.floor(t) == c).all() and (f >= FRAC_LO).all() and (f <= FRAC_HI).all()
    return p


def outside_points(P, seed):
    """Beyond the box on one, two or three axes (point i: the non-empty axis subset 1 + i % 7, side by seed), by 1 % .. 21 % of the
    extent; interior on the other axes."""
    bmin, bmax = np.asarray(fx.LBS_BMIN, np.float64), np.asarray(fx.LBS_BMAX, np.float64)
    p = interior_points(P, seed + 1).astype(np.float64)
    r = fx.det_array((P, 3), seed + 2, 1.0, np.float64)
    out = (((1 + np.arange(P) % 7)[:, None] >> np.arange(3)[None, :]) & 1).astype(bool)
    beyond = (2 * OUT_MARGIN + 0.2 * np.abs(r)) * (bmax - bmin)
    far = np.where(r < 0, bmin - beyond, bmax + beyond)
    return np.where(out, far, p).astype(np.float32), out


def lattice_points(P, seed):
    """Exactly at voxel centres (even i) and exactly on box faces (odd i: one to three axes on a face, the others on centres)."""
    S = _sizes()
    bmin, bmax = np.asarray(fx.LBS_BMIN, np.float32), np.asarray(fx.LBS_BMAX, np.float32)
    r = fx.det_array((P, 3), seed, 1.0, np.float64)
    c = np.floor((r * 0.5 + 0.5) * S).clip(0, S - 1)
    p = _from_unnormalised(c).astype(np.float32)
    i = np.arange(P)
    face = ((((1 + (i // 2) % 7)[:, None] >> np.arange(3)[None, :]) & 1).astype(bool)) & (i % 2 == 1)[:, None]
    return np.where(face, np.where(r < 0, bmin, bmax), p).astype(np.float32)


ORDERS = ("sorted", "interleaved", "empty", "last")


def frame_ids(P, N, order):
    """[P] int64.  sorted: contiguous runs; interleaved: round robin (several FramePass passes per wave); empty: sorted over all
    frames but N // 2, which owns no point; last: every point in frame N - 1."""
    i = np.arange(P, dtype=np.int64)
    if order == "sorted":
        return (i * N) // P
    if order == "interleaved":
        return i % N
    if order == "last":
        return np.full(P, N - 1, np.int64)
    assert order == "empty" and N >= 2
    used = np.array([f for f in range(N) if f != N // 2], np.int64)
    return used[(i * (N - 1)) // P]


def make_case(P, N, order, seed=1, lattice=False):
    """All tensors float32 / int64 on the CPU.  Points: interior first, then outside (a quarter), then -- forward cases only --
    on-lattice (a sixth), spread over the frames by `order`; `deriv` marks the points whose derivatives are compared (everything
    but the on-lattice class)."""
    n_lat = (P // 6) if lattice else 0
    n_out = (P - n_lat) // 4
    n_in = P - n_lat - n_out
    parts, cls = [interior_points(n_in, seed * 10)], [np.zeros(n_in, np.int64)]
    if n_out:
        parts.append(outside_points(n_out, seed * 10 + 3)[0]); cls.append(np.ones(n_out, np.int64))
    if n_lat:
        parts.append(lattice_points(n_lat, seed * 10 + 6)); cls.append(np.full(n_lat, 2, np.int64))
    p, cls = np.concatenate(parts, 0), np.concatenate(cls, 0)
    mix = np.argsort(fx.det_array((P,), seed * 10 + 7, 1.0, np.float64), kind="stable")         # classes mixed within every wave
    p, cls = p[mix], cls[mix]
    c = SimpleNamespace(P=P, N=N, order=order, p=torch.from_numpy(p), cls=torch.from_numpy(cls), bi=torch.from_numpy(frame_ids(P, N, order)))
    c.deriv = c.cls != 2
    c.poses = fx.det_tensor((N, 24, 3), seed * 10 + 8, 0.2)
    c.trans = fx.det_tensor((N, 3), seed * 10 + 9, 0.05)
    c.wy, c.wJ = fx.det_tensor((P, 3), seed * 10 + 4, 1.0), fx.det_tensor((P, 3, 3), seed * 10 + 5, 1.0)
    c.empty = sorted(set(range(N)) - set(c.bi.tolist()))
    return c


NFRAMES = (1, 3, 8, 9, 14, 15, 32)
POINTS = (1, 63, 64, 65, 255, 257, 1000)


def case_table():
    """(nframes, P, order): every frame count with every order and every point count with every order (the point count steps
    with both indices), 28 cases.  One frame cannot leave a frame empty: its point count goes to three frames instead."""
    out = [(3, POINTS[2], "empty")]
    for i, n in enumerate(NFRAMES):
        for j, order in enumerate(ORDERS):
            if n == 1 and order == "empty":
                continue
            out.append((n, POINTS[(i + j) % len(POINTS)], order))
    return out
