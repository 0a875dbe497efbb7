"""The references of the raster path tests (tests/test_raster_paths_cpu.py, tests/test_raster_paths_gpu.py), computed once per scene and
shared: oracle/raster_oracle.py (the float32 restatement of the same operation; `render_point_silhouette` evaluated on float64 leaves
gives the mask and, by autograd, the gradient) and oracle/raster_witness.py (independent float64 brute force with an ambiguity mask).

A pixel is COMPARABLE when the witness does not call it ambiguous and the oracle agrees with the witness there -- on coverage and winner
for meshes, on the mask to POINT_AGREE for points.  At most MAX_LEFT_OUT of a scene's pixels may fall outside that set (asserted by both
test files); a scene that exceeds it has to change, not the cap.  `deep_pixel` is held to the oracle alone: its equal-z pairs across
rank K are ambiguous to the witness by design, the oracle sorts them by (z, index).

Everything returned is cached; the arrays are made read-only."""
import functools

import numpy as np
import torch

import _raster_scenes as rs
from oracle import raster_oracle as ro
from oracle import raster_witness as rw

MAX_LEFT_OUT = 0.01
POINT_AGREE = 1e-5


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def point_scene(name):
    return _frozen({f.__name__[len("points_"):]: f for f in rs.POINT_SCENES}[name]())


@functools.lru_cache(maxsize=None)
def mesh_scene(name):
    return _frozen({f.__name__[len("mesh_"):]: f for f in rs.MESH_SCENES}[name]())


def cotangent(shape):
    return np.random.default_rng(41).uniform(-1.0, 1.0, shape)


@functools.lru_cache(maxsize=None)
def point_reference(name, K):
    """-> dict: mask [N,H,W] float64 (oracle), cot [N,H,W] the cotangent (zero outside comparable), grad [N,V,2] float64 of
    sum(mask * cot) with respect to xy_ndc, idx [N,H,W,K] the oracle's selection, count [N,H,W] covering points (oracle selection capped at K; the witness's uncapped count where it ran),
    comparable [N,H,W] bool, left_out (share of pixels outside comparable)."""
    s = point_scene(name)
    H, (N, V) = s["H"], s["z"].shape
    # the camera under which ndc_projection is the identity on (x z, y z, z): focal H/2, principal point (H - 1)/2, no rotation
    xy = torch.tensor(s["xy"], dtype=torch.float64).requires_grad_(True)
    z = torch.tensor(s["z"], dtype=torch.float64)
    world = torch.cat([xy * z[..., None], z[..., None]], -1)
    half = torch.tensor([H / 2.0, H / 2.0], dtype=torch.float64)
    # (largest_k: no pixel has more than 16 covering points -- asserted by its test from the witness's uncapped count -- so the K nearest
    # of K = 65 536 are those of K = 16; the oracle's [N,H,W,K] arrays are built for the latter)
    mask, idx = ro.render_point_silhouette(world, half, half - 0.5, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64),
                                           H, H, s["radius"], min(K, rs.LARGEST_K_COVER) if name == "largest_k" else K)
    mask_np = mask.detach().numpy()
    count = (idx >= 0).sum(-1).numpy()
    comparable = np.ones(mask_np.shape, bool)
    if name != "deep_pixel":
        count = np.empty(mask_np.shape, np.int64)
        for n in range(N):
            wm, count[n], amb = rw.points(s["xy"][n], s["z"][n], H, H, s["radius"], K)
            comparable[n] = ~amb & (np.abs(wm - mask_np[n]) <= POINT_AGREE)
    cot = cotangent(mask_np.shape) * comparable                          # the gradient, too, is taken over the comparable pixels only
    (grad,) = torch.autograd.grad(mask, xy, torch.from_numpy(cot))
    return _frozen(dict(mask=mask_np, grad=grad.numpy(), cot=cot, idx=idx.numpy(), count=count, comparable=comparable,
                        left_out=1.0 - comparable.mean()))


@functools.lru_cache(maxsize=None)
def mesh_reference(name):
    """-> dict: face [N,H,W] (index into faces, -1), bary [N,H,W,3], zbuf [N,H,W] of the oracle, comparable [N,H,W], left_out."""
    s = mesh_scene(name)
    H, N, faces = s["H"], s["z"].shape[0], s.get("faces_expected", s["faces"])
    verts = np.concatenate([s["xy"], s["z"][..., None]], -1)
    p2f, bary, zbuf = ro.rasterize_meshes(verts, faces, H, H)
    face = np.where(p2f[..., 0] >= 0, p2f[..., 0] - np.arange(N)[:, None, None] * len(faces), -1)
    comparable = np.empty(face.shape, bool)
    for n in range(N):
        wf, _, _, amb = rw.mesh(verts[n], faces, H, H)
        comparable[n] = ~amb & (wf == face[n])
    return _frozen(dict(face=face, bary=bary[..., 0, :], zbuf=zbuf[..., 0], comparable=comparable, left_out=1.0 - comparable.mean()))
