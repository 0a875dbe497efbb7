"""Operators of the winding-number inside / outside test (csrc/winding.hip): GPU tensors only, no autograd.
`evaluate.py` is the public interface.  The stable sort of the leaf keys and the run starts are torch's; everything per face, per node
and per point is a HIP kernel.  Two calls give identical bits.  A WindingIndex is built from a surfdist_ops.Surface, which prepares
the mesh once, shares its packed corners with the grid and keeps the pyramid of the default depth (Surface.pyramid).

The entry points are declared in csrc/winding_abi.h and bound here (_lib.bind_header): a library without them fails this import."""
import math
import os

import numpy as np
import torch

from . import _lib
from . import surfdist_ops as sd
from .build import CSRC
from .mesh_prep_ops import _lists

_DEFINES, _ = _lib.bind_header(os.path.join(CSRC, "winding_abi.h"))
MAX_LEVELS = _DEFINES["SR_WINDING_MAX_LEVELS"]
NODE_FLOATS = _DEFINES["SR_WINDING_NODE_FLOATS"]          # N [3], c [3], A, r
LEAF_FACTOR = 2.0          # default leaf cell = LEAF_FACTOR sqrt(total area / faces) (tools/winding_bench.py sweeps it)
WIDEN = 1. + 2. ** -10     # the cube's side over the longest side of the mesh's box: no centroid lies on the far boundary
BETA = 3.0                 # a node is taken as one dipole from farther than BETA radii


def level_offset(level):
    """Index of the first node of `level` in the pyramid: (8^level - 1) / 7."""
    return ((1 << (3 * level)) - 1) // 7


def cube(lo, hi):
    """(corner [3] float32, side float32) of the tree's cube round the box lo / hi [3], in float32 arithmetic: side = WIDEN times the
    box's longest side (1 for a box that is one point), centred on the box."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    side = np.float32((hi - lo).max()) * np.float32(WIDEN)
    if not side > 0:
        side = np.float32(1.)
    return (lo + hi) * np.float32(0.5) - np.float32(0.5) * side, side


def default_levels(side, area, faces, leaf_factor=LEAF_FACTOR):
    """clamp(round(log2(side / leaf)), 0, MAX_LEVELS), leaf = leaf_factor sqrt(area / faces); 0 for a mesh without area."""
    leaf = float(leaf_factor) * math.sqrt(area / faces) if area > 0 and math.isfinite(area) else 0.
    if not leaf > 0:
        return 0
    return int(min(max(math.floor(math.log2(float(side) / leaf) + 0.5), 0), MAX_LEVELS))


def signed_volume(verts, faces):
    """sum_f a . (b x c) / 6 in double (torch ops), on the device: positive for a closed mesh with outward faces."""
    p = verts.detach().double()[faces]
    return (p[:, 0] * torch.linalg.cross(p[:, 1], p[:, 2])).sum() / 6.


class WindingIndex:
    """The octree pyramid of a Surface (layout: csrc/winding_abi.h): `corner` [3] (device), `cell` (the leaf's side), `levels`, `nodes`
    [(8^(levels+1) - 1) / 7, NODE_FLOATS] float32, `leaf_start` [8^levels + 1] int64, `leaf_faces` [F] int32 (every leaf's faces in
    ascending index); shared with the Surface: `verts`, `faces`, `tri`; `volume`, the mesh's signed volume as a Python float, and
    `flipped` = volume < 0: the faces wind inward, and winding_number returns -w so that inside stays w >= 1/2."""

    def __init__(self, surface, levels=None, leaf_factor=None):
        """`levels` in [0, MAX_LEVELS] defaults to default_levels of the cube's side, the total area and F, with `leaf_factor`
        (default LEAF_FACTOR).  One device -> host read: the signed volume."""
        verts, faces, tri = self.verts, self.faces, self.tri = surface.verts, surface.faces, surface.tri
        corner_h, side = cube(surface.box[:3], surface.box[3:])
        F, dev = tri.shape[0], tri.device
        if levels is None:
            leaf_factor = LEAF_FACTOR if leaf_factor is None else leaf_factor
            if not (leaf_factor > 0 and math.isfinite(leaf_factor)):
                raise ValueError(f"leaf_factor must be a positive float, got {leaf_factor}")
            levels = default_levels(side, surface.area, F, leaf_factor)
        self.levels = levels = int(levels)
        if not 0 <= levels <= MAX_LEVELS:
            raise ValueError(f"levels in [0, {MAX_LEVELS}] expected, got {levels}")
        self.cell = float(side / np.float32(1 << levels))
        self.corner = torch.from_numpy(corner_h).to(dev)
        key = torch.empty((F,), dtype=torch.int64, device=dev)
        _lib.launch("sr_winding_keys", tri, tri, F, 1, self.corner, self.cell, levels, key)
        order, self.leaf_start = _lists(key, 1 << (3 * levels))
        self.leaf_faces = order.to(torch.int32).contiguous()
        self.nodes = torch.empty((level_offset(levels + 1), NODE_FLOATS), dtype=torch.float32, device=dev)
        _lib.launch("sr_winding_leaves", tri, tri, F, self.leaf_start, self.leaf_faces, levels, self.nodes)
        for level in range(levels - 1, -1, -1):
            _lib.launch("sr_winding_fold", self.nodes, self.nodes, level, levels)
        self.volume = float(signed_volume(verts, faces))
        self.flipped = self.volume < 0

    @classmethod
    def build(cls, verts, faces, levels=None, leaf_factor=LEAF_FACTOR):
        """The pyramid of verts [V,3] / faces [F,3] (GPU tensors), refused as surfdist_ops.Surface refuses."""
        return cls(sd.Surface(verts, faces, "WindingIndex.build"), levels, leaf_factor)


def winding_number(points, index, method="tree", beta=BETA, presort=True):
    """w [P] float32 of points [P,3] against the mesh of `index`, in the caller's order: the generalized winding number, 1 inside and 0
    outside a closed mesh whichever way its faces wind (index.flipped), in between near a hole.  A point with a NaN or Inf coordinate
    gives NaN.  method "brute" sums every face's solid angle (sr_winding_brute); "tree" walks the pyramid (sr_winding_query) and takes
    a node from farther than `beta` radii as one dipole: `beta` is a finite float >= 1, or inf, which opens every node and sums the
    same faces leaf by leaf.  With `presort` the points are visited in the order of their leaf keys, which only changes the speed."""
    _lib.require_gpu(points)
    points = sd._points(points)
    P, dev = points.shape[0], points.device
    if method not in ("tree", "brute"):
        raise ValueError(f"method must be 'tree' or 'brute', got {method!r}")
    beta = float(beta)
    if not beta >= 1.:
        raise ValueError(f"beta must be a float >= 1 or inf, got {beta}")
    w = torch.empty((P,), dtype=torch.float32, device=dev)
    if P == 0:
        return w
    F = index.faces.shape[0]
    if method == "brute":
        _lib.launch("sr_winding_brute", points, points, P, index.tri, F, w)
        return -w if index.flipped else w
    if presort:
        key = torch.empty((P,), dtype=torch.int64, device=dev)
        _lib.launch("sr_winding_keys", points, points, P, 0, index.corner, index.cell, index.levels, key)
        points, back = sd.in_key_order(points, key)
    _lib.launch("sr_winding_query", points, points, P, index.tri, F, index.nodes, index.levels, index.leaf_start, index.leaf_faces,
                beta, int(math.isinf(beta)), w)
    if presort:
        w = back(w)[0]
    return -w if index.flipped else w
