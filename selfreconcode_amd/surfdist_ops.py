"""Operators of the surface-distance evaluation (csrc/surfdist.hip): GPU tensors only, no autograd.  `evaluate.py` is
the public interface.  Sorting, cumulative sums and the cell table are torch's; everything per face, per point and per sample is a HIP
kernel.  Two calls give identical bits.

A mesh is prepared once, as a `Surface`: cleaned faces, box, packed corners, areas.  Its grid (`MeshIndex`), its octree pyramid
(winding_ops.WindingIndex) and its face normals are built on first use and kept by the Surface, which owns that cache: whoever needs
several of them for one mesh holds the Surface.  Nothing is kept across vertex positions: a moved mesh is a new Surface."""
import numpy as np
import torch

from . import _lib
from . import mesh_prep_ops as mp

CELL_FACTOR = 2.0          # default cell = CELL_FACTOR sqrt(total area / faces): about 1.3 mean edges (tools/surfdist_bench.py sweeps it)
MAX_CELLS = 1 << 24        # cap on nx ny nz
PAIR_FACTOR = 64           # cap on the (cell, face) pairs, as a multiple of the face count
MAX_DOUBLINGS = 64


def _points(points):
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points [P,3] expected, got {tuple(points.shape)}")
    return _lib.f32c(points)


def face_areas_cum(verts, faces):
    """[F] float64: the cumulative sum of the face areas |(b - a) x (c - a)| / 2, evaluated in double (torch ops)."""
    _lib.require_gpu(verts, faces)
    p = verts.detach().double()[_lib.i64c(faces)]
    return torch.cumsum(0.5 * torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=1), 0).contiguous()


def unit_normals(verts, faces):
    """[F,3] float32 unit normals (b - a) x (c - a) evaluated in double; zero for a face without area."""
    p = verts.double()[faces]
    nrm = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = nrm.norm(dim=1, keepdim=True)
    return torch.where(length > 0, nrm / length.clamp_min(1e-300), torch.zeros_like(nrm)).float()


def in_key_order(points, key):
    """(points [P,3] in the ascending order of key [P] (stable), back): back(x, ...) returns per-point results of that order in the
    caller's order.  A wave then walks neighbouring cells; the order only changes the speed of a per-point kernel."""
    order = torch.sort(key, stable=True)[1]

    def back(*results):
        inv = torch.empty_like(order)
        inv[order] = torch.arange(order.shape[0], dtype=torch.int64, device=order.device)
        return tuple(x[inv] for x in results)
    return points[order].contiguous(), back


class Surface:
    """A triangle mesh prepared once: `verts` [V,3] float32, `faces` [F,3] int64 (cleaned), `tri` [F,12] float32 (corners a, b, c of
    every face and three floats of padding: three aligned float4 per face), `cum_area` [F] float64 (face_areas_cum), `area` (its last
    entry as a Python float), `lo` [3] (device) and `box` [6] float32 (numpy: lo, hi of the vertices).  Unpacks as (verts, faces)."""

    def __init__(self, verts, faces, what="Surface", cleaned=False):
        """verts [V,3] / faces [F,3] (GPU tensors).  Rows with a negative index are dropped (clean_faces); ValueError, with `what` in
        front, for an index >= V or no faces left, and for a non-finite vertex.  `cleaned`: the faces are another Surface's.  Device ->
        host reads: the largest index, the non-finite flag, the box and the total area."""
        _lib.require_gpu(verts, faces)
        self.verts = mp._verts2(verts)
        self.faces = faces if cleaned else mp.clean_faces(faces)
        if self.faces.shape[0] == 0:
            raise ValueError(f"{what}: the mesh has no faces")
        if not cleaned and int(self.faces.max()) >= self.verts.shape[0]:
            raise ValueError(f"{what}: face indices outside [0, {self.verts.shape[0]})")
        lo, hi = mp.mesh_bounds(self.verts)
        self.lo, self.box = lo.contiguous(), torch.cat([lo, hi]).cpu().numpy()
        self.tri = torch.zeros((self.faces.shape[0], 12), dtype=torch.float32, device=self.verts.device)
        self.tri[:, :9] = self.verts[self.faces].reshape(-1, 9)
        self.cum_area = face_areas_cum(self.verts, self.faces)
        self.area = float(self.cum_area[-1])
        self._grid = self._pyramid = self._normals = None

    @classmethod
    def of(cls, mesh, what):
        """`mesh` itself if it is a Surface, else the Surface of the pair mesh = (verts, faces)."""
        return mesh if isinstance(mesh, cls) else cls(mesh[0], mesh[1], what)

    def __iter__(self):
        return iter((self.verts, self.faces))

    def moved(self, verts):
        """The Surface of the same faces over other positions verts [V,3]: only the cleaned faces are reused."""
        if verts.shape != self.verts.shape:
            raise ValueError(f"verts {tuple(self.verts.shape)} expected, got {tuple(verts.shape)}")
        return Surface(verts, self.faces, cleaned=True)

    def grid(self, cell=None):
        """The MeshIndex: kept for the default cell, built anew for a given one."""
        if cell is None and self._grid is None:
            self._grid = MeshIndex(self)
        return self._grid if cell is None else MeshIndex(self, cell)

    def pyramid(self, levels=None, leaf_factor=None):
        """The winding_ops.WindingIndex: kept for the default depth, built anew for given `levels` or `leaf_factor`."""
        from .winding_ops import WindingIndex
        default = levels is None and leaf_factor is None
        if default and self._pyramid is None:
            self._pyramid = WindingIndex(self)
        return self._pyramid if default else WindingIndex(self, levels, leaf_factor)

    def face_normals(self):
        """unit_normals of the faces."""
        if self._normals is None:
            self._normals = unit_normals(self.verts, self.faces)
        return self._normals

    def sample(self, n, seed):
        """(points [n,3], face [n], normals [n,3]) as sample_surface draws them; not kept (no two callers ask for the same)."""
        return _sample(self.tri, self.cum_area, n, seed)


class MeshIndex:
    """A uniform grid over a Surface: `cell`, `n` = (nx, ny, nz), `cell_start` [cells + 1] int64, `cell_faces` [pairs] int32 (every
    cell's faces in ascending index), `pairs`; and, shared with the Surface, `verts`, `faces`, `tri`, `cum_area`, `area`, `lo`, `box`."""

    def __init__(self, surface, cell=None):
        """The box is mesh_bounds(verts); a face belongs to every cell its own box overlaps.  `cell` defaults to CELL_FACTOR sqrt(area
        / F) (at least 1/256 of the box's longest side; 1 for a mesh that is one point).  While the grid would have more than MAX_CELLS
        cells or more than PAIR_FACTOR F pairs the cell is doubled and the count repeated, so one huge triangle among small ones costs
        a coarser grid, not memory.  Device -> host reads: the pair total of every counted grid."""
        s = surface
        self.verts, self.faces, self.tri, self.cum_area, self.area, self.lo, self.box = s.verts, s.faces, s.tri, s.cum_area, s.area, s.lo, s.box
        tri, lo, lo_h, hi_h, area = s.tri, s.lo, s.box[:3], s.box[3:], s.area
        F, dev, side = tri.shape[0], tri.device, float((hi_h - lo_h).max())
        if cell is None:
            cell = max(CELL_FACTOR * (area / F) ** 0.5, side / 256.) if np.isfinite(area) else side / 256.
            if not cell > 0:
                cell = 1.
        cell = float(np.float32(cell))
        if not (cell > 0 and np.isfinite(cell)):
            raise ValueError(f"cell must be a positive float32, got {cell}")
        count = torch.empty((F,), dtype=torch.int64, device=dev)
        for _ in range(MAX_DOUBLINGS):
            try:
                n = mp.grid_shape(lo_h, hi_h, cell)
            except ValueError:                                   # (more cells than grid_shape counts: far beyond the cap)
                n = None
            if n is not None and n[0] * n[1] * n[2] <= MAX_CELLS:
                _lib.launch("sr_surfdist_face_cells", tri, tri, F, lo, cell, n[0], n[1], n[2], count)
                pairs = int(count.sum())
                if pairs <= PAIR_FACTOR * F:
                    break
            cell = float(np.float32(2. * cell))
        else:
            raise ValueError(f"MeshIndex.build: no grid within the caps after {MAX_DOUBLINGS} doublings of the cell")
        offset = (torch.cumsum(count, 0) - count).contiguous()
        key = torch.empty((pairs,), dtype=torch.int64, device=dev)
        pair_face = torch.empty((pairs,), dtype=torch.int32, device=dev)
        _lib.launch("sr_surfdist_emit_pairs", tri, tri, F, lo, cell, n[0], n[1], n[2], offset, pairs, key, pair_face)
        order, self.cell_start = mp._lists(key, n[0] * n[1] * n[2])
        self.cell_faces, self.pairs, self.cell, self.n, (self.nx, self.ny, self.nz) = pair_face[order].contiguous(), pairs, cell, n, n

    @classmethod
    def build(cls, verts, faces, cell=None):
        """The grid of verts [V,3] / faces [F,3] (GPU tensors), refused as Surface refuses."""
        return cls(Surface(verts, faces, "MeshIndex.build"), cell)

    def args(self):
        """tri, F, lo, cell, nx, ny, nz, cell_start, cell_faces, pairs: what sr_surfdist_query, sr_icp_accumulate and sr_icp_score take."""
        return (self.tri, self.tri.shape[0], self.lo, self.cell, *self.n, self.cell_start, self.cell_faces, self.pairs)

    def keys(self, points):
        """key [P] int64 of the cells of points [P,3] (mesh_prep_ops.cell_keys)."""
        return mp.cell_keys(points, self.lo, self.cell, self.n)

    def face_normals(self):
        """unit_normals of the faces, evaluated on every call (the Surface keeps its own)."""
        return unit_normals(self.verts, self.faces)


def closest_point(points, index, method="grid", presort=True):
    """(dist [P] f32, face [P] i64, closest [P,3] f32) of points [P,3] against the mesh of `index`, in the caller's order: the
    Euclidean distance to the mesh as a set of closed triangles, the face that attains it (lowest index among equal float32 squared
    distances; indices count the index's cleaned faces) and the closest point on it.  A point with a NaN or Inf coordinate gives (NaN,
    -1, NaN).  method "grid" walks the index (sr_surfdist_query; with `presort` the points are visited in the order of their cell
    keys, which only changes the speed), "brute" loops over all faces (sr_surfdist_brute); both give the same bits."""
    _lib.require_gpu(points)
    points = _points(points)
    P, dev = points.shape[0], points.device
    if method not in ("grid", "brute"):
        raise ValueError(f"method must be 'grid' or 'brute', got {method!r}")
    out = (torch.empty((P,), dtype=torch.float32, device=dev), torch.empty((P,), dtype=torch.int64, device=dev),
           torch.empty((P, 3), dtype=torch.float32, device=dev))
    if P == 0:
        return out
    if method == "brute":
        _lib.launch("sr_surfdist_brute", points, points, P, index.tri, index.tri.shape[0], *out)
        return out
    points, back = in_key_order(points, index.keys(points)) if presort else (points, lambda *x: x)
    _lib.launch("sr_surfdist_query", points, points, P, *index.args(), *out)
    return back(*out)


def _sample(tri, cum_area, n, seed):
    F, dev = tri.shape[0], tri.device
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty((n,), dtype=torch.int64, device=dev)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n:
        _lib.launch("sr_mesh_sample", tri, tri, cum_area, F, n, int(seed), points, face, normals)
    return points, face, normals


def sample_surface(verts, faces, n, seed, cum_area=None):
    """(points [n,3] f32, face [n] i64, normals [n,3] f32): n samples of the surface, area-weighted and stratified (sr_mesh_sample).
    Sample i lies at r_i = (i + xi_i) / n A of the cumulative face areas (`cum_area`, default face_areas_cum of the cleaned faces; A
    its last entry), on the first face whose cumulative area exceeds r_i -- a face without area is never chosen --, at barycentrics (1
    - sqrt u, sqrt u (1 - v), sqrt u v); xi, u, v are (synthetic._splitmix(3 i + {0, 1, 2}, seed) >> 11) 2^-53.  `normals` is the
    face's unit normal.  ValueError for a mesh without area, and as Surface refuses."""
    s = Surface(verts, faces, "sample_surface")
    n = int(n)
    if n < 0:
        raise ValueError(f"n >= 0 expected, got {n}")
    cum_area = s.cum_area if cum_area is None else cum_area
    _lib.require_gpu(cum_area)
    if cum_area.dtype != torch.float64 or cum_area.shape != (s.faces.shape[0],):
        raise ValueError("cum_area [F] float64 expected")
    area = float(cum_area[-1])
    if not (area > 0 and np.isfinite(area)):
        raise ValueError(f"sample_surface: the mesh has total area {area}")
    return _sample(s.tri, cum_area.contiguous(), n, seed)
