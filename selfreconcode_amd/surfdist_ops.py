"""Operators of the surface-distance evaluation (csrc/surfdist.hip): GPU tensors only, no autograd.  `evaluate.py` is
the public interface.  Sorting, cumulative sums and the cell table are torch's; everything per face, per point and per sample is a HIP
kernel.  Two calls give identical bits."""
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


def _mesh(verts, faces, what):
    """(verts [V,3] f32, faces [F,3] i64) with the -1 rows dropped, F > 0 and every index below V (ValueError otherwise)."""
    _lib.require_gpu(verts, faces)
    verts = mp._verts2(verts)
    faces = mp.clean_faces(faces)
    if faces.shape[0] == 0:
        raise ValueError(f"{what}: the mesh has no faces")
    if int(faces.max()) >= verts.shape[0]:
        raise ValueError(f"{what}: face indices outside [0, {verts.shape[0]})")
    return verts, faces


def _pack(verts, faces):
    """tri [F,12] float32: corners a, b, c of every face and three floats of padding (three aligned float4 per face)."""
    tri = torch.zeros((faces.shape[0], 12), dtype=torch.float32, device=verts.device)
    tri[:, :9] = verts[faces].reshape(-1, 9)
    return tri


def face_areas_cum(verts, faces):
    """[F] float64: the cumulative sum of the face areas |(b - a) x (c - a)| / 2, evaluated in double (torch ops)."""
    _lib.require_gpu(verts, faces)
    p = verts.detach().double()[_lib.i64c(faces)]
    return torch.cumsum(0.5 * torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=1), 0).contiguous()


class MeshIndex:
    """A uniform grid over a triangle mesh: `lo` [3] (device), `cell`, `n` = (nx, ny, nz), `cell_start` [cells + 1] int64, `cell_faces`
    [pairs] int32 (every cell's faces in ascending index), `pairs`; and the mesh itself: `verts`, `faces` (cleaned), `tri` [F,12],
    `cum_area` [F] float64 (face_areas_cum) and `area`, its last entry as a Python float."""

    def __init__(self, verts, faces, tri, cum_area, area, lo, cell, n, cell_start, cell_faces):
        self.verts, self.faces, self.tri, self.lo, self.cell, self.n = verts, faces, tri, lo, cell, n
        self.cum_area, self.area = cum_area, area
        self.cell_start, self.cell_faces, self.pairs = cell_start, cell_faces, int(cell_faces.shape[0])
        self._normals = None

    @property
    def nx(self):
        return self.n[0]

    @property
    def ny(self):
        return self.n[1]

    @property
    def nz(self):
        return self.n[2]

    @classmethod
    def build(cls, verts, faces, cell=None):
        """The grid of verts [V,3] / faces [F,3] (GPU tensors).  Rows with a negative index are dropped (clean_faces); ValueError for
        an index >= V, no faces left, or a non-finite vertex.  The box is mesh_bounds(verts); a face belongs to every cell its own
        box overlaps.  `cell` defaults to CELL_FACTOR sqrt(area / F) (at least 1/256 of the box's longest side; 1 for a mesh that is
        one point).  While the grid would have more than MAX_CELLS cells or more than PAIR_FACTOR F pairs the cell is doubled and the
        count repeated, so one huge triangle among small ones costs a coarser grid, not memory.  Device -> host reads: the
        non-finite flag and the box, the total area and the pair total of every counted grid."""
        verts, faces = _mesh(verts, faces, "MeshIndex.build")
        lo, hi = mp.mesh_bounds(verts)
        lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
        F, dev = faces.shape[0], verts.device
        tri = _pack(verts, faces)
        side = float((hi_h - lo_h).max())
        cum_area = face_areas_cum(verts, faces)
        area = float(cum_area[-1])
        if cell is None:
            cell = max(CELL_FACTOR * (area / F) ** 0.5, side / 256.) if np.isfinite(area) else side / 256.
            if not cell > 0:
                cell = 1.
        cell = float(np.float32(cell))
        if not (cell > 0 and np.isfinite(cell)):
            raise ValueError(f"cell must be a positive float32, got {cell}")
        lo = lo.contiguous()
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
        key, perm = torch.sort(key, stable=True)
        cells = n[0] * n[1] * n[2]
        cell_start = torch.zeros((cells + 1,), dtype=torch.int64, device=dev)
        cell_start[1:] = torch.cumsum(torch.bincount(key, minlength=cells), 0)
        return cls(verts, faces, tri, cum_area, area, lo, cell, n, cell_start, pair_face[perm].contiguous())

    def face_normals(self):
        """[F,3] float32 unit normals (b - a) x (c - a) evaluated in double; zero for a face without area."""
        if self._normals is None:
            p = self.verts.double()[self.faces]
            nrm = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
            length = nrm.norm(dim=1, keepdim=True)
            self._normals = torch.where(length > 0, nrm / length.clamp_min(1e-300), torch.zeros_like(nrm)).float()
        return self._normals


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
    dist = torch.empty((P,), dtype=torch.float32, device=dev)
    face = torch.empty((P,), dtype=torch.int64, device=dev)
    closest = torch.empty((P, 3), dtype=torch.float32, device=dev)
    if P == 0:
        return dist, face, closest
    F = index.faces.shape[0]
    if method == "brute":
        _lib.launch("sr_surfdist_brute", points, points, P, index.tri, F, dist, face, closest)
        return dist, face, closest
    n = index.n
    order = None
    if presort:
        order = torch.sort(mp.cell_keys(points, index.lo, index.cell, n), stable=True)[1]
        points = points[order].contiguous()
    _lib.launch("sr_surfdist_query", points, points, P, index.tri, F, index.lo, index.cell, n[0], n[1], n[2], index.cell_start, index.cell_faces,
                index.pairs, dist, face, closest)
    if order is None:
        return dist, face, closest
    inv = torch.empty_like(order)
    inv[order] = torch.arange(P, dtype=torch.int64, device=dev)
    return dist[inv], face[inv], closest[inv]


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
    face's unit normal.  ValueError for a mesh without area.  One device -> host read (A)."""
    verts, faces = _mesh(verts, faces, "sample_surface")
    n = int(n)
    if n < 0:
        raise ValueError(f"n >= 0 expected, got {n}")
    if cum_area is None:
        cum_area = face_areas_cum(verts, faces)
    _lib.require_gpu(cum_area)
    if cum_area.dtype != torch.float64 or cum_area.shape != (faces.shape[0],):
        raise ValueError("cum_area [F] float64 expected")
    area = float(cum_area[-1])
    if not (area > 0 and np.isfinite(area)):
        raise ValueError(f"sample_surface: the mesh has total area {area}")
    return _sample(_pack(verts, faces), cum_area.contiguous(), n, seed)
