"""Operators of the template preparation (csrc/mesh_prep.hip, csrc/mesh_collapse.hip): GPU tensors only, no autograd.  `mesh_prep.py` is the public interface.
Sorting, unique and compaction are torch's; everything per element is a HIP kernel.  Two calls give identical bits."""
import numpy as np
import torch

from . import _lib
from .ops import _faces

MAX_ROUNDS = 4096          # passes of the component search before it is declared stuck (a 40 000-face strip needs about 20)
QUADRIC_CLAMPED, QUADRIC_NO_PLANES = _lib.SR_QUADRIC_CLAMPED, _lib.SR_QUADRIC_NO_PLANES          # bits of cell_quadric_optima's flags


def _verts2(verts):
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts [V,3] expected, got {tuple(verts.shape)}")
    if verts.shape[0] == 0:
        raise ValueError("verts [V,3] expected, got no vertices")
    return _lib.f32c(verts)


def _indexed(faces, V, what):
    """faces [F,3] int64 with every index in [0, V) (ValueError otherwise: the kernels would skip such a face silently)."""
    faces = _faces(faces)
    if faces.shape[0] and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise ValueError(f"{what}: face indices outside [0, {V})")
    return faces


def clean_faces(faces):
    """The rows of faces [F,3] without a negative index (marching cubes pads its list with -1 rows), in order."""
    _lib.require_gpu(faces)
    faces = _faces(faces)
    return faces[(faces >= 0).all(1)].contiguous()


def mesh_bounds(verts):
    """(lo [3], hi [3]) float32 on the device: the per-axis extremes of verts [V,3] (sr_meshprep_bounds).  ValueError for a
    non-finite coordinate.  One device -> host copy (the flag)."""
    _lib.require_gpu(verts)
    verts = _verts2(verts)
    box = torch.empty((8,), dtype=torch.int32, device=verts.device)
    _lib.launch("sr_meshprep_bounds", verts, verts, verts.shape[0], box)
    if int(box[6]):
        raise ValueError("non-finite vertex coordinates")
    b = box[:6].view(torch.float32)
    return b[:3], b[3:]


def grid_shape(lo, hi, cell):
    """(n_x, n_y, n_z) = floor((hi - lo) / cell) + 1 in float32 arithmetic (what the kernel evaluates for the extreme vertices), as
    Python ints.  ValueError for cell <= 0 or a grid of 2^62 cells or more."""
    cell = np.float32(cell)
    if not cell > 0 or not np.isfinite(cell):
        raise ValueError(f"cell must be a positive float32, got {cell}")
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.floor((np.asarray(hi, np.float32) - np.asarray(lo, np.float32)) / cell)
    if not np.isfinite(q).all():
        raise ValueError(f"cell {cell}: the grid has 2^62 cells or more")
    n = [int(x) + 1 for x in q.tolist()]
    if n[0] * n[1] * n[2] >= 1 << 62:
        raise ValueError(f"cell {cell}: the grid {n[0]} x {n[1]} x {n[2]} has 2^62 cells or more")
    return tuple(n)


def cell_keys(verts, lo, cell, n):
    """key [V] int64 = (k n_y + j) n_x + i of every vertex's grid cell (sr_meshprep_cell_keys); lo [3] on the device."""
    _lib.require_gpu(verts, lo)
    verts = _verts2(verts)
    key = torch.empty((verts.shape[0],), dtype=torch.int64, device=verts.device)
    _lib.launch("sr_meshprep_cell_keys", verts, verts, verts.shape[0], _lib.f32c(lo), float(np.float32(cell)), n[0], n[1], n[2], key)
    return key


def cluster(key):
    """(cells [C] ascending, vertex_map [V]) of the keys: torch.unique."""
    cells, vmap = torch.unique(key, sorted=True, return_inverse=True)
    return cells, vmap.contiguous()


def _lists(key, C):
    """(order, offsets [C + 1]): the positions of `key` grouped by value in [0, C), each group in ascending position (a stable sort);
    positions whose key is C or more come after offsets[C]."""
    order = torch.sort(key, stable=True)[1].contiguous()
    offsets = torch.zeros((C + 1,), dtype=torch.int64, device=key.device)
    offsets[1:] = torch.cumsum(torch.bincount(key, minlength=C)[:C], 0)
    return order, offsets


def cell_means(verts, vertex_map, C):
    """[C,3] float32: the mean of every cell's members, summed in ascending original index in double (sr_meshprep_cell_mean)."""
    _lib.require_gpu(verts, vertex_map)
    verts = _verts2(verts)
    order, offsets = _lists(_lib.i64c(vertex_map), C)
    out = torch.empty((C, 3), dtype=torch.float32, device=verts.device)
    _lib.launch("sr_meshprep_cell_mean", verts, verts, verts.shape[0], order, offsets, C, out)
    return out


def cell_quadric_optima(verts, faces, vertex_map, cells, lo, cell, n, reg=1e-3):
    """(positions [C,3] float32, flags [C] int32, shift [C] float32) of the cells `cells` [C] (ascending keys of the grid lo / cell / n
    that vertex_map [V] indexes): every cell's representative at the minimiser of the summed plane quadrics of the original faces that
    touch the cell plus reg trace(A) / 3 |x - mean|^2, clamped to the cell's box (sr_meshprep_cell_faces, a stable sort,
    sr_meshprep_cell_quadric).  flags: QUADRIC_CLAMPED, QUADRIC_NO_PLANES (such a cell sits at its mean); shift = |x - mean| / cell.
    Rows of `faces` with a negative index are skipped.  No device -> host copy."""
    _lib.require_gpu(verts, faces, vertex_map, cells, lo)
    verts = _verts2(verts); faces = _faces(faces); vmap = _lib.i64c(vertex_map); cells = _lib.i64c(cells)
    C, dev = cells.shape[0], verts.device
    if faces.shape[0] == 0:
        faces = torch.full((1, 3), -1, dtype=torch.int64, device=dev)            # (no face: every cell keeps its mean)
    F = faces.shape[0]
    slot = torch.empty((3 * F,), dtype=torch.int64, device=dev)
    _lib.launch("sr_meshprep_cell_faces", verts, faces, F, vmap, vmap.shape[0], C, slot)
    face_slots, face_offsets = _lists(slot, C)
    order, offsets = _lists(vmap, C)
    out = torch.empty((C, 3), dtype=torch.float32, device=dev)
    flags = torch.empty((C,), dtype=torch.int32, device=dev); shift = torch.empty((C,), dtype=torch.float32, device=dev)
    _lib.launch("sr_meshprep_cell_quadric", verts, verts, verts.shape[0], faces, F, face_slots, face_offsets, order, offsets, cells, C, _lib.f32c(lo),
                float(np.float32(cell)), n[0], n[1], float(reg), out, flags, shift)
    return out, flags, shift


def face_flips(verts, faces, new_verts, new_faces, source):
    """(flipped, zero_area) as Python ints: of the faces new_faces [Fn,3] at new_verts, how many have a normal whose dot product with
    the normal of faces[source[g]] at verts is negative, and how many have no area at all (sr_meshprep_face_flips; the normals are
    unnormalised cross products in double).  One device -> host copy."""
    _lib.require_gpu(verts, faces, new_verts, new_faces, source)
    verts = _verts2(verts); new_verts = _verts2(new_verts)
    faces = _faces(faces); new_faces = _faces(new_faces); source = _lib.i64c(source)
    Fn = new_faces.shape[0]
    if source.shape != (Fn,):
        raise ValueError(f"source [{Fn}] expected, got {tuple(source.shape)}")
    if Fn == 0 or faces.shape[0] == 0:
        return 0, 0
    counts = torch.empty((2,), dtype=torch.int64, device=verts.device)
    _lib.launch("sr_meshprep_face_flips", verts, verts, verts.shape[0], faces, faces.shape[0], new_verts, new_verts.shape[0], new_faces, source, Fn, counts)
    flipped, flat = counts.tolist()
    return flipped, flat


def surviving_faces(faces, vertex_map, Vn):
    """(remapped [F,3], keep [F] bool): vertex_map[faces], and which faces survive -- no repeated corner, and the lowest index among
    the faces with the same unordered vertex set (sr_meshprep_face_keys, two stable sorts, sr_meshprep_face_first)."""
    _lib.require_gpu(faces, vertex_map)
    faces = _faces(faces); vmap = _lib.i64c(vertex_map)
    F, dev = faces.shape[0], faces.device
    out = torch.empty((F, 3), dtype=torch.int64, device=dev)
    if F == 0:
        return out, torch.zeros((0,), dtype=torch.bool, device=dev)
    key_hi = torch.empty((F,), dtype=torch.int64, device=dev); key_lo = torch.empty_like(key_hi)
    _lib.launch("sr_meshprep_face_keys", faces, faces, F, vmap, vmap.shape[0], int(Vn), out, key_hi, key_lo)
    lo_sorted, p1 = torch.sort(key_lo, stable=True)
    hi_sorted, p2 = torch.sort(key_hi[p1], stable=True)
    keep = torch.empty((F,), dtype=torch.uint8, device=dev)
    _lib.launch("sr_meshprep_face_first", faces, hi_sorted.contiguous(), lo_sorted[p2].contiguous(), p1[p2].contiguous(), F, keep)
    return out, keep.bool()


def face_classes(verts, faces):
    """cls [F] int32 = 2 axis + (negative ? 1 : 0) of every face's float64 normal (sr_chart_classify)."""
    _lib.require_gpu(verts, faces)
    verts = _verts2(verts); faces = _indexed(faces, verts.shape[0], "face_classes")
    cls = torch.empty((faces.shape[0],), dtype=torch.int32, device=verts.device)
    if faces.shape[0]:
        _lib.launch("sr_chart_classify", verts, verts, verts.shape[0], faces, faces.shape[0], cls)
    return cls


def _jump_to_fixed_point(entry, P, Q, changed, passes, limit, stuck):
    """Pointer doubling of the forest P with the double-buffered kernel `entry` (sr_chart_jump, sr_collapse_map_jump) until a pass changes
    nothing: one launch and one flag read per pass.  -> (the fixed point, the other buffer, `passes` plus the passes made here).
    RuntimeError(stuck) when the count has gone past `limit` and the last pass still changed something."""
    while True:
        _lib.launch(entry, P, P, P.shape[0], Q, changed)
        passes += 1
        P, Q = Q, P
        if not int(changed):
            return P, Q, passes
        if passes > limit:
            raise RuntimeError(stuck.format(passes=passes))


def chart_components(faces, V, cls):
    """(label [F] int32, rounds): label = the lowest face index of the connected component of faces of equal class that share an edge
    (all faces on a non-manifold edge are connected).  Min-label hooking of roots, then pointer doubling until every tree is a star,
    repeated until no edge joins two trees; `rounds` counts every pass over the faces or edges, and each pass costs one flag read."""
    _lib.require_gpu(faces, cls)
    faces = _faces(faces)
    F, dev = faces.shape[0], faces.device
    key = torch.empty((3 * F,), dtype=torch.int64, device=dev)
    _lib.launch("sr_chart_edge_keys", faces, faces, F, int(V), cls, key)
    skey, perm = torch.sort(key)
    P = torch.arange(F, dtype=torch.int32, device=dev); Q = torch.empty_like(P)
    changed = torch.zeros((1,), dtype=torch.int32, device=dev)
    rounds = 0
    while True:
        _lib.launch("sr_chart_hook", faces, skey, perm, 3 * F, P, Q, F, changed)
        rounds += 1
        if not int(changed):
            return P, rounds
        P, Q, rounds = _jump_to_fixed_point("sr_chart_jump", Q, P, changed, rounds, MAX_ROUNDS, "chart_components: no fixed point after {passes} passes")


def chart_boxes(verts, faces, cls, chart, C):
    """(bbox_min [C,2], extent [C,2]) float32 of the charts' projected corners (sr_chart_bbox)."""
    _lib.require_gpu(verts, faces, cls, chart)
    verts = _verts2(verts); faces = _faces(faces)
    dev = verts.device
    box = torch.empty((C, 4), dtype=torch.int32, device=dev)
    bbox_min = torch.empty((C, 2), dtype=torch.float32, device=dev); extent = torch.empty_like(bbox_min)
    _lib.launch("sr_chart_bbox", verts, verts, verts.shape[0], faces, faces.shape[0], cls, _lib.i64c(chart), C, box, bbox_min, extent)
    return bbox_min, extent


def chart_uv(verts, faces, cls, chart, bbox_min, origin, scale, padding, resolution):
    """vt [3F,2] float32 (sr_chart_uv): every corner's place in its chart's rectangle of the atlas."""
    _lib.require_gpu(verts, faces, cls, chart, bbox_min, origin)
    verts = _verts2(verts); faces = _faces(faces)
    vt = torch.empty((3 * faces.shape[0], 2), dtype=torch.float32, device=verts.device)
    _lib.launch("sr_chart_uv", verts, verts, verts.shape[0], faces, faces.shape[0], cls, _lib.i64c(chart), bbox_min.shape[0], _lib.f32c(bbox_min),
                _lib.i64c(origin), float(scale), int(padding), int(resolution), vt)
    return vt


def uv_overlap_count(vt, ft, resolution, eps=1e-6):
    """The number of texel centres (uv_texel_map's convention: u = (c + 0.5) / R, v = 1 - (r + 0.5) / R) that lie strictly inside two
    or more UV triangles, i.e. every barycentric > eps (sr_uv_overlap_count: an int32 count image and integer atomics).  0 for an atlas
    whose triangles do not overlap; a patch that folds over itself in projection, as a spiral ramp does, gives a positive count."""
    _lib.require_gpu(vt, ft)
    if vt.dim() != 2 or vt.shape[1] != 2:
        raise ValueError(f"vt [Vt,2] expected, got {tuple(vt.shape)}")
    vt = _lib.f32c(vt); ft = _faces(ft)
    R = int(resolution)
    if ft.shape[0] == 0 or vt.shape[0] == 0:
        return 0
    count = torch.empty((max(R, 0), max(R, 0)), dtype=torch.int32, device=vt.device)
    total = torch.empty((1,), dtype=torch.int64, device=vt.device)
    _lib.launch("sr_uv_overlap_count", vt, vt, ft, vt.shape[0], ft.shape[0], R, float(eps), count, total)
    return int(total)


# ------------------------------------------------------------------------------------------------ edge collapse (csrc/mesh_collapse.hip)
INT64_MAX = (1 << 63) - 1          # the key of an edge that is no candidate
QUADRIC_DOUBLES = 10               # xx xy xz yy yz zz of sum w n n^T, sum w d n, sum w d^2


def proper_faces(faces):
    """The rows of faces [F,3] without a negative index or a repeated corner, in order."""
    faces = clean_faces(faces)
    a, b, c = faces.unbind(1)
    return faces[(a != b) & (b != c) & (a != c)].contiguous()


def _collapse_mesh(verts, faces, what):
    """(verts, faces) checked for a round: float32 [V,3], int64 [F,3] with F > 0, every index in [0, V) and no repeated corner."""
    _lib.require_gpu(verts, faces)
    verts = _verts2(verts)
    faces = _indexed(faces, verts.shape[0], what)
    if faces.shape[0] == 0:
        raise ValueError(f"{what}: no faces")
    a, b, c = faces.unbind(1)
    if bool(((a == b) | (b == c) | (a == c)).any()):
        raise ValueError(f"{what}: a face with a repeated corner")
    return verts, faces


def _quadrics(quadrics, V):
    if quadrics.dtype != torch.float64 or tuple(quadrics.shape) != (V, QUADRIC_DOUBLES) or not quadrics.is_contiguous():
        raise ValueError(f"quadrics: a contiguous float64 [{V},{QUADRIC_DOUBLES}] expected, got {quadrics.dtype} {tuple(quadrics.shape)}")
    return quadrics


def vertex_quadrics(verts, faces):
    """Q [V,10] float64: per vertex the plane quadrics (w n n^T as xx xy xz yy yz zz, w d n, w d^2; n the unit normal, w the area, d = n . p0
    as cell_quadric_optima takes them) of its faces, summed in ascending face index (a stable sort, sr_collapse_vertex_quadrics)."""
    verts, faces = _collapse_mesh(verts, faces, "vertex_quadrics")
    V, F = verts.shape[0], faces.shape[0]
    slots, offsets = _lists(faces.view(-1), V)
    Q = torch.empty((V, QUADRIC_DOUBLES), dtype=torch.float64, device=verts.device)
    _lib.launch("sr_collapse_vertex_quadrics", verts, verts, V, faces, F, slots, offsets, Q)
    return Q


def _round(verts, faces, quadrics, reg, flip_cos):
    """Steps 1-4 of a round on checked arguments -> (edges, keys, positions, selected uint8, record [2] int64 on the device: selected,
    candidates; locked [V] int32).  No device -> host copy but the edge count (torch.unique_consecutive's)."""
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    hkey = torch.empty((3 * F,), dtype=torch.int64, device=dev)
    _lib.launch("sr_collapse_edge_keys", verts, faces, F, V, hkey)
    skey, perm = torch.sort(hkey, stable=True)
    ukey, counts = torch.unique_consecutive(skey, return_counts=True)
    E = ukey.shape[0]
    offsets = torch.zeros((E + 1,), dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    edges = torch.empty((E, 2), dtype=torch.int64, device=dev); opp = torch.empty_like(edges)
    count = torch.empty((E,), dtype=torch.int32, device=dev); locked = torch.empty((V,), dtype=torch.int32, device=dev)
    directed = torch.empty((2 * E,), dtype=torch.int64, device=dev)
    _lib.launch("sr_collapse_edge_heads", verts, ukey, offsets, E, perm, faces, F, V, edges, count, opp, locked, directed)
    nbr = torch.sort(directed)[0]
    noff = torch.searchsorted(nbr, torch.arange(V + 1, dtype=torch.int64, device=dev) * V).contiguous()
    slots, soff = _lists(faces.view(-1), V)
    pos = torch.empty((E, 3), dtype=torch.float32, device=dev)
    keys = torch.empty((E,), dtype=torch.int64, device=dev)
    _lib.launch("sr_collapse_candidates", verts, verts, V, faces, F, quadrics, slots, soff, nbr, noff, edges, count, opp, locked, E, float(reg),
                float(flip_cos), pos, keys)
    m1 = torch.empty((V,), dtype=torch.int64, device=dev); m2 = torch.empty_like(m1)
    _lib.launch("sr_collapse_min1", verts, edges, keys, E, V, m1)
    _lib.launch("sr_collapse_min2", verts, edges, E, V, m1, m2)
    selected = torch.empty((E,), dtype=torch.uint8, device=dev)
    record = torch.empty((2,), dtype=torch.int64, device=dev)
    _lib.launch("sr_collapse_select", verts, edges, keys, E, V, m2, selected, record)
    return edges, keys, pos, selected, record, locked


def collapse_round(verts, faces, quadrics, reg=1e-3, flip_cos=0.2):
    """Steps 1-4 of one round of the edge-collapse decimation on verts [V,3] float32 / faces [F,3] int64 / quadrics [V,10] float64 (GPU
    tensors), nothing applied -> (edges [E,2] int64: a < b in ascending a V + b, keys [E] int64: (float32 bits of the
    cost) << 32 | fmix32(e), or INT64_MAX for an edge that is no candidate, positions [E,3] float32: where a collapse of the edge would
    put its vertex, selected [E] bool: key == m2[a] == m2[b] -- no two selected edges have adjacent or common endpoints).  ValueError for
    an index outside [0, V), a repeated corner or no faces."""
    verts, faces = _collapse_mesh(verts, faces, "collapse_round")
    _lib.require_gpu(quadrics)
    edges, keys, pos, selected, _, _ = _round(verts, faces, _quadrics(quadrics, verts.shape[0]), reg, flip_cos)
    return edges, keys, pos, selected.bool()


def collapse_apply(verts, faces, quadrics, target, edges, positions, selected):
    """Applies the collapses of the edges `selected` [E] (bool or uint8; no two may share or have adjacent endpoints, as collapse_round
    selects them) IN PLACE to verts [V,3] float32, quadrics [V,10] float64 and target [V] int64: verts[a] = positions[e], quadrics[a] +=
    quadrics[b], target[b] = a.  -> the surviving faces: target[faces] (one level) without the rows with a repeated corner, in order."""
    _lib.require_gpu(verts, faces, quadrics, target, edges, positions, selected)
    V, E = verts.shape[0], edges.shape[0]
    if verts.dtype != torch.float32 or not verts.is_contiguous() or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("collapse_apply: a contiguous float32 verts [V,3] expected (it is updated in place)")
    if target.dtype != torch.int64 or tuple(target.shape) != (V,) or not target.is_contiguous():
        raise ValueError(f"collapse_apply: a contiguous int64 target [{V}] expected")
    if tuple(edges.shape) != (E, 2) or tuple(positions.shape) != (E, 3) or tuple(selected.shape) != (E,):
        raise ValueError("collapse_apply: edges [E,2], positions [E,3] and selected [E] expected")
    quadrics = _quadrics(quadrics, V)
    faces = _indexed(faces, V, "collapse_apply")
    F, dev = faces.shape[0], verts.device
    selected = selected.to(torch.uint8).contiguous()
    if E:
        _lib.launch("sr_collapse_apply_vertices", verts, _lib.i64c(edges), _lib.f32c(positions), selected, E, verts, V, quadrics, target)
    if F == 0:
        return faces
    out = torch.empty((F, 3), dtype=torch.int64, device=dev); keep = torch.empty((F,), dtype=torch.uint8, device=dev)
    _lib.launch("sr_collapse_apply_faces", verts, faces, F, target, V, out, keep)
    return out[keep.bool()].contiguous()


def collapse_roots(target):
    """root [V] int64 of the forest target [V] (target[v] = v for a root) by pointer doubling (sr_collapse_map_jump; one flag read per
    pass, at most 64 passes: a chain of V links needs log2 V)."""
    _lib.require_gpu(target)
    P = _lib.i64c(target).clone()
    changed = torch.zeros((1,), dtype=torch.int32, device=P.device)
    # (limit 63: a 64th pass that still changes something raises)
    return _jump_to_fixed_point("sr_collapse_map_jump", P, torch.empty_like(P), changed, 0, 63, "collapse_roots: target is not a forest")[0]
