"""Template preparation for the texture stage, on the GPU: what the reference's README leaves to the user ("you need to simplify and
parameterize the template mesh tmp.ply yourself, then save the result mesh as .../template/uvmap.obj").

    simplify_mesh / simplify_to   vertex clustering on a uniform grid (87k-196k marching-cubes vertices -> a face budget); the new
                                  vertices at the cell means (default) or, placement="quadric", at the quadric optima of their cells
    simplify_collapse             edge-collapse decimation to a face budget in rounds of independent collapses: keeps a manifold a manifold
    simplify_quality              surface distances and volume ratio between a simplified mesh and its source
    unwrap_charts                 box projection: charts = connected faces of one dominant normal axis and sign, shelf-packed
    prepare_template              extract -> simplify -> unwrap -> template/uvmap.obj

The reference has no code for this step and pytorch3d / xatlas are not dependencies, so the semantics are this package's own (DESIGN.md
3.15: stated, unpinned) and are held to a float64 numpy restatement by the tests.  Known limits, also in DESIGN: the stretch of box
projection (UV area / surface area of a face is |n_axis| / |n|, between 1 / sqrt(3) and 1), seams at every change of the dominant axis,
and no repair of a chart that overlaps itself in projection -- that is counted (`overlap_texels`), not fixed.  The default placement
puts a vertex at its cell's mean, which lies inside the hull of the members: the body shrinks and creases are rounded off.
placement="quadric" moves it to the regularised minimiser of the cell's plane quadrics instead (Lindstrom's out-of-core
simplification), clamped to the cell's box: two clamped neighbours can meet on their shared wall.  Clustering decides by position alone:
it can weld two sheets of the surface that pass through one cell and leave non-manifold edges.  simplify_collapse does not -- every
collapse passes the link condition -- at the price of some tens of rounds instead of one pass; boundary and non-manifold edges are kept
as they are (their vertices are locked).  Boundary-edge quadrics for open meshes and attribute-aware quadrics are out of scope.
"""
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import mesh_prep_ops as mp

SimplifiedMesh = namedtuple("SimplifiedMesh", "verts faces vertex_map cell")
ChartAtlas = namedtuple("ChartAtlas", "vt ft chart labels bbox_min extent origin size scale rounds overlap_texels")
PreparedTemplate = namedtuple("PreparedTemplate", "mesh atlas obj_path source_faces")

BISECT_STEPS = 16
PLACEMENTS = ("mean", "quadric")
METHODS = ("cluster", "collapse")
PACK_STEPS = 24


def _grid(verts, cell):
    lo, hi = mp.mesh_bounds(verts)
    return lo, mp.grid_shape(lo.cpu().numpy(), hi.cpu().numpy(), cell)


def _clustered(verts, faces, lo, n, cell):
    """(vertex_map, the occupied cells' keys, remapped faces, keep) of one grid."""
    cells, vmap = mp.cluster(mp.cell_keys(verts, lo, cell, n))
    remapped, keep = mp.surviving_faces(faces, vmap, cells.shape[0])
    return vmap, cells, remapped, keep


def _reg(reg):
    """The checked reg as a float: ValueError for one that is not finite and positive."""
    try:
        reg = float(reg)
    except (TypeError, ValueError):
        raise ValueError(f"reg must be a finite positive number, got {reg!r}") from None
    if not (np.isfinite(reg) and reg > 0):
        raise ValueError(f"reg must be a finite positive number, got {reg}")
    return reg


def _placement(placement, reg):
    """The checked (placement, reg): ValueError for a placement that is not one of PLACEMENTS or a reg that _reg refuses."""
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be one of {PLACEMENTS}, got {placement!r}")
    return placement, _reg(reg)


def simplify_mesh(verts, faces, cell, placement="mean", reg=1e-3, report=None):
    """Vertex clustering of verts [V,3] float32 / faces [F,3] int64 (GPU tensors) on a uniform grid of side `cell`.

    Faces with a negative index are dropped first.  With lo the per-axis float32 minimum, a vertex lies in cell ijk = floor((v - lo) /
    cell) (float32 subtraction and IEEE division), key (k n_y + j) n_x + i, n = max ijk + 1.  The new vertices are the occupied cells
    in ascending key, each at the mean of its members (summed in ascending original index, in double, rounded once); vertex_map [V]
    gives old -> new.  Faces are remapped; a face with a repeated corner is dropped, and of the faces with the same unordered vertex set
    the one with the lowest original index stays.  Survivors keep their corner order and their relative order; new vertices no face
    references are kept.  ValueError for cell <= 0, non-finite vertices or a grid of 2^62 cells or more.  Two calls give identical
    bits.  -> SimplifiedMesh(verts [Vn,3], faces [Fn,3], vertex_map [V], cell).

    placement="quadric" changes the positions only -- the clustering, vertex_map, the faces and their order are those of "mean".  Every
    original face with area feeds its plane quadric (w n n^T, w d n; w its area) once to each distinct cell among its corners; a cell's
    vertex goes to x = m + (A + lambda I)^-1 (b - A m), m its mean and lambda = reg trace(A) / 3, clamped per component to the cell's
    box and rounded once (mesh_prep_ops.cell_quadric_optima).  A cell no face with area touches stays at its mean.
    `reg` = 1e-3 is a documented default, not a tuned one: it keeps the directions the planes leave free (a flat patch, a straight
    crease) at the mean, with a condition number of at most 3 / reg.  ValueError, before any GPU work, for another placement or a
    reg that is not finite and positive.

    `report`, a dict, receives placement, cells, clamped, no_planes (cells at the clamp / without a usable quadric; 0 for "mean"),
    max_shift (the largest |x - m| in units of the cell), and flipped / zero_area: the surviving faces whose normal at the new positions
    points against the normal of the original face they come from, or has vanished (mesh_prep_ops.face_flips, either placement).
    Filling it costs one launch and three small device -> host copies."""
    placement, reg = _placement(placement, reg)
    _lib.require_gpu(verts, faces)
    verts = _lib.f32c(verts)
    faces = mp.clean_faces(faces)
    cell = float(np.float32(cell))
    if not cell > 0:
        raise ValueError(f"cell must be positive, got {cell}")
    lo, n = _grid(verts, cell)
    vmap, cells, remapped, keep = _clustered(verts, faces, lo, n, cell)
    C = cells.shape[0]
    flags = shift = None
    if placement == "quadric":
        new_verts, flags, shift = mp.cell_quadric_optima(verts, faces, vmap, cells, lo, cell, n, reg)
    else:
        new_verts = mp.cell_means(verts, vmap, C)
    mesh = SimplifiedMesh(new_verts, remapped[keep].contiguous(), vmap, cell)
    if report is not None:
        _fill_report(report, placement, verts, faces, mesh, keep.nonzero().view(-1), flags, shift)
    return mesh


def _fill_report(report, placement, verts, faces, mesh, source, flags, shift):
    clamped = no_planes = 0
    max_shift = 0.
    if flags is not None:
        clamped, no_planes = torch.stack([((flags & mp.QUADRIC_CLAMPED) != 0).sum(), ((flags & mp.QUADRIC_NO_PLANES) != 0).sum()]).tolist()
        max_shift = float(shift.max())
    flipped, zero_area = mp.face_flips(verts, faces, mesh.verts, mesh.faces, source)
    report.update(placement=placement, cells=int(mesh.verts.shape[0]), clamped=clamped, no_planes=no_planes, flipped=flipped, zero_area=zero_area,
                  max_shift=max_shift)


def simplify_to(verts, faces, target_faces, probes=None, placement="mean", reg=1e-3, report=None):
    """simplify_mesh at the smallest probed cell that leaves at most `target_faces` faces.  A mesh that is within the budget already
    comes back cleaned (no negative rows) with the identity map and cell 0.  Otherwise the cell is bisected geometrically in [d / 1024,
    d / 2], d the longest side of the box, in 16 steps of keys -> count of surviving faces (no positions); ValueError if even d / 2
    leaves more.  `probes`, a list, receives every (cell, face count) tried, in order.  `placement`, `reg` and `report` are
    simplify_mesh's; the bisection never needs positions, so the cell, the probes and the faces are the same for both placements."""
    placement, reg = _placement(placement, reg)
    _lib.require_gpu(verts, faces)
    verts = _lib.f32c(verts)
    faces = mp.clean_faces(faces)
    target = int(target_faces)
    if faces.shape[0] <= target:
        mp.mesh_bounds(verts)                                            # (the refusal of non-finite vertices holds here too)
        if report is not None:                                           # (nothing moved: every vertex is its own cell)
            report.update(placement=placement, cells=int(verts.shape[0]), clamped=0, no_planes=0, flipped=0, zero_area=0, max_shift=0.)
        return SimplifiedMesh(verts, faces, torch.arange(verts.shape[0], dtype=torch.int64, device=verts.device), 0.)
    lo, hi = mp.mesh_bounds(verts)
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    d = float((hi_h - lo_h).max())
    if not (np.isfinite(d) and d > 0):
        raise ValueError(f"simplify_to: the box of the vertices has longest side {d}")

    def count(cell):
        cell = float(np.float32(cell))
        _, _, _, keep = _clustered(verts, faces, lo, mp.grid_shape(lo_h, hi_h, cell), cell)
        k = int(keep.sum())
        if probes is not None:
            probes.append((cell, k))
        return cell, k
    a, b = d / 1024., d / 2.
    best, k = count(b)
    if k > target:
        raise ValueError(f"simplify_to: {k} faces are left at the coarsest cell {best}, more than the target {target}")
    for _ in range(BISECT_STEPS):
        cell, k = count((a * b) ** 0.5)
        if k <= target:
            b = best = cell
        else:
            a = cell
    return simplify_mesh(verts, faces, best, placement, reg, report)


def simplify_collapse(verts, faces, target_faces, reg=1e-3, flip_cos=0.2, max_rounds=1024, report=None):
    """Edge-collapse decimation of verts [V,3] float32 / faces [F,3] int64 (GPU tensors) to `target_faces` faces, in rounds of
    independent collapses (mesh_prep_ops.collapse_round / collapse_apply).  Unlike the clustering it changes the
    connectivity one valid collapse at a time: a closed oriented manifold stays one, and boundary or non-manifold edges keep their
    vertices untouched (they are locked).

    Rows with a negative index or a repeated corner are dropped first; a mesh within the budget then comes back as simplify_to returns
    it (identity map, cell 0).  Every vertex gets the summed plane quadrics of its faces once (float64).  A round lists the edges,
    gives each one that may collapse (two faces, unlocked ends, link condition, valences, no face turned by more than acos(flip_cos))
    the position x = m + (A + lambda I)^-1 (b - A m) of Q_a + Q_b about its midpoint, lambda = reg trace(A) / 3, rounded to float32, and
    the key (float32 bits of the cost at x) << 32 | hash(edge index); the edges whose key is the least among all edges at their ends and
    at their ends' neighbours collapse -- they touch disjoint faces -- the cheapest first when fewer are needed: verts[a] = x, Q_a +=
    Q_b, b -> a.  A full run ends at F - 2 ceil((F - target) / 2) faces.  It stops early ("stalled") when a round selects nothing or
    after `max_rounds`.  Unreferenced vertices are dropped at the end, the survivors keep their ascending original order, and
    vertex_map [V] sends every original vertex to its survivor (-1 for a vertex no face ever used).  The host reads one small record
    per round.  ValueError for non-finite vertices, an index outside [0, V), reg not finite and positive or flip_cos outside [-1, 1).
    Two calls give identical bits.  -> SimplifiedMesh(verts [Vn,3], faces [Fn,3], vertex_map [V], cell = 0.).

    `report`, a dict, receives method ("collapse"), rounds, collapses, stalled, locked_vertices (of the first round), candidates_first
    / candidates_last (of the first and the last round), vertices, faces, and flipped / zero_area: the surviving faces whose normal
    points against the normal of the triangle their three survivors made at their original positions, or has vanished
    (mesh_prep_ops.face_flips with every face as its own source).  `flipped` measures how far survivors have travelled, not folds: a
    vertex that has moved past a neighbour's old place counts, on a flat grid too; every collapse has passed the flip test."""
    reg = _reg(reg)
    flip_cos = float(flip_cos)
    if not -1. <= flip_cos < 1.:
        raise ValueError(f"flip_cos must lie in [-1, 1), got {flip_cos}")
    _lib.require_gpu(verts, faces)
    verts = _lib.f32c(verts)
    mp.mesh_bounds(verts)                                                # (refuses non-finite vertices, as simplify_mesh does)
    V, dev = verts.shape[0], verts.device
    faces = mp._indexed(mp.proper_faces(faces), V, "simplify_collapse")
    target, F = int(target_faces), faces.shape[0]
    parent = torch.arange(V, dtype=torch.int64, device=dev)
    stats = dict(method="collapse", rounds=0, collapses=0, stalled=False, locked_vertices=0, candidates_first=0, candidates_last=0)
    if F <= target:
        if report is not None:
            report.update(stats, vertices=V, faces=F, flipped=0, zero_area=0)
        return SimplifiedMesh(verts, faces, parent, 0.)
    moved = verts.clone()
    quadrics = mp.vertex_quadrics(verts, faces)
    while F > target:
        if stats["rounds"] >= int(max_rounds):
            stats["stalled"] = True
            break
        edges, keys, positions, selected, record, locked = mp._round(moved, faces, quadrics, reg, flip_cos)
        n_selected, n_candidates = record.tolist()                       # the round's one device -> host copy
        if stats["rounds"] == 0:
            stats.update(locked_vertices=int(locked.sum()), candidates_first=n_candidates)
        stats["rounds"] += 1
        stats["candidates_last"] = n_candidates
        if n_selected == 0:
            stats["stalled"] = True
            break
        need = (F - target + 1) // 2
        if n_selected > need:                                            # the `need` cheapest of the selected (the keys are unique)
            ranked = torch.where(selected.bool(), keys, torch.full_like(keys, mp.INT64_MAX))
            selected = ranked <= torch.kthvalue(ranked, need)[0]
            n_selected = need
        faces = mp.collapse_apply(moved, faces, quadrics, parent, edges, positions, selected)
        stats["collapses"] += n_selected
        if faces.shape[0] != F - 2 * n_selected:
            raise RuntimeError(f"simplify_collapse: {n_selected} collapses removed {F - faces.shape[0]} faces")
        F = faces.shape[0]
    root = mp.collapse_roots(parent)
    used = torch.zeros((V,), dtype=torch.bool, device=dev)
    used[faces.view(-1)] = True
    new = torch.cumsum(used, 0) - 1
    vertex_map = torch.where(used[root], new[root], torch.full_like(root, -1))
    mesh = SimplifiedMesh(moved[used].contiguous(), new[faces].contiguous(), vertex_map, 0.)
    if report is not None:
        flipped, zero_area = mp.face_flips(verts, faces, moved, faces, torch.arange(F, dtype=torch.int64, device=dev))
        report.update(stats, vertices=int(mesh.verts.shape[0]), faces=F, flipped=flipped, zero_area=zero_area)
    return mesh


def signed_volume(verts, faces):
    """The signed volume sum p0 . (p1 x p2) / 6 of a triangle mesh (positive for outward normals), in double: a 0-d GPU tensor."""
    p = verts.double()[faces]
    return (p[:, 0] * torch.linalg.cross(p[:, 1], p[:, 2])).sum() / 6.


def simplify_quality(mesh, verts, faces, samples=200_000, seed=0):
    """How far a SimplifiedMesh is from its source verts / faces, as a dict of Python floats: `simplified_to_source` and
    `source_to_simplified` with mean / rms / max of the exact distances of `samples` area-weighted surface samples of one mesh to the
    other (evaluate.surface_metrics, no alignment), `chamfer`, and `volume_source`, `volume_simplified`, `volume_ratio` = simplified /
    source of the signed volumes (below 1: the simplified body has shrunk)."""
    from .evaluate import surface_metrics
    _lib.require_gpu(mesh.verts, mesh.faces, verts, faces)
    verts = _lib.f32c(verts)
    faces = mp.clean_faces(faces)
    m = surface_metrics((mesh.verts, mesh.faces), (verts, faces), samples=samples, seed=seed)
    vs, vm = torch.stack([signed_volume(verts, faces), signed_volume(mesh.verts, mesh.faces)]).tolist()
    return {"simplified_to_source": m["pred_to_gt"], "source_to_simplified": m["gt_to_pred"], "chamfer": m["chamfer"], "volume_source": vs,
            "volume_simplified": vm, "volume_ratio": vm / vs if vs != 0 else float("nan")}


def _shelves(size, R):
    """Shelf packing of the rectangles size [C,2] (w, h) into R x R: order (height desc, width desc, label asc), left to right, a new
    shelf when x + w > R, a shelf as high as its first rectangle.  -> origin [C,2] int64, or None when it does not fit."""
    w, h = size[:, 0], size[:, 1]
    if w.max() > R:
        return None
    order = np.lexsort((np.arange(len(w)), -w, -h))
    origin = np.zeros((len(w), 2), np.int64)
    x = y = shelf = 0
    for i, wi, hi in zip(order.tolist(), w[order].tolist(), h[order].tolist()):
        if x + wi > R:
            x, y = 0, y + shelf
            shelf = 0
        if shelf == 0:
            shelf = hi
            if y + shelf > R:
                return None
        origin[i] = (x, y)
        x += wi
    return origin


def pack_charts(extent, R, padding):
    """Host-side packing of charts with projected extents extent [C,2] (numpy) into an R x R atlas.  A chart's rectangle is size =
    ceil(extent scale) + 2 padding + 1 texels, which leaves `padding` texels and half a texel around its triangles, so different
    charts stay at least 2 padding texels apart.  `scale` (texels per unit length) is the largest value for which the shelf packing
    (see _shelves) fits, found by 24 bisection steps on [0, R / max extent]; all-zero extents give scale 0.  ValueError if the charts
    do not fit even at scale 0.  Deterministic.  -> (scale float, origin [C,2] int64, size [C,2] int64)."""
    extent = np.asarray(extent, np.float64).reshape(-1, 2)
    R, padding = int(R), int(padding)
    if len(extent) == 0:
        return 0., np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64)
    if not np.isfinite(extent).all() or (extent < 0).any() or padding < 0 or R <= 0:
        raise ValueError("pack_charts: finite non-negative extents, padding >= 0 and R > 0 expected")

    def sizes(s):
        return np.ceil(extent * s).astype(np.int64) + 2 * padding + 1
    lo, origin = 0., _shelves(sizes(0.), R)
    if origin is None:
        raise ValueError(f"pack_charts: {len(extent)} charts do not fit a {R} x {R} atlas at padding {padding}, even as points")
    emax = float(extent.max())
    if emax > 0:
        hi = R / emax
        for _ in range(PACK_STEPS):
            mid = 0.5 * (lo + hi)
            o = _shelves(sizes(mid), R)
            if o is None:
                hi = mid
            else:
                lo, origin = mid, o
    return lo, origin, sizes(lo)


def unwrap_charts(verts, faces, resolution=1680, padding=2):
    """Box-projection UV atlas of verts [V,3] float32 / faces [F,3] int64 (GPU tensors, every index valid).

    A face's class is the axis of the largest |component| of its float64 normal (lowest axis on a tie, +x for a zero normal) and that
    component's sign; charts are the connected components of faces of one class that share an edge (label: lowest face index).  A chart
    is projected along its axis -- (u, v) = (x_{k+1}, x_{k+2}), swapped for a negative sign, so UV areas are positive --, all charts are
    scaled by one factor and shelf-packed (pack_charts; one device -> host copy of the boxes), and vt[3 f + c] = (origin + padding + 0.5
    + (p - bbox_min) scale) / R.  Faces do not share UV vertices: ft = arange(3 F).  A chart that overlaps itself in projection (a spiral
    ramp) is not split; `overlap_texels` (uv_overlap_count) reports the texels it costs.
    -> ChartAtlas(vt [3F,2] f32, ft [F,3] i64, chart [F] i64 (index into labels), labels [C] i64, bbox_min [C,2] f32, extent [C,2] f32,
    origin [C,2] i64, size [C,2] i64, scale, rounds, overlap_texels).  Two calls give identical bits."""
    _lib.require_gpu(verts, faces)
    verts = _lib.f32c(verts)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] == 0:
        raise ValueError(f"verts [V,3] expected, got {tuple(verts.shape)}")
    cls = mp.face_classes(verts, faces)                                  # (checks the indices)
    faces = _lib.i64c(faces)
    F, dev = faces.shape[0], verts.device
    if F == 0:
        raise ValueError("unwrap_charts: no faces")
    R, padding = int(resolution), int(padding)
    label, rounds = mp.chart_components(faces, verts.shape[0], cls)
    labels, chart = torch.unique(label.long(), sorted=True, return_inverse=True)
    chart = chart.contiguous()
    C = labels.shape[0]
    bbox_min, extent = mp.chart_boxes(verts, faces, cls, chart, C)
    scale, origin, size = pack_charts(extent.cpu().numpy(), R, padding)
    origin_d = torch.from_numpy(origin).to(dev)
    vt = mp.chart_uv(verts, faces, cls, chart, bbox_min, origin_d, scale, padding, R)
    ft = torch.arange(3 * F, dtype=torch.int64, device=dev).view(F, 3)
    return ChartAtlas(vt, ft, chart, labels, bbox_min, extent, origin_d, torch.from_numpy(size).to(dev), float(scale), rounds,
                      mp.uv_overlap_count(vt, ft, R))


def prepare_template(net, out_root, ratio=None, target_faces=20000, resolution=1680, padding=2, TmpVs=None, Tmpfs=None, placement="mean", reg=1e-3,
                     report=None, method="cluster"):
    """Extracts the template of `net` with discretizeSDF(ratio, None, 0.) as infer does (all ratios 1 unless given; or takes TmpVs /
    Tmpfs), simplifies it to `target_faces`, unwraps it and writes out_root/template/uvmap.obj, the file export_texture reads.
    -> PreparedTemplate(mesh SimplifiedMesh, atlas ChartAtlas, obj_path, source_faces: the faces of the extracted template).

    20000 faces is a default, not a measured optimum: at 1680^2 texels with about half of the atlas covered it leaves some 70 texels
    per face.  `method` is "cluster" (simplify_to, which takes `placement`, `reg` and `report`) or "collapse" (simplify_collapse, which
    takes `reg` and `report`; ValueError with placement="quadric", which places cluster representatives)."""
    from .mesh_io import write_obj_uv
    from .posed import FULL_RATIO
    placement, reg = _placement(placement, reg)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if method == "collapse" and placement != "mean":
        raise ValueError(f"placement={placement!r} belongs to method='cluster'; method='collapse' places every vertex by its own quadric")
    if TmpVs is None or Tmpfs is None:
        TmpVs, Tmpfs = net.discretizeSDF(ratio or FULL_RATIO, None, 0.)
    if method == "collapse":
        mesh = simplify_collapse(TmpVs.detach(), Tmpfs, target_faces, reg=reg, report=report)
    else:
        mesh = simplify_to(TmpVs.detach(), Tmpfs, target_faces, placement=placement, reg=reg, report=report)
    atlas = unwrap_charts(mesh.verts, mesh.faces, resolution, padding)
    folder = os.path.join(out_root, "template")
    os.makedirs(folder, exist_ok=True)
    obj = os.path.join(folder, "uvmap.obj")
    write_obj_uv(obj, mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), atlas.vt.cpu().numpy(), atlas.ft.cpu().numpy())
    return PreparedTemplate(mesh, atlas, obj, int((Tmpfs >= 0).all(1).sum()))
