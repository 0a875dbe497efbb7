"""Geometry evaluation on the GPU: point-to-mesh distance, Chamfer, point-to-surface (P2S), normal consistency and F-score between two
triangle meshes (csrc/surfdist.hip, surfdist_ops.py).

    python -m selfreconcode_amd.evaluate --gpu-ids 0 --pred A.ply --gt B.ply [--samples N] [--seed S] [--tau t ...] [--out FILE.json]
    python -m selfreconcode_amd.evaluate --gpu-ids 0 --rec-root R --gt-root G [--frames N] [--samples N] [--seed S] [--tau t ...]
    ... [--align {none,rigid,similarity}] [--align-samples N] [--align-iters K] [--align-max-dist d] [--align-shared]
    ... [--align-init {centroid,none,axes,search}] [--align-candidates N] [--align-top K]
    ... [--signed] [--beta b] [--error-range d] [--error-mesh FILE.ply | --error-meshes]

Mesh-pair mode prints the metrics of two files.  Folder mode compares every posed mesh `R/meshs/<fid>.npy` of an `infer` run (faces
from `R/tmp.ply`) with `G/<fid>.ply` or `G/<fid>.obj` and writes `R/geometry_errors.txt` and `R/geometry_errors.json`.  By default no
alignment and no scaling is applied: both meshes are taken in the coordinates they are given.  `--align rigid` / `--align similarity`
first takes the predicted mesh onto the ground truth by point-to-plane ICP (align.py; local: it starts from matched
centroids), per frame, or with `--align-shared` once on the first compared frame for all of them (a constant camera-frame offset).
`--align-init axes` / `--align-init search` put a rotation search in front of the ICP for a scan in another
orientation -- another up axis, facing the other way --: the 24 rotations of the cube, or those and `--align-candidates` more, of
which the `--align-top` best are refined; the frame's line is then followed by one that says what the search chose.
`--signed` adds on which side the surfaces lie of each other (the generalized winding number, winding_ops.py): the mean
signed distance and the share of samples inside, per direction, and both signed volumes.  `--error-mesh FILE.ply` (mesh-pair mode) /
`--error-meshes` (folder mode: `R/geometry_errors/<fid>.ply`) write the predicted mesh, aligned if an alignment was asked for, coloured
by each vertex's distance to the ground truth: white to red up to `--error-range` (default: the 95th percentile of |d| over the mesh,
which is printed), and with `--signed` white to blue for the vertices inside the ground truth.
Every mesh is prepared once, as a surfdist_ops.Surface that owns its grid, pyramid and normals: both modes make one per ground-truth
file, resolve the alignment once against its grid and pass the Alignment on, and the functions here take a Surface in place of a pair.
Out of scope: partial overlap, reflections, quads, rendering the error map to an image.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import align as al
from . import surfdist_ops as sd
from . import winding_ops as wn
from .mesh_io import read_mesh, read_ply, write_ply


def _directed(src, dst, samples, seed):
    """samples of Surface `src` against Surface `dst`: (dist [n], dot of the sample's and the closest face's normal [n], the samples
    [n,3])."""
    pts, _, nrm = src.sample(samples, seed)
    dist, face, _ = sd.closest_point(pts, dst.grid())
    return dist, (nrm * dst.face_normals()[face]).sum(1), pts


def _signed(dist, w):
    """-dist where w >= 1/2, else dist; a distance of 0 stays +0 and NaN stays NaN."""
    return torch.where((w >= 0.5) & (dist > 0), -dist, dist)


def signed_distance(points, mesh_index, winding_index, beta=wn.BETA):
    """(signed [P], winding [P]) float32 of points [P,3] against one mesh given as its MeshIndex and its WindingIndex: the exact
    distance (closest_point), negative where the winding number (winding_number with `beta`) is >= 1/2, that is inside; a distance of
    0 stays +0; a non-finite point gives NaN in both.  On an open mesh the sign is that of the surface closed smoothly over its
    holes."""
    dist = sd.closest_point(points, mesh_index)[0]
    w = wn.winding_number(points, winding_index, beta=beta)
    return _signed(dist, w), w


ALIGN_MODES = ("rigid", "similarity")


def _alignment(pred, gt, align, align_opts):
    """The Alignment `align` asks for: "rigid" / "similarity" estimate it (pred, a pair or a Surface, against the grid of the Surface
    gt, with `align_opts` as keywords of align.icp_align), an Alignment or None is taken as it is."""
    if align is None or isinstance(align, al.Alignment):
        return align
    if align not in ALIGN_MODES:
        raise ValueError(f"align must be None, 'rigid', 'similarity' or an Alignment, got {align!r}")
    opts = dict(align_opts or {})
    if "scale" in opts:
        raise ValueError("align_opts: `scale` is what `align` decides")
    return al.icp_index(pred, gt.grid(), scale=align == "similarity", **opts)


def surface_metrics(pred, gt, samples=1_000_000, seed=0, taus=(), align=None, align_opts=None, signed=False, beta=wn.BETA):
    """Distances between the surfaces of pred = (verts [V,3], faces [F,3]) and gt, GPU tensors, as a dict of Python floats.  Either
    may be a surfdist_ops.Surface instead of a pair: what it has built is used, what is built here stays with it for the next call.

    `samples` points are drawn on each surface (surfdist_ops.sample_surface: area-weighted, stratified; pred with `seed`, gt with
    `seed + 1`) and each is given its exact distance to the other mesh (closest_point).  Per direction, `pred_to_gt` and `gt_to_pred`:
    `mean`, `rms`, `max` of those distances.  `chamfer` = (mean pred_to_gt + mean gt_to_pred) / 2: the L1 Chamfer distance, of
    distances and not of squared distances.  `p2s` = mean gt_to_pred, the direction the paper reports.  `normal_consistency` = the mean
    over both directions of the dot product between the sample's face normal and the unit normal of the closest face (signed; 0 for a
    closest face without area).  `fscore@tau` for every tau: 2 P R / (P + R) with P the share of pred_to_gt < tau and R the share of
    gt_to_pred < tau (0 when both are 0).  Reductions are torch's on fixed shapes, in double; two calls give identical numbers; the
    results come to the host in one copy (preparing a mesh and building its grid read their sizes on the way).

    `align` = None: no alignment or scaling.  "rigid" / "similarity": pred is first taken onto gt by align.icp_align (keywords in
    `align_opts`: samples, seed, iters, max_dist, tol, init, candidates, search_samples, top, refine_iters), its vertices are
    replaced by Alignment.apply of them, and `alignment` in the result carries matrix, scale, iterations, converged, rank, rms_before
    and rms_after, and `search` (Alignment.search) when `init` asked for a rotation search.  An Alignment is applied as it is.

    `signed` = True adds the block `signed`: per direction `mean`, the mean of the same samples' distances taken negative where the
    sample lies inside the other mesh (signed_distance with `beta`; a positive pred_to_gt mean says the prediction lies outside the
    ground truth there: inflated), and `inside_share`, the share of the samples inside; and `volume_pred` / `volume_gt`, the signed
    volumes of the two meshes (pred after the alignment).  It reuses the samples and distances, and its reductions ride in the same
    copy.  With `signed` = False the result is what it is without the keyword."""
    samples = int(samples)
    if samples <= 0:
        raise ValueError(f"samples > 0 expected, got {samples}")
    a, b = sd.Surface.of(pred, "MeshIndex.build"), sd.Surface.of(gt, "MeshIndex.build")
    found = _alignment(a, b, align, align_opts)
    if found is not None:
        a = a.moved(found.apply(a.verts))
    for name, m in (("pred", a), ("gt", b)):
        if not m.area > 0:
            raise ValueError(f"surface_metrics: the {name} mesh has no area")
    d_ab, n_ab, p_ab = _directed(a, b, samples, seed)
    d_ba, n_ba, p_ba = _directed(b, a, samples, seed + 1)
    names, vals = [], []
    for name, d in (("pred_to_gt", d_ab.double()), ("gt_to_pred", d_ba.double())):
        names += [(name, "mean"), (name, "rms"), (name, "max")]
        vals += [d.mean(), (d * d).mean().sqrt(), d.max()]
    names.append("normal_consistency")
    vals.append(0.5 * (n_ab.double().mean() + n_ba.double().mean()))
    taus = [float(t) for t in taus]
    for t in taus:
        names += [("P", t), ("R", t)]
        vals += [(d_ab < t).sum().double(), (d_ba < t).sum().double()]                 # (counts: the shares are divided on the host)
    if signed:
        wa, wb = a.pyramid(), b.pyramid()
        for name, d, pts, other in (("pred_to_gt", d_ab, p_ab, wb), ("gt_to_pred", d_ba, p_ba, wa)):
            w = wn.winding_number(pts, other, beta=beta)
            names += [("S", name, "mean"), ("S", name, "inside_share")]
            vals += [_signed(d, w).double().mean(), (w >= 0.5).sum().double()]
    host = torch.stack(vals).cpu().tolist()
    out, pr = {"pred_to_gt": {}, "gt_to_pred": {}}, {}
    for name, v in zip(names, host):
        if name == "normal_consistency":
            out[name] = v
        elif name[0] == "S":
            out.setdefault("signed", {"pred_to_gt": {}, "gt_to_pred": {}})[name[1]][name[2]] = v / samples if name[2] == "inside_share" else v
        elif name[0] in ("P", "R"):
            pr[name] = v
        else:
            out[name[0]][name[1]] = v
    out["chamfer"] = 0.5 * (out["pred_to_gt"]["mean"] + out["gt_to_pred"]["mean"])
    out["p2s"] = out["gt_to_pred"]["mean"]
    for t in taus:
        p, r = pr[("P", t)] / samples, pr[("R", t)] / samples
        out[f"fscore@{t:g}"] = 2. * p * r / (p + r) if p + r > 0 else 0.
    if signed:
        out["signed"]["volume_pred"], out["signed"]["volume_gt"] = wa.volume, wb.volume
    if found is not None:
        out["alignment"] = found.summary()
    return out


def vertex_to_surface(verts, gt, align=None, align_opts=None, faces=None, signed=False, beta=wn.BETA):
    """dist [V] float32: the distance of every vertex of verts [V,3] to the mesh gt = (verts, faces) or Surface -- for colouring a mesh
    (error_colors, write_error_mesh).  `align` as in surface_metrics; "rigid" / "similarity" need the `faces` [F,3] of verts, whose
    surface is what gets aligned.  With `signed` the distance of a vertex inside gt is negative (signed_distance with `beta`)."""
    gt = sd.Surface.of(gt, "MeshIndex.build")
    if align is not None:
        if faces is None and not isinstance(align, al.Alignment):
            raise ValueError("vertex_to_surface: estimating an alignment needs the faces of verts")
        verts = _alignment((verts, faces), gt, align, align_opts).apply(verts)
    if signed:
        return signed_distance(verts, gt.grid(), gt.pyramid(), beta)[0]
    return sd.closest_point(verts, gt.grid())[0]


def error_colors(d, limit, signed):
    """uint8 [V,3] red / green / blue of distances d [V] (torch ops on d's device): with t = clamp(d / limit, -1, 1), for t >= 0
    (255, 255 (1 - t), 255 (1 - t)), white to red -- outside, or too far --, and for t < 0 (255 (1 + t), 255 (1 + t), 255), white to
    blue -- inside.  Channels are rounded half up: floor(x + 1/2), in double.  `signed` = False uses the red half only: t = clamp(d
    / limit, 0, 1).  A NaN distance gives grey (128, 128, 128)."""
    limit = float(limit)
    if not (limit > 0 and np.isfinite(limit)):
        raise ValueError(f"error_colors: limit > 0 expected, got {limit}")
    t = (d.detach().double() / limit).clamp(-1. if signed else 0., 1.)
    fade = torch.floor(255. * (1. - t.abs()) + 0.5)
    full = torch.full_like(fade, 255.)
    rgb = torch.stack([torch.where(t >= 0, full, fade), fade, torch.where(t >= 0, fade, full)], 1)
    return torch.where(torch.isnan(t)[:, None], torch.full_like(rgb, 128.), rgb).to(torch.uint8)


def error_range(d):
    """The default range of the error map: the 95th percentile of |d| over the finite entries (the ceil(0.95 n)-th smallest), 1 when
    that is 0 or nothing is finite.  One device -> host read."""
    mag = d.detach().abs()
    mag = mag[torch.isfinite(mag)]
    if mag.numel() == 0:
        return 1.
    limit = float(torch.kthvalue(mag, max(1, int(np.ceil(0.95 * mag.numel()))))[0])
    return limit if limit > 0 else 1.


def write_error_mesh(path, pred, gt, alignment=None, signed=False, beta=wn.BETA, limit=None, out=print):
    """Writes pred = (verts, faces), taken through `alignment` (an Alignment or None), as a PLY coloured by error_colors of
    vertex_to_surface against gt (each a pair or a Surface); `limit` = None takes error_range of those distances and says so through
    `out`.  -> the limit."""
    verts, faces = pred
    if alignment is not None:
        verts = alignment.apply(verts)
    d = vertex_to_surface(verts, gt, signed=signed, beta=beta)
    if limit is None:
        limit = error_range(d)
        out("      error range %.6g (95th percentile of |d|) for %s" % (limit, path))
    write_ply(path, verts.cpu().numpy(), faces.cpu().numpy(), error_colors(d, limit, signed).cpu().numpy())
    return limit


def _surface(mesh, device):
    """The Surface, on `device`, of mesh = (verts, faces) as numpy arrays: a file is prepared once for everything asked of it."""
    verts, faces = torch.from_numpy(np.asarray(mesh[0], np.float32)).to(device), torch.from_numpy(np.asarray(mesh[1], np.int64)).to(device)
    return sd.Surface(verts, faces, "MeshIndex.build")


def write_columns(path, fids, columns):
    """geometry_errors.txt / geometry_signed.txt in the layout of infer's errors.txt: a line of the names of `columns` (name -> one
    value per frame), one line per frame, then mean / max / min and the ten worst frames (as positions in the list of compared frames,
    like `maxinds` there) of each column."""
    with open(path, "w") as ff:
        ff.write("      %s\n" % " ".join(columns))
        for fid, row in zip(fids, zip(*columns.values())):
            ff.write("%4s: %s\n" % (fid, " ".join("%.6f" % v for v in row)))
        for name, col in columns.items():
            col = np.asarray(col, np.float64)
            ff.write("%s mean: %.6f, max: %.6f, min: %.6f, maxinds:" % (name, col.mean(), col.max(), col.min()))
            for ind in (-col).argsort()[:10]:
                ff.write("%d " % ind)
            ff.write("\n")


def signed_line(block):
    """What folder mode prints under a frame with --signed."""
    return "      signed pred_to_gt %.6f (inside %.3f) gt_to_pred %.6f (inside %.3f)" % (
        block["pred_to_gt"]["mean"], block["pred_to_gt"]["inside_share"], block["gt_to_pred"]["mean"], block["gt_to_pred"]["inside_share"])


def search_line(search):
    """What folder mode prints under a frame whose alignment started from a rotation search."""
    k = search["top"].index(search["winner"])
    return "      search %s: candidate %d of %d, %.1f deg from the centroid start, J %.3g -> %.3g" % (
        search["kind"], search["winner"], search["candidates"], search["angle_deg"], search["score"][k], search["refined"][k])


def _frame_ids(folder):
    fids = [os.path.splitext(f)[0] for f in os.listdir(folder) if f.endswith(".npy")]
    return sorted(fids, key=lambda s: (0, int(s), s) if s.lstrip("-").isdigit() else (1, 0, s))


def evaluate_folder(rec_root, gt_root, device, frames=None, samples=1_000_000, seed=0, taus=(), out=print, align=None, align_opts=None,
                    align_shared=False, signed=False, beta=wn.BETA, error_meshes=False, limit=None):
    """Folder mode (see the module text).  -> dict(frames: {fid: metrics}, skipped: [fid], summary).  With `align_shared` the
    alignment is estimated on the first compared frame and applied to every frame.  `signed` adds the signed blocks, a line per frame
    and geometry_signed.txt; `error_meshes` writes geometry_errors/<fid>.ply (write_error_mesh with `limit`)."""
    _, faces = read_ply(os.path.join(rec_root, "tmp.ply"))
    faces_d = torch.from_numpy(faces).to(device)
    fids = _frame_ids(os.path.join(rec_root, "meshs"))
    if frames is not None:
        fids = fids[:int(frames)]
    per, skipped = {}, []
    for fid in fids:
        gt_file = next((p for p in (os.path.join(gt_root, fid + ext) for ext in (".ply", ".obj")) if os.path.isfile(p)), None)
        if gt_file is None:
            skipped.append(fid)
            continue
        verts = torch.from_numpy(np.load(os.path.join(rec_root, "meshs", fid + ".npy")).astype(np.float32).reshape(-1, 3)).to(device)
        pred, gt = sd.Surface(verts, faces_d, "MeshIndex.build"), _surface(read_mesh(gt_file), device)
        used = _alignment(pred, gt, align, align_opts)                                           # once per frame, against gt's kept grid
        align = used if align_shared else align
        per[fid] = surface_metrics(pred, gt, samples, seed, taus, used, signed=signed, beta=beta)
        out("%4s: chamfer %.6f p2s %.6f" % (fid, per[fid]["chamfer"], per[fid]["p2s"]))
        found = per[fid].get("alignment", {}).get("search")
        if found is not None:
            out(search_line(found))
        if signed:
            out(signed_line(per[fid]["signed"]))
        if error_meshes:
            os.makedirs(os.path.join(rec_root, "geometry_errors"), exist_ok=True)
            write_error_mesh(os.path.join(rec_root, "geometry_errors", fid + ".ply"), pred, gt, used, signed, beta, limit, out)
    out("%d frames compared, %d skipped (no ground-truth file)" % (len(per), len(skipped)))
    if not per:
        raise ValueError(f"evaluate: no frame of {rec_root}/meshs has a ground-truth file in {gt_root}")
    order = list(per)
    chamfer, p2s = [per[f]["chamfer"] for f in order], [per[f]["p2s"] for f in order]
    write_columns(os.path.join(rec_root, "geometry_errors.txt"), order, {"chamfer": chamfer, "p2s": p2s})
    if signed:
        write_columns(os.path.join(rec_root, "geometry_signed.txt"), order,
                      {k: [per[f]["signed"][k]["mean"] for f in order] for k in ("pred_to_gt", "gt_to_pred")})
    result = {"frames": per, "skipped": skipped,
              "summary": {"chamfer_mean": float(np.mean(chamfer)), "chamfer_max": float(np.max(chamfer)), "p2s_mean": float(np.mean(p2s)),
                          "p2s_max": float(np.max(p2s)), "samples": int(samples), "seed": int(seed)}}
    with open(os.path.join(rec_root, "geometry_errors.json"), "w") as fh:
        json.dump(result, fh, indent=1)
    return result


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m selfreconcode_amd.evaluate",
                                     description="Chamfer / P2S / normal consistency / F-score between triangle meshes on the GPU.  No alignment "
                                                 "and no scaling is applied by default: both meshes are taken in the coordinates they are given.  "
                                                 "--align first takes the predicted mesh onto the ground truth by point-to-plane ICP.")
    parser.add_argument("--gpu-ids", nargs="+", type=int, metavar="IDs", default=[0], help="gpu ids (the first is used)")
    parser.add_argument("--pred", default=None, metavar="A", help="mesh-pair mode: the predicted mesh (.ply / .obj)")
    parser.add_argument("--gt", default=None, metavar="B", help="mesh-pair mode: the ground-truth mesh (.ply / .obj)")
    parser.add_argument("--rec-root", default=None, metavar="R", help="folder mode: a result folder of infer (tmp.ply, meshs/<fid>.npy)")
    parser.add_argument("--gt-root", default=None, metavar="G", help="folder mode: the folder of <fid>.ply / <fid>.obj ground-truth meshes")
    parser.add_argument("--frames", default=None, type=int, metavar="N", help="folder mode: only the first N frames")
    parser.add_argument("--samples", default=1_000_000, type=int, metavar="N", help="surface samples per direction")
    parser.add_argument("--seed", default=0, type=int, metavar="S", help="seed of the sampler")
    parser.add_argument("--tau", nargs="*", type=float, default=[], metavar="t", help="F-score thresholds, in the meshes' units")
    parser.add_argument("--out", default=None, metavar="FILE.json", help="mesh-pair mode: also write the metrics here")
    parser.add_argument("--align", default="none", choices=("none",) + ALIGN_MODES,
                        help="align the predicted mesh onto the ground truth first: rigid, or similarity (with a scale); ICP from matched centroids")
    parser.add_argument("--align-samples", default=100_000, type=int, metavar="N", help="surface samples of the predicted mesh the alignment uses")
    parser.add_argument("--align-iters", default=30, type=int, metavar="K", help="ICP iterations launched (they stop updating once converged)")
    parser.add_argument("--align-max-dist", default=None, type=float, metavar="d", help="only pairs within this distance take part (default: all)")
    parser.add_argument("--align-init", default="centroid", choices=al.INITS,
                        help="the start of the ICP: matched centroids, nothing, or a rotation search in front of it -- the 24 rotations of the "
                             "cube (axes), or those and --align-candidates more (search) -- for a scan in any orientation")
    parser.add_argument("--align-candidates", default=4096, type=int, metavar="N", help="rotations --align-init search tries beyond the 24")
    parser.add_argument("--align-top", default=8, type=int, metavar="K", help="candidates of the search that are refined by short ICP runs")
    parser.add_argument("--align-shared", action="store_true",
                        help="folder mode: estimate the alignment on the first compared frame and use it for every frame (default: per frame)")
    parser.add_argument("--signed", action="store_true",
                        help="also say on which side the surfaces lie: signed means, inside shares and volumes (winding number)")
    parser.add_argument("--beta", default=wn.BETA, type=float, metavar="b",
                        help="--signed: a cluster of faces counts as one dipole from farther than b of its radii (>= 1; inf: never)")
    parser.add_argument("--error-range", default=None, type=float, metavar="d",
                        help="the distance at which the error map saturates (default: the 95th percentile of |d| over the mesh, printed)")
    parser.add_argument("--error-mesh", default=None, metavar="FILE.ply",
                        help="mesh-pair mode: write the (aligned) predicted mesh coloured by its vertices' distance to the ground truth")
    parser.add_argument("--error-meshes", action="store_true", help="folder mode: write such a mesh per frame, R/geometry_errors/<fid>.ply")
    return parser


def parse_args(argv=None):
    """The arguments, refused (SystemExit) unless exactly one of the two modes is given in full."""
    parser = build_parser()
    args = parser.parse_args(argv)
    pair, folder = (args.pred, args.gt), (args.rec_root, args.gt_root)
    if any(pair) and any(folder):
        parser.error("give either --pred / --gt or --rec-root / --gt-root, not both")
    if not any(pair) and not any(folder):
        parser.error("give --pred A --gt B (mesh-pair mode) or --rec-root R --gt-root G (folder mode)")
    if any(pair) and not all(pair):
        parser.error("mesh-pair mode needs both --pred and --gt")
    if any(folder) and not all(folder):
        parser.error("folder mode needs both --rec-root and --gt-root")
    if args.samples <= 0:
        parser.error("--samples must be positive")
    if args.align_samples <= 0 or args.align_iters <= 0:
        parser.error("--align-samples and --align-iters must be positive")
    if args.align_max_dist is not None and not args.align_max_dist >= 0:
        parser.error("--align-max-dist must not be negative")
    if args.align_candidates <= 0 or args.align_top <= 0:
        parser.error("--align-candidates and --align-top must be positive")
    if args.align == "none" and args.align_init != "centroid":
        parser.error("--align-init needs --align rigid or similarity")
    if args.align_shared and (args.align == "none" or not all(folder)):
        parser.error("--align-shared needs folder mode and --align rigid or similarity")
    if args.error_mesh is not None and not all(pair):
        parser.error("--error-mesh needs mesh-pair mode (folder mode: --error-meshes)")
    if args.error_meshes and not all(folder):
        parser.error("--error-meshes needs folder mode (mesh-pair mode: --error-mesh FILE.ply)")
    if args.error_range is not None and not (args.error_range > 0 and np.isfinite(args.error_range)):
        parser.error("--error-range must be positive")
    if not args.beta >= 1:
        parser.error("--beta must be at least 1")
    return args


def _align_args(args):
    """(align, align_opts) of surface_metrics from the parsed arguments."""
    if args.align == "none":
        return None, None
    return args.align, {"samples": args.align_samples, "seed": args.seed, "iters": args.align_iters, "max_dist": args.align_max_dist,
                        "init": args.align_init, "candidates": args.align_candidates, "top": args.align_top}


def main(argv=None, out=print):
    args = parse_args(argv)
    device = torch.device("cuda", args.gpu_ids[0])
    align, align_opts = _align_args(args)
    if args.pred:
        pred, gt = _surface(read_mesh(args.pred), device), _surface(read_mesh(args.gt), device)
        align = _alignment(pred, gt, align, align_opts)
        m = surface_metrics(pred, gt, args.samples, args.seed, args.tau, align, signed=args.signed, beta=args.beta)
        out(json.dumps(m))
        if args.error_mesh is not None:
            write_error_mesh(args.error_mesh, pred, gt, align, args.signed, args.beta, args.error_range, out)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(m, fh, indent=1)
        return m
    return evaluate_folder(args.rec_root, args.gt_root, device, args.frames, args.samples, args.seed, args.tau, out, align, align_opts,
                           args.align_shared, args.signed, args.beta, args.error_meshes, args.error_range)


if __name__ == "__main__":
    main()
