"""Numpy restatement of the winding-number evaluation (selfreconcode_amd.winding_ops / evaluate), written from the stated
semantics: w(p) = 1 / (4 pi) sum_f Omega_f(p), Omega = 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|) with a, b,
c the corners minus p.

`exact` in float64 is the truth; in float32 (every term in float32 in the stated order, the sum in double) it is the noise floor of the
number format, E32.  `build_tree` / `tree_query` restate the octree pyramid: same cube, same keys, same face-to-leaf map, same node
quantities, same acceptance test (which is float32 by definition: it decides what is summed, so it is part of the semantics); the sums
are float64 and level by level instead of depth first, which float64 does not notice."""
import math

import numpy as np

MAX_LEVELS = 7
LEAF_FACTOR = 2.0
WIDEN = np.float32(1. + 2. ** -10)
SHELLS = (0.05, 0.5, 0.9, 0.97, 1.03, 1.1, 2., 20.)


def solid_angles(p, tri, dtype=np.float64):
    """Omega [P,F] of points p [P,3] against triangles tri [F,3,3], every operation in `dtype` in the stated order."""
    p, tri = np.asarray(p, dtype), np.asarray(tri, dtype)
    a, b, c = (tri[None, :, k, :] - p[:, None, :] for k in range(3))

    def dot(u, v):
        return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]

    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    det = (a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) + a[..., 1] * (b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2])) \
        + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0])
    den = ((la * lb * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb
    return (dtype(2) * np.arctan2(det, den)).astype(dtype)


def exact(p, verts, faces, dtype=np.float64, chunk=4096):
    """w [P] float64: the sum over all faces; NaN for a non-finite point."""
    p = np.asarray(p)
    tri = np.asarray(verts)[np.asarray(faces)]
    w = np.full(len(p), np.nan)
    ok = np.isfinite(p).all(1)
    total = np.zeros(int(ok.sum()))
    for f0 in range(0, len(tri), chunk):
        total += solid_angles(p[ok], tri[f0:f0 + chunk], dtype).astype(np.float64).sum(1)
    w[ok] = total / (4. * np.pi)
    return w


def e32(p, verts, faces):
    """(w64, E32): the float64 sum and the largest error of its float32 twin on the same input."""
    w64 = exact(p, verts, faces)
    w32 = exact(np.asarray(p, np.float32), np.asarray(verts, np.float32), faces, np.float32)
    ok = np.isfinite(w64)
    return w64, float(np.abs(w32[ok] - w64[ok]).max(initial=0.))


def shell_points(n, seed, shells=SHELLS):
    """n points on spheres of the radii `shells` round the origin, float32."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * np.asarray(shells)[np.arange(n) % len(shells), None]).astype(np.float32)


def signed_volume(verts, faces):
    t = np.asarray(verts, np.float64)[np.asarray(faces)]
    return float((t[:, 0] * np.cross(t[:, 1], t[:, 2])).sum() / 6.)


# ------------------------------------------------------------------------------------------------------------ the tree
def level_offset(level):
    return (8 ** level - 1) // 7


def cube(verts):
    """(corner [3] float32, side float32): the box's longest side times WIDEN (1 for a point), centred on the box, in float32."""
    v = np.asarray(verts, np.float32)
    lo, hi = v.min(0), v.max(0)
    side = np.float32((hi - lo).max()) * WIDEN
    if not side > 0:
        side = np.float32(1.)
    return (lo + hi) * np.float32(0.5) - np.float32(0.5) * side, side


def default_levels(side, area, faces, leaf_factor=LEAF_FACTOR):
    if not area > 0:
        return 0
    leaf = leaf_factor * math.sqrt(area / faces)
    return int(min(max(math.floor(math.log2(float(side) / leaf) + 0.5), 0), MAX_LEVELS))


def _spread3(x):
    out = np.zeros_like(x)
    for b in range(MAX_LEVELS + 1):
        out |= ((x >> b) & 1) << (3 * b)
    return out


def leaf_keys(xyz, corner, cell, levels):
    """Morton index of the leaf of each row of xyz [n,3] float32: floor((x - corner) / cell) in float32, clamped to [0, 2^levels - 1],
    bit b of the coordinate on axis a at bit 3 b + a."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((np.asarray(xyz, np.float32) - corner) / np.float32(cell))
    t = np.where(t > 0, t, np.float32(0))                  # (NaN -> 0)
    ijk = np.minimum(t, np.float32((1 << levels) - 1)).astype(np.int64)
    return _spread3(ijk[:, 0]) | (_spread3(ijk[:, 1]) << 1) | (_spread3(ijk[:, 2]) << 2)


def clean(faces):
    faces = np.asarray(faces, np.int64)
    return faces[(faces >= 0).all(1)]


def build_tree(verts, faces, levels=None, leaf_factor=LEAF_FACTOR):
    """dict(corner, cell, levels, nodes [n,8] float32, leaf_start, leaf_faces) of the mesh (faces cleaned of their negative rows)."""
    v32, faces = np.asarray(verts, np.float32), clean(faces)
    tri32 = v32[faces]
    tri = tri32.astype(np.float64)
    fn = 0.5 * np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fa = np.linalg.norm(fn, axis=1)
    corner, side = cube(v32)
    if levels is None:
        levels = default_levels(side, float(fa.sum()), len(faces), leaf_factor)
    cell = side / np.float32(1 << levels)
    cen32 = ((tri32[:, 0] + tri32[:, 1]) + tri32[:, 2]) / np.float32(3)
    key = leaf_keys(cen32, corner, cell, levels)
    order = np.argsort(key, kind="stable")
    leaves = 8 ** levels
    leaf_start = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=leaves))]).astype(np.int64)
    nodes = np.zeros((level_offset(levels + 1), 8), np.float32)
    # leaves: double sums over each leaf's faces
    N, A, M = np.zeros((leaves, 3)), np.zeros(leaves), np.zeros((leaves, 3))
    np.add.at(N, key, fn)
    np.add.at(A, key, fa)
    np.add.at(M, key, fa[:, None] * (((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / 3.))
    any_ = A > 0
    c = np.where(any_[:, None], M / np.where(any_, A, 1.)[:, None], 0.).astype(np.float32)
    r2 = np.zeros(leaves)
    np.maximum.at(r2, key, ((tri - c.astype(np.float64)[key][:, None, :]) ** 2).sum(-1).max(1))
    base = level_offset(levels)
    nodes[base:, 0:3], nodes[base:, 3:6], nodes[base:, 6], nodes[base:, 7] = N, c, A, np.where(any_, np.sqrt(r2), 0.)
    # upper levels: each parent from its eight float32 children, in double
    for level in range(levels - 1, -1, -1):
        count = 8 ** level
        ch = nodes[level_offset(level + 1):level_offset(level + 2)].astype(np.float64).reshape(count, 8, 8)
        a = np.where(ch[:, :, 6] > 0, ch[:, :, 6], 0.)
        A = a.sum(1)
        any_ = A > 0
        c = np.where(any_[:, None], (a[:, :, None] * ch[:, :, 3:6]).sum(1) / np.where(any_, A, 1.)[:, None], 0.).astype(np.float32)
        reach = np.linalg.norm(ch[:, :, 3:6] - c.astype(np.float64)[:, None, :], axis=2) + ch[:, :, 7]
        r = np.where(ch[:, :, 6] > 0, reach, 0.).max(1)
        b = level_offset(level)
        nodes[b:b + count, 0:3], nodes[b:b + count, 3:6], nodes[b:b + count, 6], nodes[b:b + count, 7] = ch[:, :, 0:3].sum(1), c, A, r
    return {"corner": corner, "cell": float(cell), "levels": int(levels), "nodes": nodes, "leaf_start": leaf_start,
            "leaf_faces": order.astype(np.int32), "verts": v32, "faces": faces}


def tree_query(p, tree, beta, nodes=None, counts=None):
    """w [P] float64 of the walk over `tree` (with `nodes` in place of its own node array, if given): a node without area is skipped; a
    node with |p - c|^2 > (beta r)^2, evaluated in float32 as (dx dx + dy dy) + dz dz against (beta r)(beta r), contributes -N . d /
    (4 pi |d|^3); otherwise a leaf contributes its faces exactly and an inner node is opened.  beta = inf accepts nothing.  NaN for a
    non-finite point.  `counts`, a dict, receives the accepted nodes and exact faces per point."""
    nodes = tree["nodes"] if nodes is None else np.asarray(nodes, np.float32)
    p32 = np.asarray(p, np.float32)
    tri = tree["verts"].astype(np.float64)[tree["faces"]]
    levels, beta32 = tree["levels"], np.float32(beta)
    ok = np.isfinite(p32).all(1)
    total = np.zeros(len(p32))
    accepted, exact_faces = np.zeros(len(p32), np.int64), np.zeros(len(p32), np.int64)
    pi, ni = np.nonzero(ok)[0], np.zeros(int(ok.sum()), np.int64)
    for level in range(levels + 1):
        n = nodes[level_offset(level) + ni]
        live = n[:, 6] > 0
        d = p32[pi] - n[:, 3:6]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        with np.errstate(invalid="ignore", over="ignore"):
            br = beta32 * n[:, 7]
            far = live & (d2 > br * br) & bool(np.isfinite(beta32))
        d64, n64 = p32[pi][far].astype(np.float64) - n[far, 3:6].astype(np.float64), n[far, 0:3].astype(np.float64)
        np.add.at(total, pi[far], -(n64 * d64).sum(1) / np.linalg.norm(d64, axis=1) ** 3)
        np.add.at(accepted, pi[far], 1)
        rest = live & ~far
        if level < levels:
            pi, ni = np.repeat(pi[rest], 8), (ni[rest][:, None] * 8 + np.arange(8)).reshape(-1)
            continue
        s, e = tree["leaf_start"][ni[rest]], tree["leaf_start"][ni[rest] + 1]
        cnt = e - s
        pp = np.repeat(pi[rest], cnt)
        ff = tree["leaf_faces"][np.repeat(s, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
        for k0 in range(0, len(pp), 1 << 18):
            sl = slice(k0, k0 + (1 << 18))
            np.add.at(total, pp[sl], _pairwise(p32[pp[sl]].astype(np.float64), tri[ff[sl]]))
        np.add.at(exact_faces, pp, 1)
    if counts is not None:
        counts["accepted"], counts["faces"] = accepted, exact_faces
    w = total / (4. * np.pi)
    w[~ok] = np.nan
    return w


def _pairwise(q, t):
    """Omega [n] float64 of point q[i] against triangle t[i]."""
    a, b, c = t[:, 0] - q, t[:, 1] - q, t[:, 2] - q
    la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
    det = (a * np.cross(b, c)).sum(1)
    den = la * lb * lc + (a * b).sum(1) * lc + (b * c).sum(1) * la + (c * a).sum(1) * lb
    return 2. * np.arctan2(det, den)


def open_sphere(verts, faces, z=0.8):
    """The faces whose centroid lies at z <= `z`: the sphere with its cap removed."""
    faces = np.asarray(faces)
    return faces[np.asarray(verts, np.float64)[faces].mean(1)[:, 2] <= z]
