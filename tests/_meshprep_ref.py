"""Float64 numpy restatement of the template preparation (selfreconcode_amd.mesh_prep) and the small meshes its tests
use.  Written from the stated semantics, not from the kernels: a dictionary of seen vertex sets instead of sorts, union-find instead of
hooking, np.add.at instead of a per-cell loop.  It does not restate the packer: `chart_uv` recomputes vt from the product's scale, origin
and bbox_min."""
import numpy as np


# ------------------------------------------------------------------------------------------------ simplify
def cell_keys(verts, cell):
    """(key [V] int64, n [3]): float32 subtraction and division, as stated."""
    v = np.asarray(verts, np.float32)
    lo = v.min(0)
    ijk = np.floor((v - lo) / np.float32(cell)).astype(np.int64)
    n = ijk.max(0) + 1
    return (ijk[:, 2] * n[1] + ijk[:, 1]) * n[0] + ijk[:, 0], n


def simplify(verts, faces, cell):
    """-> dict(verts [Vn,3] float64, faces [Fn,3], vertex_map [V], members [Vn]: the cells' sizes)."""
    v = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[(f >= 0).all(1)]
    key, _ = cell_keys(v, cell)
    cells, vmap, members = np.unique(key, return_inverse=True, return_counts=True)
    vmap = vmap.reshape(-1)
    sums = np.zeros((len(cells), 3))
    np.add.at(sums, vmap, v.astype(np.float64))                      # (unbuffered, in index order)
    g = vmap[f]
    seen, keep = set(), []
    for i, (a, b, c) in enumerate(g.tolist()):
        if a == b or b == c or a == c:
            continue
        s = frozenset((a, b, c))
        if s not in seen:
            seen.add(s)
            keep.append(i)
    return {"verts": sums / members[:, None], "faces": g[keep].reshape(-1, 3), "vertex_map": vmap, "members": members}


def position_bound(ref, verts):
    """(n_max + 2) 2^-24 max |coordinate|: a float32 sum of n_max terms and the division (the product may do better)."""
    return (int(ref["members"].max()) + 2) * 2. ** -24 * float(np.abs(np.asarray(verts, np.float64)).max())


# ------------------------------------------------------------------------------------------------ unwrap
def face_classes(verts, faces):
    """2 axis + (negative ? 1 : 0); numpy rounds every product and difference on its own, argmax takes the first maximum."""
    p = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    u, w = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    k = np.argmax(np.abs(n), 1)
    return (2 * k + (n[np.arange(len(k)), k] < 0)).astype(np.int32), n


def chart_labels(faces, cls):
    """label [F]: the lowest face index among the faces connected to it through edges shared by faces of its class (union-find)."""
    f = np.asarray(faces, np.int64)
    parent = list(range(len(f)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    first = {}
    for i, tri in enumerate(f.tolist()):
        for c in range(3):
            a, b = tri[c], tri[(c + 1) % 3]
            if a == b:
                continue
            e = (min(a, b), max(a, b), int(cls[i]))
            if e in first:
                ra, rb = find(first[e]), find(i)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            else:
                first[e] = i
    return np.array([find(i) for i in range(len(f))], np.int64)


def project(verts, faces, cls):
    """uv [F,3,2] float32: (x_{k+1}, x_{k+2}) of the corners, swapped for a negative sign."""
    p = np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]
    k, neg = cls // 2, (cls % 2).astype(bool)
    i = np.arange(len(k))
    s, t = p[i, :, (k + 1) % 3], p[i, :, (k + 2) % 3]
    return np.stack([np.where(neg[:, None], t, s), np.where(neg[:, None], s, t)], -1)


def charts(verts, faces):
    """-> dict(cls, chart [F], labels [C], bbox_min [C,2] float32, extent [C,2] float32 (a float32 subtraction), uv [F,3,2])."""
    cls, _ = face_classes(verts, faces)
    label = chart_labels(faces, cls)
    labels, chart = np.unique(label, return_inverse=True)
    chart = chart.reshape(-1)
    uv = project(verts, faces, cls)
    C = len(labels)
    lo = np.full((C, 2), np.inf, np.float32); hi = np.full((C, 2), -np.inf, np.float32)
    np.minimum.at(lo, chart, uv.min(1)); np.maximum.at(hi, chart, uv.max(1))
    return {"cls": cls, "chart": chart, "labels": labels, "bbox_min": lo, "extent": hi - lo, "uv": uv}


def chart_uv(ref, scale, origin, bbox_min, padding, R):
    """vt [3F,2] float64 of the stated expression, from the product's packing."""
    c = ref["chart"]
    o = np.asarray(origin, np.float64)[c][:, None, :]; b = np.asarray(bbox_min, np.float64)[c][:, None, :]
    return ((o + padding + 0.5 + (ref["uv"].astype(np.float64) - b) * float(scale)) / R).reshape(-1, 2)


def tri_area2(p):
    """twice the signed area of 2-D triangles p [F,3,2]"""
    return (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])


def overlap_count(vt, ft, R, eps=1e-6, near=1e-4):
    """(contested, doubtful): texel centres (u = (c + 0.5) / R, v = 1 - (r + 0.5) / R) with every barycentric > eps in two or more
    triangles, and the texel centres where some triangle's smallest barycentric is within `near` of eps (only those may be counted
    otherwise in another precision)."""
    vt = np.asarray(vt, np.float64); ft = np.asarray(ft, np.int64)
    cnt = np.zeros((R, R), np.int64); doubt = np.zeros((R, R), bool)
    for a, b, c in vt[ft]:
        area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if not abs(area2) > 1e-14:
            continue
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        c0, c1 = max(int(np.floor(lo[0] * R - 0.5)) - 1, 0), min(int(np.ceil(hi[0] * R - 0.5)) + 1, R - 1)
        r0, r1 = max(int(np.floor((1 - hi[1]) * R - 0.5)) - 1, 0), min(int(np.ceil((1 - lo[1]) * R - 0.5)) + 1, R - 1)
        if c1 < c0 or r1 < r0:
            continue
        rr, cc = np.meshgrid(np.arange(r0, r1 + 1), np.arange(c0, c1 + 1), indexing="ij")
        u, v = (cc + 0.5) / R, 1. - (rr + 0.5) / R
        e0 = ((c[0] - b[0]) * (v - b[1]) - (c[1] - b[1]) * (u - b[0])) / area2
        e1 = ((a[0] - c[0]) * (v - c[1]) - (a[1] - c[1]) * (u - c[0])) / area2
        m = np.minimum(np.minimum(e0, e1), 1. - e0 - e1)
        cnt[r0:r1 + 1, c0:c1 + 1] += m > eps
        doubt[r0:r1 + 1, c0:c1 + 1] |= np.abs(m - eps) <= near
    return int((cnt >= 2).sum()), int(doubt.sum())


# ------------------------------------------------------------------------------------------------ meshes
def jitter(verts, seed, scale=0.01):
    v = np.asarray(verts, np.float32)
    return (v + np.random.default_rng(seed).normal(0., scale, v.shape)).astype(np.float32)


def flat_strip(n):
    """1 x n quads in the plane z = 0, normals +z: 2 (n + 1) vertices, 2 n faces; face 2 q and 2 q + 1 make quad q."""
    i = np.arange(n + 1, dtype=np.float32)
    verts = np.concatenate([np.stack([i, np.zeros_like(i), np.zeros_like(i)], 1), np.stack([i, np.ones_like(i), np.zeros_like(i)], 1)])
    q = np.arange(n)
    a, b, c, d = q, q + 1, q + 1 + (n + 1), q + (n + 1)
    return verts, np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int64)


def spiral_ramp(turns=2, segments=64, r0=1., r1=2., pitch=0.15):
    """A ramp that winds `turns` times round the z axis: one connected patch of class +z that covers itself in the xy projection."""
    n = turns * segments
    th = 2 * np.pi * np.arange(n + 1) / segments
    z = pitch * th / (2 * np.pi)
    verts = np.concatenate([np.stack([r0 * np.cos(th), r0 * np.sin(th), z], 1), np.stack([r1 * np.cos(th), r1 * np.sin(th), z], 1)]).astype(np.float32)
    q = np.arange(n)
    a, b, c, d = q, q + (n + 1), q + 1 + (n + 1), q + 1                # inner, outer, outer next, inner next
    return verts, np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int64)


def fan_on_edge():
    """Three faces of class +z on the edge (0, 1): one chart although the edge is not manifold."""
    verts = np.float32([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 2, 0.1], [0.5, 3, 0.2]])
    return verts, np.int64([[0, 1, 2], [0, 1, 3], [0, 1, 4]])
