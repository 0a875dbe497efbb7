"""Float64 numpy restatement of the quadric-optimal vertex placement of the template simplification (selfreconcode_amd.mesh_prep,
placement="quadric"), the face-flip count, and the shapes and error measures its tests use.  Written from the stated
semantics, not from the kernels: np.add.at over the (face, corner) pairs in face order, np.linalg.solve, np.clip.  The clustering is
_meshprep_ref's."""
import numpy as np

import _meshprep_ref as mr


def clean(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return f[(f >= 0).all(1)]


def surviving(vmap, faces):
    """Indices (into the cleaned faces) of the faces that survive the clustering, as _meshprep_ref.simplify keeps them."""
    seen, keep = set(), []
    for i, (a, b, c) in enumerate(vmap[faces].tolist()):
        if a == b or b == c or a == c:
            continue
        s = frozenset((a, b, c))
        if s not in seen:
            seen.add(s)
            keep.append(i)
    return np.asarray(keep, np.int64)


def face_planes(v, f):
    """(n [F,3], w [F], d [F], ok [F]) of faces f at float64 positions v: unit normal, area, offset; ok = the face has a finite area > 0."""
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        N = np.cross(p1 - p0, p2 - p0)
        L = np.sqrt((N * N).sum(1))
        ok = np.isfinite(L) & (L > 0)
        n = N / np.where(ok, L, 1.)[:, None]
        return n, L / 2, (n * p0).sum(1), ok


def simplify_quadric(verts, faces, cell, reg=1e-3):
    """-> dict(verts [C,3] float64 (clamped optima, not rounded), mean [C,3], faces, vertex_map, source (surviving faces' indices into
    the cleaned faces), clamped [C] bool, no_planes [C] bool, near_wall [C] bool: the unclamped optimum lies within 1e-9 cell of a wall of
    its box, max_shift: the largest |x - m| / cell)."""
    v32 = np.asarray(verts, np.float32)
    v = v32.astype(np.float64)
    f = clean(faces)
    base = mr.simplify(v32, f, cell)
    vmap, m = base["vertex_map"], base["verts"]
    key, n = mr.cell_keys(v32, cell)
    cells = np.unique(key)
    C = len(cells)
    A, b = np.zeros((C, 3, 3)), np.zeros((C, 3))
    if len(f):
        nrm, w, d, ok = face_planes(v, f)
        g = vmap[f]
        feeds = np.stack([np.ones(len(f), bool), g[:, 1] != g[:, 0], (g[:, 2] != g[:, 0]) & (g[:, 2] != g[:, 1])], 1) & ok[:, None]
        face = np.repeat(np.arange(len(f)), 3)[feeds.reshape(-1)]                 # (face, corner) pairs in face order: one entry per distinct cell
        cell_of = g.reshape(-1)[feeds.reshape(-1)]
        with np.errstate(all="ignore"):
            np.add.at(A, cell_of, (w[:, None, None] * nrm[:, :, None] * nrm[:, None, :])[face])
            np.add.at(b, cell_of, ((w * d)[:, None] * nrm)[face])
    with np.errstate(all="ignore"):
        lam = float(reg) * np.trace(A, axis1=1, axis2=2) / 3.
        solve = lam > 0
        x = m.copy()
        if solve.any():
            M = A[solve] + lam[solve, None, None] * np.eye(3)
            r = b[solve] - np.einsum("cij,cj->ci", A[solve], m[solve])
            x[solve] = m[solve] + np.linalg.solve(M, r[:, :, None])[:, :, 0]
    bad = ~np.isfinite(x).all(1)
    x[bad] = m[bad]
    no_planes = ~solve | bad
    lo, h = v32.min(0).astype(np.float64), float(np.float32(cell))
    ijk = np.stack([cells % n[0], (cells // n[0]) % n[1], cells // (n[0] * n[1])], 1).astype(np.float64)
    wlo, whi = lo + ijk * h, lo + (ijk + 1) * h
    clamped = ((x < wlo) | (x > whi)).any(1)
    near = (np.minimum(np.abs(x - wlo), np.abs(x - whi)).min(1) <= 1e-9 * h)
    xc = np.clip(x, wlo, whi)
    return {"verts": xc, "mean": m, "faces": base["faces"], "vertex_map": vmap, "source": surviving(vmap, f), "clamped": clamped,
            "no_planes": no_planes, "near_wall": near, "max_shift": float(np.sqrt(((xc - m) ** 2).sum(1)).max() / h)}


def face_flips(verts, faces, new_verts, new_faces, source):
    """(flipped, zero_area): new faces whose unnormalised normal has a negative dot product with that of faces[source], or is zero."""
    if len(new_faces) == 0:
        return 0, 0
    v, nv = np.asarray(verts, np.float64), np.asarray(new_verts, np.float64)

    def normal(p, t):
        return np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    N0, N1 = normal(v, clean(faces)[source]), normal(nv, np.asarray(new_faces, np.int64))
    flat = (N1 == 0).all(1)
    return int((((N0 * N1).sum(1) < 0) & ~flat).sum()), int(flat.sum())


# ------------------------------------------------------------------------------------------------ shapes
def uv_sphere(nlon=64, nlat=32):
    """Unit sphere: two poles and nlat - 1 rings of nlon vertices (64 x 32: 1986 vertices, 3968 faces), outward normals."""
    th = np.pi * np.arange(1, nlat) / nlat
    ph = 2 * np.pi * np.arange(nlon) / nlon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None], np.cos(th)[:, None] * np.ones(nlon)[None]], -1)
    verts = np.concatenate([[[0., 0., 1.]], ring.reshape(-1, 3), [[0., 0., -1.]]]).astype(np.float32)
    j, jn = np.arange(nlon), (np.arange(nlon) + 1) % nlon
    faces = [np.stack([np.zeros(nlon, np.int64), 1 + j, 1 + jn], 1)]
    for r in range(nlat - 2):
        a, b = 1 + r * nlon, 1 + (r + 1) * nlon
        faces += [np.stack([a + j, b + j, b + jn], 1), np.stack([a + j, b + jn, a + jn], 1)]
    last, south = 1 + (nlat - 2) * nlon, 1 + (nlat - 1) * nlon
    faces.append(np.stack([last + j, np.full(nlon, south), last + jn], 1))
    return verts, np.concatenate(faces).astype(np.int64)


def cube(n=12):
    """The cube [-1, 1]^3 with n x n quads per side, shared vertices (n = 12: 866 vertices, 1728 faces), outward normals."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append([2. * c / n - 1. for c in p])
        return index[p]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        quad.append(vid(tuple(p)))
                    if side == 0:
                        quad.reverse()                                            # (e_u x e_w = e_axis: reversed on the low side)
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.float32(verts), np.int64(faces)


def flat_grid(n, z=0.):
    """n x n vertices at integer (x, y) in the plane `z`, 2 (n - 1)^2 faces with normal +z; vertex j n + i is (i, j, z)."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    verts = np.stack([i.reshape(-1), j.reshape(-1), np.full(n * n, z)], 1).astype(np.float32)
    q = (np.arange(n - 1)[None, :] + n * np.arange(n - 1)[:, None]).reshape(-1)
    faces = np.stack([np.stack([q, q + 1, q + n + 1], 1), np.stack([q, q + n + 1, q + n], 1)], 1).reshape(-1, 3)
    return verts, faces.astype(np.int64)


# ------------------------------------------------------------------------------------------------ error measures
def sample_surface(verts, faces, n, seed):
    """n area-weighted uniform samples of the surface (numpy's generator; the GPU tests draw theirs with surfdist_ops.sample_surface)."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1)
    rng = np.random.default_rng(seed)
    t = rng.choice(len(f), n, p=area / area.sum())
    su, w = np.sqrt(rng.random(n))[:, None], rng.random(n)[:, None]
    return (1 - su) * p0[t] + su * (1 - w) * p1[t] + su * w * p2[t]


def volume(verts, faces):
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.)


def sphere_error(points):
    """mean | |s| - 1 |"""
    return float(np.abs(np.linalg.norm(np.asarray(points, np.float64), axis=1) - 1.).mean())


def cube_distance(points):
    """[n]: the distance of every point to the surface of [-1, 1]^3."""
    q = np.abs(np.asarray(points, np.float64)) - 1.
    return np.linalg.norm(np.maximum(q, 0.), axis=1) + np.maximum(-q.max(1), 0.)


SHAPES = ("sphere", "sphere_jitter", "cube", "cube_jitter")
CELLS = (0.61, 0.43, 0.31)
_SHAPES = {}


def shape(name):
    """(verts float32, faces): the UV sphere 64 x 32 and the cube of 12 x 12 quads per side, plain or with a seeded 0.002 Gaussian jitter."""
    if name not in _SHAPES:
        v, f = uv_sphere(64, 32) if name.startswith("sphere") else cube(12)
        _SHAPES[name] = (mr.jitter(v, 7, 0.002) if name.endswith("jitter") else v, f)
    return _SHAPES[name]


def quality(name, verts, faces, points=None):
    """The figures the quality conditions compare, for a simplified mesh of shape `name`: dict(surface: the mean distance of surface
    samples to the true surface (`points`: samples drawn elsewhere), volume: |1 - volume / true volume|, vertex: the largest vertex
    distance to the true surface)."""
    pts = sample_surface(verts, faces, 20000, 1) if points is None else np.asarray(points, np.float64)
    v = np.asarray(verts, np.float64)
    if name.startswith("sphere"):
        return {"surface": sphere_error(pts), "volume": abs(1. - volume(verts, faces) / (4. * np.pi / 3.)), "vertex": float(np.abs(np.linalg.norm(v, axis=1) - 1.).max())}
    return {"surface": float(cube_distance(pts).mean()), "volume": abs(1. - volume(verts, faces) / 8.), "vertex": float(cube_distance(v).max())}
