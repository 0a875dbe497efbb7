"""float64 numpy restatement of the textured renderer's three entries (include/selfrecon_hip.h: sr_texture_mips, sr_texture_face_lod,
sr_shade_textured) and of render.turntable_vertices, written from their stated semantics, not from the kernels."""
import numpy as np


def layout(R):
    """(sides, offsets): level l + 1 has side (R_l + 1) // 2 down to 1; a level starts where the one before ends."""
    sides = [int(R)]
    while sides[-1] > 1:
        sides.append((sides[-1] + 1) // 2)
    return sides, [int(x) for x in np.concatenate([[0], np.cumsum([s * s for s in sides[:-1]])])]


def mips(texture, valid=None):
    """-> list of [R_l,R_l,4] float64 levels.  A uint8 texture is x / 255 in float32 (the kernel's IEEE division), then exact."""
    tex = np.asarray(texture)
    rgb = (tex.astype(np.float32) / np.float32(255.)).astype(np.float64) if tex.dtype == np.uint8 else tex.astype(np.float64)
    R = rgb.shape[0]
    w = np.ones((R, R)) if valid is None else (np.asarray(valid) != 0).astype(np.float64)
    levels = [np.concatenate([rgb * w[..., None], w[..., None]], -1)]
    while levels[-1].shape[0] > 1:
        src = levels[-1]
        m = src.shape[0]
        n = (m + 1) // 2
        pad = np.zeros((2 * n, 2 * n, 4))
        pad[:m, :m] = src
        cnt = np.zeros((2 * n, 2 * n))
        cnt[:m, :m] = 1.
        s = pad[0::2, 0::2] + pad[0::2, 1::2] + pad[1::2, 0::2] + pad[1::2, 1::2]
        c = cnt[0::2, 0::2] + cnt[0::2, 1::2] + cnt[1::2, 0::2] + cnt[1::2, 1::2]
        levels.append(s / c[..., None])
    return levels


def face_lod(xy_pix, faces, vt, ft, R, bias, L):
    """lod [N,F] float64."""
    xy, vt = np.asarray(xy_pix, np.float64), np.asarray(vt, np.float64)
    faces, ft = np.asarray(faces, np.int64), np.asarray(ft, np.int64)
    N, V = xy.shape[:2]
    out = np.full((N, faces.shape[0]), float(L - 1))
    for f in range(faces.shape[0]):
        if (faces[f] < 0).any() or (faces[f] >= V).any() or (ft[f] < 0).any() or (ft[f] >= vt.shape[0]).any():
            continue
        t = vt[ft[f]]
        U = np.stack([t[1] - t[0], t[2] - t[0]], 1)                       # columns: uv edges
        for n in range(N):
            p = xy[n, faces[f]]
            E = np.stack([p[1] - p[0], p[2] - p[0]], 1)                   # columns: pixel edges
            if abs(np.linalg.det(E)) < 1e-12:
                continue
            J = U @ np.linalg.inv(E)                                      # d uv / d (x, y)
            rho = R * max(np.linalg.norm(J[:, 0]), np.linalg.norm(J[:, 1]))
            with np.errstate(divide='ignore'):
                out[n, f] = min(max(np.log2(rho) + bias, 0.), L - 1.)
    return out


def sample_level(level, u, v):
    """Bilinear, clamp to edge: u, v [P] -> [P,4]."""
    n = level.shape[0]
    x, y = u * n - 0.5, (1. - v) * n - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]

    def tap(yy, xx):
        return level[np.clip(yy, 0, n - 1).astype(np.int64), np.clip(xx, 0, n - 1).astype(np.int64)]
    return ((1. - fx) * (1. - fy) * tap(y0, x0) + fx * (1. - fy) * tap(y0, x0 + 1) + (1. - fx) * fy * tap(y0 + 1, x0)
            + fx * fy * tap(y0 + 1, x0 + 1))


def shade(pix_to_face, bary, ft, vt, levels, lod, background=(1., 1., 1.), hole=(.5, .5, .5), bg_image=None):
    """-> rgba [N,H,W,4], coverage [N,H,W], covered [N,H,W] bool (float64).  `lod` [N,F] is taken as given.  Colours given as Python
    floats are rounded to float32 first, as the entry receives them."""
    p2f = np.asarray(pix_to_face, np.int64)
    N, H, W = p2f.shape
    ft, vt, lod = np.asarray(ft, np.int64), np.asarray(vt, np.float64), np.asarray(lod, np.float64)
    F, L = ft.shape[0], len(levels)
    rgba = np.zeros((N, H, W, 4))
    rgba[..., :3] = np.asarray(background, np.float32).astype(np.float64) if bg_image is None else np.asarray(bg_image, np.float64)
    cov = np.zeros((N, H, W))
    inrange = (p2f >= 0) & (p2f < N * F)
    f = np.where(inrange, p2f % F, 0)
    covered = inrange & ((ft[f] >= 0) & (ft[f] < vt.shape[0])).all(-1)
    idx = np.nonzero(covered)
    p = p2f[idx]
    b = np.asarray(bary, np.float64)[idx]
    uv = np.einsum('pk,pkj->pj', b, vt[ft[p % F]])
    l = lod.reshape(-1)[p]
    l0 = np.floor(l).astype(np.int64)
    l1 = np.minimum(l0 + 1, L - 1)
    t = (l - l0)[:, None]
    s = np.zeros((p.shape[0], 4))
    for k in range(L):
        a = l0 == k
        if a.any():
            s[a] += (1. - t[a]) * sample_level(levels[k], uv[a, 0], uv[a, 1])
        a = l1 == k
        if a.any():
            s[a] += t[a] * sample_level(levels[k], uv[a, 0], uv[a, 1])
    w = s[:, 3]
    out = np.empty((p.shape[0], 4))
    out[:, 3] = 1.
    out[:, :3] = np.asarray(hole, np.float32).astype(np.float64)
    pos = w > 0
    out[pos, :3] = s[pos, :3] / w[pos, None]
    rgba[idx] = out
    cov[idx] = w
    return rgba, cov, covered


def turntable_vertices(verts, K):
    v = np.asarray(verts, np.float64)
    c = v.mean(0)
    out = [v]
    for k in range(1, K):
        a = 2. * np.pi * k / K
        Ry = np.array([[np.cos(a), 0., np.sin(a)], [0., 1., 0.], [-np.sin(a), 0., np.cos(a)]])
        out.append(c + (v - c) @ Ry.T)
    return np.stack(out)
