"""float64 numpy restatement of the texture bake (steps 2-8 of selfreconcode_amd/texture.py's docstring), written from that list and
from texture_mesh_extract.py's use of opendr / Isomapper -- not from the kernels -- plus the CPU-built scenes the CPU and the GPU tests
share.  The rasteriser's pix_to_face is an input (it has its own tests); without one every face counts as owning a pixel."""
import numpy as np

TIE = 1e-5            # two float64 cosines closer than this may be ordered the other way by the float32 product
ATLAS_MARGIN = 0.37   # texels; not a multiple of half a texel, so that no cell border of per_face_atlas runs through texel centres
ROUND_EPS = 1e-3      # a projection this close (px) to a rounding boundary may round the other way in float32


# ------------------------------------------------------------------ step 2
def texel_map(vt, ft, R):
    vt = np.asarray(vt, np.float64); ft = np.asarray(ft, np.int64)
    face = -np.ones((R, R), np.int64)
    bary = np.zeros((R, R, 3))
    for f in range(len(ft) - 1, -1, -1):                       # descending, overwriting: the lowest index wins
        t = ft[f]
        if (t < 0).any() or (t >= len(vt)).any():
            continue
        a, b, c = vt[t[0]], vt[t[1]], vt[t[2]]
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
        e0 = (c[0] - b[0]) * (v - b[1]) - (c[1] - b[1]) * (u - b[0])
        e1 = (a[0] - c[0]) * (v - c[1]) - (a[1] - c[1]) * (u - c[0])
        e2 = (b[0] - a[0]) * (v - a[1]) - (b[1] - a[1]) * (u - a[0])
        s = 1. if area2 > 0 else -1.
        inside = (s * e0 >= 0) & (s * e1 >= 0) & (s * e2 >= 0)
        face[rr[inside], cc[inside]] = f
        bary[rr[inside], cc[inside]] = np.stack([e0, e1, e2], -1)[inside] / area2
    return face, bary


# ------------------------------------------------------------------ steps 3-4
def vertex_normals(verts, faces):
    """corner cross products summed per vertex (faces with a -1 skipped), n / max(|n|, 1e-6) -- ops.vertex_normals' definition"""
    v = np.asarray(verts, np.float64)
    f = faces[(faces >= 0).all(1)]
    n = np.zeros_like(v)
    for k in range(3):
        a, b, c = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        np.add.at(n, a, np.cross(v[b] - v[a], v[c] - v[a]))
    return n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-6)


def project(verts, cam):
    """cameras.project: pixel (x, y), integer coordinates = pixel centres"""
    pc = np.asarray(verts, np.float64) @ cam["R"] + cam["T"]
    return np.stack([cam["c"][0] - pc[:, 0] * cam["f"][0] / pc[:, 2], cam["c"][1] - pc[:, 1] * cam["f"][1] / pc[:, 2]], -1)


def cam_pos(cam):
    return -cam["R"] @ cam["T"]


def in_mask(xy, mask):
    H, W = mask.shape
    rx, ry = np.round(xy[:, 0]), np.round(xy[:, 1])
    ok = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    out = np.zeros(len(xy), bool)
    out[ok] = mask[ry[ok].astype(int), rx[ok].astype(int)]
    return out


def rounding_unsafe(xy, mask):
    """vertices whose in-mask test could come out differently if the projection moved by ROUND_EPS px"""
    base = in_mask(xy, mask)
    bad = np.zeros(len(xy), bool)
    for dx in (-ROUND_EPS, ROUND_EPS):
        for dy in (-ROUND_EPS, ROUND_EPS):
            bad |= in_mask(xy + np.array([dx, dy]), mask) != base
    return bad


def bilinear(img, x, y):
    H, W = img.shape[:2]
    x, y = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx, wy = (x - x0)[:, None], (y - y0)[:, None]
    img = np.asarray(img, np.float64)
    return (img[y0, x0] * (1 - wx) + img[y0, x1] * wx) * (1 - wy) + (img[y1, x0] * (1 - wx) + img[y1, x1] * wx) * wy


# ------------------------------------------------------------------ steps 5-8
def new_slots(T, agg_num, normal_ang):
    cosv0 = np.cos(normal_ang / 180. * np.pi)
    return np.ones((T, agg_num)) * cosv0, np.full((T, agg_num, 3), np.nan), -np.ones((T, agg_num), np.int64), cosv0


def slot_update(normal_agg, tex_agg, view_agg, cosv, colour, fid):
    """step 6 for one view: where cosv > min(slots), the first slot holding the minimum takes (cosv, colour, fid)"""
    sel = cosv > normal_agg.min(1)
    where = normal_agg.argmin(1)                               # (argmin returns the first)
    i = np.nonzero(sel)[0]
    normal_agg[i, where[i]] = cosv[i]
    tex_agg[i, where[i]] = colour[i]
    view_agg[i, where[i]] = fid


def resolve_slots(normal_agg, tex_agg, view_agg, cosv0, check_num):
    """step 7: count, mask_final, view_id (-1 outside mask_final), median (0 outside mask_final)"""
    T = len(normal_agg)
    count = (normal_agg > cosv0).sum(1)
    fin = count >= check_num
    vid = view_agg[np.arange(T), normal_agg.argmax(1)]         # (argmax returns the first)
    vid[~fin] = -1
    med = np.zeros((T, 3))
    if fin.any():
        med[fin] = np.nanmedian(tex_agg[fin], axis=1)          # even count: mean of the two middle values
    return count, fin, vid, med


def bake(verts, faces, vt, ft, cam, images, masks, fids, R, agg_num=50, normal_ang=68., check_num=5, p2f=None, tmap=None):
    """verts [K,V,3] posed vertices, images [K,H,W,3], masks [K,H,W] bool, p2f [K,H,W] (face index per pixel, -1: none; None: every face
    owns a pixel).  Returns a dict of the [R,R] results plus, per covered texel, every view's cosine (`cos_all` [K,T]) and whether a
    vertex of its face sits on a rounding boundary in some view (`unsafe` [T])."""
    faces = np.asarray(faces, np.int64)
    face, bary = tmap if tmap is not None else texel_map(vt, ft, R)
    rr, cc = np.nonzero(face >= 0)
    tf, tb = face[rr, cc], bary[rr, cc]
    T, K = len(tf), len(verts)
    normal_agg, tex_agg, view_agg, cosv0 = new_slots(T, agg_num, normal_ang)
    cos_all = np.zeros((K, T))
    unsafe = np.zeros(T, bool)
    fv = faces[tf]                                             # (UV face i is mesh face i)
    whole = (faces >= 0).all(1)
    for k in range(K):
        p = np.asarray(verts[k], np.float64)
        xy = project(p, cam)
        owns = np.ones(len(faces), bool)
        if p2f is not None:
            owns[:] = False
            owns[p2f[k][p2f[k] >= 0]] = True
        vin = in_mask(xy, masks[k])
        visible = owns & whole & vin[faces].all(1)
        unsafe |= rounding_unsafe(xy, masks[k])[fv].any(1)
        d = p - cam_pos(cam)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        alpha = np.maximum((d * -vertex_normals(p, faces)).sum(1), 0.)
        cosv = (tb * alpha[fv]).sum(1) * visible[tf]
        pix = np.einsum("tk,tkj->tj", tb, xy[fv])
        colour = bilinear(images[k], pix[:, 0], pix[:, 1])
        cos_all[k] = cosv
        slot_update(normal_agg, tex_agg, view_agg, cosv, colour, fids[k])
    count, fin, vid, med = resolve_slots(normal_agg, tex_agg, view_agg, cosv0, check_num)
    out = {"tex_mask": face >= 0, "face": face, "bary": bary, "rows": rr, "cols": cc, "cos_all": cos_all, "unsafe": unsafe, "cosv0": cosv0,
           "slot_cos": normal_agg, "slot_rgb": tex_agg, "slot_view": view_agg}
    for name, val, fillv, dt in (("count", count, 0, np.int64), ("mask_final", fin, False, bool), ("view_id", vid, -1, np.int64)):
        g = np.full((R, R), fillv, dt)
        g[rr, cc] = val
        out[name] = g
    g = np.zeros((R, R, 3))
    g[rr, cc] = med
    out["tex_median"] = g
    return out


def excluded(res):
    """Per covered texel: ill-conditioned for a float32 comparison.  Candidates are the views whose cosine could enter the slots in either
    arithmetic (>= cosv0 - TIE; anything lower is rejected by both and its order is irrelevant): excluded where a candidate lies within TIE
    of cosv0 or of another candidate, or where a vertex of the texel's face sits on a rounding boundary of the in-mask test."""
    c = np.sort(res["cos_all"], axis=0)
    cand = c >= res["cosv0"] - TIE
    near0 = (cand & (np.abs(c - res["cosv0"]) <= TIE)).any(0)
    pair = (cand[1:] & cand[:-1] & (np.diff(c, axis=0) <= TIE)).any(0)
    return near0 | pair | res["unsafe"]


def dilate(mask, k):
    """square dilation, window i - k // 2 .. i - k // 2 + k - 1 on both axes (cv2.dilate's anchor); k = 0: unchanged"""
    if k <= 0:
        return mask.copy()
    R = mask.shape[0]
    out = mask.copy()
    for axis in (0, 1):
        src, out = out, np.zeros_like(mask)
        for off in range(-(k // 2), -(k // 2) + k):
            idx = np.arange(R) + off
            ok = (idx >= 0) & (idx < R)
            if axis == 0:
                out[ok] |= src[idx[ok]]
            else:
                out[:, ok] |= src[:, idx[ok]]
    return out


def _pull(coarse, n):
    """bilinear sample of `coarse` at the centres of an n x n grid twice as fine: 3/4 of the parent, 1/4 of the neighbour on the cell's
    own side, neighbours clamped at the border"""
    nc = coarse.shape[0]
    i = np.arange(n)
    p = i // 2
    q = np.clip(p + np.where(i % 2 == 1, 1, -1), 0, nc - 1)
    rows = 0.75 * coarse[p] + 0.25 * coarse[q]
    return 0.75 * rows[:, p] + 0.25 * rows[:, q]


def fill(tex_median, mask_final, tex_mask, k=None):
    """push-pull: known texels averaged down a 2x pyramid to 1 x 1 (a cell = mean of its known children), then unknown cells take the
    bilinear sample of the next coarser level; applied on dilate(tex_mask, k) - mask_final, mask_final untouched, 0 elsewhere"""
    R = tex_median.shape[0]
    k = int(0.1 * R) if k is None else k
    vals = [np.where(mask_final[..., None], np.asarray(tex_median, np.float64), 0.)]
    known = [mask_final.astype(np.float64)]
    while vals[-1].shape[0] > 1 or len(vals) == 1:
        v, w = vals[-1], known[-1]
        n = v.shape[0]
        m = (n + 1) // 2
        vp, wp = np.zeros((2 * m, 2 * m, 3)), np.zeros((2 * m, 2 * m))
        vp[:n, :n], wp[:n, :n] = v * w[..., None], w
        s = vp.reshape(m, 2, m, 2, 3).sum((1, 3)); ws = wp.reshape(m, 2, m, 2).sum((1, 3))
        vals.append(np.where(ws[..., None] > 0, s / np.maximum(ws, 1)[..., None], 0.))
        known.append((ws > 0).astype(np.float64))
        if m == 1:
            break
    for l in range(len(vals) - 2, -1, -1):
        up = _pull(vals[l + 1], vals[l].shape[0])
        vals[l] = np.where(known[l][..., None] > 0, vals[l], up)
    region = dilate(tex_mask, k) & ~mask_final
    out = np.zeros((R, R, 3))
    out[region] = vals[0][region]
    out[mask_final] = np.asarray(tex_median, np.float64)[mask_final]
    return out


# ------------------------------------------------------------------ scenes (built on the CPU; the GPU tests upload them)
def sequence_camera(H, W):
    """the camera of synthetic.SyntheticSequence(H, W)"""
    from selfreconcode_amd.synthetic import SyntheticSequence
    cp = SyntheticSequence(frame_num=4, H=H, W=W, device="cpu").camera_params
    q = cp["cam2world_coord_quat"].double().numpy()
    assert np.array_equal(q, [0., 0., 1., 0.])                                    # R = diag(-1, 1, -1)
    return {"f": cp["focal_length"].double().numpy(), "c": cp["princeple_points"].double().numpy(), "R": np.diag([-1., 1., -1.]),
            "T": cp["world2cam_coord_trans"].double().numpy()}


def smooth_image(H, W, phase):
    """a smooth analytic image in [0,1]: low-frequency sines (a period of at least 40 px), so bilinear sampling is well conditioned"""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ch = [0.5 + 0.4 * np.sin(2 * np.pi * (x / (40. + 9 * c) + y / (55. + 7 * c)) + phase + c) for c in range(3)]
    return np.stack(ch, -1).astype(np.float32)


def _rot_y(a):
    return np.array([[np.cos(a), 0., np.sin(a)], [0., 1., 0.], [-np.sin(a), 0., np.cos(a)]])


def _rot_x(a):
    return np.array([[1., 0., 0.], [0., np.cos(a), -np.sin(a)], [0., np.sin(a), np.cos(a)]])


def sphere_scene(K, angles_deg, H=128, R=256, levels=3):
    """An icosphere 'body' of radius 0.45 under the SyntheticSequence camera, turned about the vertical axis by angles_deg[k] (and tilted a
    little, differently per view) in view k; per_face_atlas UVs; a smooth image per view; a mask (a disc smaller than the body, without its
    top) that cuts part of the body off.  Everything float32 where the product takes float32."""
    from selfreconcode_amd.synthetic import icosphere, per_face_atlas
    v, f = icosphere(levels)
    v, f = v.double().numpy(), f.numpy()
    vt, ft = per_face_atlas(len(f), R, ATLAS_MARGIN)
    cam = sequence_camera(H, H)
    verts = []
    for k in range(K):
        M = _rot_x(np.deg2rad(7. * np.sin(1.3 * k + 0.4))) @ _rot_y(np.deg2rad(angles_deg[k]))
        verts.append((0.45 * v @ M.T + np.array([0.01 * k, -0.15 + 0.004 * k, 0.])).astype(np.float32))
    verts = np.stack(verts)
    images = np.stack([smooth_image(H, H, 0.7 * k) for k in range(K)])
    y, x = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    masks = np.stack([(y > 0.38 * H + 2 * np.sin(k)) & ((x - H / 2.) ** 2 + (y - H / 2.) ** 2 < (0.21 * H) ** 2) for k in range(K)])
    fids = np.arange(K) * 3 + 1
    return {"verts": verts, "faces": f, "vt": vt.numpy(), "ft": ft.numpy(), "cam": cam, "images": images, "masks": masks, "fids": fids, "H": H, "R": R}


def scene_a():
    """K = 8 views within +-40 degrees: with the defaults (agg_num 50) no slot is ever evicted"""
    return sphere_scene(8, np.linspace(-40., 40., 8))


SCENE_B = dict(agg_num=4, check_num=2, normal_ang=80.)


def scene_b():
    """K = 12 views 17 degrees apart, for agg_num = 4: a texel is seen well enough in up to eight of them, so slots are evicted"""
    return sphere_scene(12, np.arange(12) * 17. + 5.)


def hand_atlas():
    """UV triangles with a shared edge (0, 1), an overlap (2 lies over part of 0; the lower index keeps it), either winding, a degenerate
    face (3), a face with a -1 (4) and a small face that stands alone (5); no edge is aligned with the texel grid"""
    vt = np.array([[0.103, 0.131], [0.617, 0.127], [0.622, 0.583], [0.097, 0.611], [0.31, 0.22], [0.52, 0.47], [0.28, 0.49],
                   [0.7, 0.7], [0.8, 0.8], [0.9, 0.9], [0.71, 0.12], [0.93, 0.17], [0.83, 0.41]], np.float32)
    ft = np.array([[0, 1, 2], [0, 3, 2], [4, 5, 6], [7, 8, 9], [10, -1, 12], [10, 11, 12]], np.int64)
    return vt, ft
