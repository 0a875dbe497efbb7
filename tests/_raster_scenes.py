"""Scenes that drive every launch path of csrc/raster.hip (tests/test_raster_paths_cpu.py asserts that each scene reaches its path,
tests/test_raster_paths_gpu.py runs the kernels on it).  Pure numpy, deterministic from fixed default_rng seeds, square images only.

A point scene is a dict  name, path, H, xy [N,V,2] float32 (NDC), z [N,V] float32, radius, Ks (the points_per_pixel values to run).
A mesh scene is a dict   name, path, H, xy [N,V,2] float32, z [N,V] float32, faces [F,3] int64; `skip_rules` adds `faces_expected`,
the face list the references are given (see there).  `path` names the kernel lines the scene is for.

The two helpers at the end restate, in float32, the integer boxes the kernels derive (point_box, tri_box): the CPU tests use them to
assert which side of a launch threshold a primitive falls on."""
import numpy as np

STREAM_PASS = 2048 * 256          # work items one capped launch of sr_launch_stream covers before its grid-stride loop repeats
SELECT_WAVES = 512 * 4            # waves of the ps_select / rm_pass1b launches
RASTER_SMALL = 32                 # largest box (pixel centres) a lane of rm_pass1 rasterises itself


def centre(i, S):
    """NDC coordinate of pixel row / column i of an S-pixel side."""
    return 1.0 - (2.0 * i + 1.0) / S


# ------------------------------------------------------------------------------------------------ point silhouette
def points_select_queue():
    H, g = 64, np.random.default_rng(3)
    c = centre(np.arange(H), H)
    cx, cy = np.meshgrid(c, c)
    base = np.stack([cx.ravel(), cy.ravel()], -1)                              # [4096, 2]
    xy = (base[:, None, :] + g.uniform(-0.01, 0.01, (H * H, 3, 2))).reshape(1, -1, 2)
    z = g.uniform(1.0, 3.0, (1, H * H * 3))
    return dict(name="select_queue", path="ps_select wave-stride loop (raster.hip:149): more queued pixels than the launch has waves",
                H=H, xy=xy.astype(np.float32), z=z.astype(np.float32), radius=0.04, Ks=(2,))


DEEP_N, DEEP_PIXEL = 300, (11, 19)                                             # points on the pixel, its (row, col)
DEEP_TIES = (0, 10, 20, 30, 63, 100, 150, 200, 250, 298)                       # depth ranks r with z[r] == z[r + 1]: 20 points in pairs


def points_deep_pixel():
    """300 points on ONE pixel, each just inside the disc edge (alpha 0.002 .. 0.012, so that the composite of all 300 stays near
    0.88 and every single point is worth more than the mask tolerance), 10 equal-z pairs of which three straddle the ranks K = 1, 64
    and 299, and 5 points behind the camera on the same pixel.  -> also `order`: the point indices by (z, index)."""
    H, g = 32, np.random.default_rng(5)
    radius = 0.2 * 2.0 / H                                                     # 0.2 pixel: no other pixel centre is within reach
    n = DEEP_N
    alpha = g.uniform(0.002, 0.012, n)
    zs = np.linspace(1.0, 3.0, n)
    for r in DEEP_TIES:
        zs[r + 1] = zs[r]
    order = g.permutation(n)                                                   # order[r] = the point of depth rank r ...
    for r in DEEP_TIES:                                                        # ... with the lower index first inside a tie, as the oracle sorts
        lo, hi = sorted((order[r], order[r + 1]))
        order[r], order[r + 1] = lo, hi
        alpha[lo], alpha[hi] = 0.012, 0.002                                    # a swapped pair moves the mask by 0.01 T
    alpha[order[n - 2]], alpha[order[n - 1]] = 0.002, 0.012                    # the last pair: K = 299 drops the higher index, the weightier one
    z = np.empty(n); z[order] = zs
    ang = g.uniform(0, 2 * np.pi, n)
    rho = radius * np.sqrt(1.0 - alpha)
    row, col = DEEP_PIXEL
    xy = np.stack([centre(col, H) + rho * np.cos(ang), centre(row, H) + rho * np.sin(ang)], -1)
    back = np.stack([centre(col, H) + 0.3 * radius * np.cos(np.arange(5.0)), centre(row, H) + 0.3 * radius * np.sin(np.arange(5.0))], -1)
    xy = np.concatenate([xy, back])[None]; z = np.concatenate([z, -np.ones(5)])[None]
    return dict(name="deep_pixel", path="ps_resolve n == K / n == K + 1 (raster.hip:105), buckets longer than a wave and equal depths across "
                "rank K in ps_select (:155-170), the threshold test of ps_backward (:200)",
                H=H, xy=xy.astype(np.float32), z=z.astype(np.float32), radius=radius, Ks=(1, 64, 299, 300), order=order)


def points_second_pass():
    H, N, V, live, g = 96, 2, 264193, 4098, np.random.default_rng(7)
    assert N * V == STREAM_PASS + live
    xy = g.uniform(-1.02, 1.02, (N, V, 2))
    z = -np.ones((N, V))
    z[1, V - live:] = g.uniform(1.0, 3.0, live)                                # exactly the work items of the second pass
    a = g.choice(V, 20, replace=False)                                         # 37 live points of the first pass: a clump in image 0 ...
    xy[0, a] = g.normal(0.0, 0.03, (20, 2)) + (0.3, -0.2); z[0, a] = g.uniform(1.0, 3.0, 20)
    b = g.choice(V - live, 17, replace=False)                                  # ... and 17 spread over image 1
    z[1, b] = g.uniform(1.0, 3.0, 17)
    return dict(name="second_pass", path="second grid-stride pass of ps_accumulate (raster.hip:71), ps_gather (:121) and ps_backward (:186), "
                "and their i / V decode across work item 524 288",
                H=H, xy=xy.astype(np.float32), z=z.astype(np.float32), radius=0.05, Ks=(8,))


def points_many_pixels():
    H, g = 728, np.random.default_rng(9)
    xy = g.uniform(-1.0, 1.0, (3000, 2))
    clump = 600                                                                # rows 722-727, columns 100-139
    xy[:clump, 0] = g.uniform(centre(139.5, H), centre(99.5, H), clump)
    xy[:clump, 1] = g.uniform(centre(727.5, H), centre(721.5, H), clump)
    early = slice(clump, clump + 300)                                          # and a smaller clump on rows 100-105, queued in the first pass
    xy[early, 0] = g.uniform(centre(639.5, H), centre(599.5, H), 300)
    xy[early, 1] = g.uniform(centre(105.5, H), centre(99.5, H), 300)
    z = g.uniform(1.0, 3.0, 3000)
    z[-4:] = -1.0
    return dict(name="many_pixels", path="second grid-stride pass of ps_resolve (raster.hip:96): pixels, queued ones among them, past flat index 524 288",
                H=H, xy=xy[None].astype(np.float32), z=z[None].astype(np.float32), radius=0.006, Ks=(4,))


def points_wide_discs():
    H, g = 32, np.random.default_rng(13)
    xy = g.uniform(-0.95, 0.95, (40, 2))
    out = g.uniform(1.05, 1.45, 12)                                            # 12 centres outside the image, by less than the radius: 3 per side
    xy[0:3, 0] = out[0:3]; xy[3:6, 0] = -out[3:6]; xy[6:9, 1] = out[6:9]; xy[9:12, 1] = -out[9:12]
    z = g.uniform(1.0, 3.0, 40)
    z[20] = -1.0
    return dict(name="wide_discs", path="point_box clamps on all four sides (raster.hip:40-41) and the pairs-per-point capacity of ps_layout (:218-219)",
                H=H, xy=xy[None].astype(np.float32), z=z[None].astype(np.float32), radius=0.5, Ks=(50, 5))


LARGEST_K, LARGEST_K_COVER = 65536, 16


def points_largest_k():
    """A cloud thinned (highest point index first) until no pixel is covered by more than 16 points: with K = 65 536 the fixed-point
    step of ps_frac_bits is 2^-21 per term.  (With at most 16 covering points the K nearest of K = 65 536 are the K nearest of K = 16: the
    references are evaluated at LARGEST_K_COVER, whose per-pixel arrays fit; the kernels run at LARGEST_K.)"""
    H, g, radius = 64, np.random.default_rng(17), 0.04
    xy = g.uniform(-1.0, 1.0, (9000, 2)).astype(np.float32)
    z = g.uniform(1.0, 3.0, 9000).astype(np.float32)
    c = centre(np.arange(H), H)
    d2 = (c[None, None, :] - xy[:, 0, None, None]) ** 2 + (c[None, :, None] - xy[:, 1, None, None]) ** 2
    cov = (d2 < radius * radius * (1 + 1e-3)).reshape(len(xy), -1)             # (a hair generous: the float32 tests may differ at the rim)
    alive = np.ones(len(xy), bool)
    count = cov.sum(0)
    while count.max() > LARGEST_K_COVER:
        v = np.nonzero(cov[:, count.argmax()] & alive)[0][-1]
        alive[v] = False
        count -= cov[v]
    return dict(name="largest_k", path="ps_frac_bits at the largest admitted K (raster.hip:57-62, :238): 21 fractional bits",
                H=H, xy=xy[alive][None], z=z[alive][None], radius=radius, Ks=(LARGEST_K,))


POINT_SCENES = (points_select_queue, points_deep_pixel, points_second_pass, points_many_pixels, points_wide_discs, points_largest_k)


# ------------------------------------------------------------------------------------------------ mesh rasteriser
def _random_mesh(g, N, V, F, spread):
    xy = g.uniform(-spread, spread, (N, V, 2)).astype(np.float32)
    z = g.uniform(0.6, 3.0, (N, V)).astype(np.float32)
    faces = np.stack([g.choice(V, 3, replace=False) for _ in range(F)]).astype(np.int64)
    return xy, z, faces


def mesh_queue_overflow():
    H, g = 8, np.random.default_rng(11)
    xy, z, faces = _random_mesh(g, 1, 240, 240, 1.6)
    # constructed faces on both sides of RASTER_SMALL, should the random ones leave a side out: columns 1-4 x rows 0-7 (32) and columns 1-5 x rows 0-6 (35)
    ex = np.array([[centre(0.6, H), centre(-0.4, H)], [centre(4.4, H), centre(-0.4, H)], [centre(2.0, H), centre(7.4, H)],
                   [centre(0.6, H), centre(-0.4, H)], [centre(5.4, H), centre(-0.4, H)], [centre(2.0, H), centre(6.4, H)]], np.float32)
    xy = np.concatenate([xy, ex[None]], 1); z = np.concatenate([z, np.full((1, 6), 2.9, np.float32)], 1)
    faces = np.concatenate([faces, [[240, 241, 242], [243, 244, 245]]]).astype(np.int64)
    return dict(name="queue_overflow", path="overflow of the large-face queue (raster.hip:357-358: past N H W queued faces a lane rasterises its large "
                "face itself), both sides of RASTER_SMALL (:343, :356), the queue scratch in pix_to_face / bary[0..1] (:446-448)",
                H=H, xy=xy, z=z, faces=faces)


def mesh_queue_batch():
    H, g = 16, np.random.default_rng(19)
    xy, z, faces = _random_mesh(g, 3, 240, 240, 1.6)
    return dict(name="queue_batch", path="the i / F, i % F decode of queued faces of several images and both line orientations of rm_pass1b (raster.hip:373, :389)",
                H=H, xy=xy, z=z, faces=faces)


MESH_SECOND_PASS_LIVE_FROM = 260000


def mesh_second_pass():
    """Every face row falls to a face-level skip rule (a -1 index; zero or tiny area; all three vertices behind the camera) except 160
    live faces at indices >= 260 000: in image 1 those are work items 530 000 and up, past the first pass of rm_pass1."""
    H, N, F, g = 64, 2, 270000, np.random.default_rng(23)
    xy = g.uniform(-1.2, 1.2, (N, 400, 2)); z = g.uniform(0.6, 3.0, (N, 400))
    behind_xy = g.uniform(-0.9, 0.9, (N, 6, 2)); behind_z = -g.uniform(0.5, 2.0, (N, 6))          # vertices 400-405
    b = 1.0 - 2.0 * 20 / H                                                                       # a pixel BOUNDARY: no pixel centre near the tiny face
    tiny_xy = np.broadcast_to(np.array([[b, b], [b + 1e-5, b], [b, b + 1e-4]]), (N, 3, 2)); tiny_z = np.full((N, 3), 1.0)   # vertices 406-408, area 1e-9
    xy = np.concatenate([xy, behind_xy, tiny_xy], 1); z = np.concatenate([z, behind_z, tiny_z], 1)
    faces = g.integers(0, 400, (F, 3))
    rule = g.choice(4, F, p=[0.9, 0.04, 0.04, 0.02])
    neg = rule == 0
    faces[neg, g.integers(0, 3, int(neg.sum()))] = -1                                            # one -1 among valid indices
    faces[rule == 1] = g.integers(400, 406, (int((rule == 1).sum()), 3))                         # behind the camera
    same = rule == 2
    faces[same] = faces[same][:, :1]                                                             # (a, a, a): area exactly 0
    faces[rule == 3] = (406, 407, 408)                                                           # area 1e-9
    live = MESH_SECOND_PASS_LIVE_FROM + np.sort(g.choice(F - MESH_SECOND_PASS_LIVE_FROM, 160, replace=False))
    faces[live] = np.stack([g.choice(400, 3, replace=False) for _ in range(160)])
    return dict(name="second_pass", path="second grid-stride pass of rm_pass1 (raster.hip:349) and its i / F, i % F decode (:350) across work item 524 288; "
                "the face-level skip rules of load_tri (:289, :294, :296)",
                H=H, xy=xy.astype(np.float32), z=z.astype(np.float32), faces=faces.astype(np.int64), live=live)


def mesh_many_pixels():
    H, g = 728, np.random.default_rng(29)
    xy, z, faces = _random_mesh(g, 1, 90, 60, 1.6)
    return dict(name="many_pixels", path="second grid-stride pass of rm_pass2 (raster.hip:420) and its pixel decode (:425-426) past flat index 524 288",
                H=H, xy=xy * np.float32(0.8), z=z, faces=faces)


SKIP_FACES = dict(backdrop=0, minus_one=1, collinear=2, tiny=3, behind=4, nan=5, inside_8=6, beyond_8=7)
SKIP_TINY_PIXEL = (20, 30)                                                     # (row, col) whose centre the tiny face contains
SKIP_TINY_LEG = 7e-5                                                           # legs of the tiny right triangle: edge-function area 4.9e-9


def mesh_skip_rules(tiny_leg=SKIP_TINY_LEG):
    """One face per skip rule, each nearer than a backdrop face that fills the image.  `faces_expected` is what the references are given:
    the same list with the face that has a coordinate of 8.1 replaced by a -1 row -- the kernels drop a face with any |x| or |y| >= 8
    (raster.hip:355), pytorch3d and its restatement do not.

    Which rules can change a winner.  The -1 row, the 8.1 face and the tiny face can: behind each is a face the later pixel test would
    accept.  The tiny face (area 4.9e-9, inside the +-1e-8 rule) CONTAINS the centre of pixel SKIP_TINY_PIXEL; without the rule face_hit
    would accept it there (its denominator is area + 1e-8, so the weights stay positive), and with `tiny_leg` 1.05e-4 (area 1.1e-8, just
    outside the rule) it is drawn.  The collinear face, the face behind the camera and the NaN face are rejected again by the pixel
    test whatever the early-out does (strict b > 0, pz >= 0, NaN comparisons): they are here to be survived, they pin no threshold."""
    H = 48
    nan = np.nan
    b = 1.0 - 2.0 * 30 / H                                                     # a pixel boundary
    ty, tx = centre(SKIP_TINY_PIXEL[0], H) - 0.3 * tiny_leg, centre(SKIP_TINY_PIXEL[1], H) - 0.3 * tiny_leg
    v = [(-7.0, -6.0, 3.0), (7.5, -6.0, 3.0), (0.0, 7.5, 3.0),                 # 0-2   backdrop, all of the image, z = 3
         (-0.9, 0.5, 1.0), (-0.5, 0.5, 1.0), (-0.7, 0.9, 1.0),                 # 3-5   a plain near face; listed with a -1 index
         (-0.6, b, 1.0), (0.0, b, 1.0), (0.6, b, 1.0),                         # 6-8   collinear along a pixel boundary: area 0
         (tx, ty, 1.0), (tx, ty + tiny_leg, 1.0), (tx + tiny_leg, ty, 1.0),    # 9-11  area +tiny_leg^2 around a pixel centre
         (0.1, 0.1, -1.0), (0.6, 0.1, -2.0), (0.3, 0.6, -1.5),                 # 12-14 entirely behind the camera
         (nan, -0.2, 1.0), (0.5, -0.2, 1.0), (0.3, -0.7, 1.0),                 # 15-17 a NaN coordinate
         (7.9, -0.9, 1.2), (-0.1, -0.3, 1.2), (-0.1, -0.9, 1.2),               # 18-20 a coordinate of 7.9: drawn
         (0.3, 8.1, 1.4), (0.1, 0.2, 1.4), (0.6, 0.2, 1.4)]                    # 21-23 a coordinate of 8.1: skipped by the kernels
    v = np.asarray(v, np.float32)
    faces = np.array([(0, 1, 2), (3, -1, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (15, 16, 17), (18, 19, 20), (21, 22, 23)], np.int64)
    expected = faces.copy(); expected[SKIP_FACES["beyond_8"]] = -1
    return dict(name="skip_rules", path="the skip rules: -1 index (raster.hip:289), face behind the camera (:294), area within +-1e-8 and NaN (:296), "
                "NaN or |coordinate| >= 8 (:355)",
                H=H, xy=v[None, :, :2].copy(), z=v[None, :, 2].copy(), faces=faces, faces_expected=expected)


MESH_SCENES = (mesh_queue_overflow, mesh_queue_batch, mesh_second_pass, mesh_many_pixels, mesh_skip_rules)


# ------------------------------------------------------------------------------------------------ the kernels' integer boxes, restated
def point_boxes(xy, radius, H):
    """point_box of raster.hip before and after its clamps: (c0, c1, r0, r1) unclamped, and the same clamped to the image."""
    f = np.float32
    cc = ((f(1) - xy[..., 0]) * f(H) - f(1)) * f(0.5); rc = ((f(1) - xy[..., 1]) * f(H) - f(1)) * f(0.5)
    rx = f(radius) * f(H) * f(0.5)
    raw = np.stack([np.floor(cc - rx) - 1, np.ceil(cc + rx) + 1, np.floor(rc - rx) - 1, np.ceil(rc + rx) + 1], -1).astype(np.int64)
    lo, hi = np.array([0, -10 ** 9, 0, -10 ** 9]), np.array([10 ** 9, H - 1, 10 ** 9, H - 1])
    return raw, np.minimum(np.maximum(raw, lo), hi)


def layout_box_side(radius, H):
    """The side of the per-point pixel box ps_layout sizes the buckets for."""
    return int(np.ceil(np.float32(radius) * np.float32(H) * np.float32(0.5))) * 2 + 5


def face_boxes(xy, faces, H):
    """tri_box of raster.hip for one image: (width, height) in pixel centres of every face, 0 where the box is empty or an index is -1."""
    f = np.float32
    ok = faces.min(1) >= 0
    t = xy[np.where(ok[:, None], faces, 0)].astype(f)                          # [F,3,2]
    with np.errstate(invalid="ignore"):
        lo, hi = np.fmin.reduce(t, 1), np.fmax.reduce(t, 1)                    # fminf / fmaxf: a NaN loses
        a = np.ceil(((f(1) - hi) * f(H) - f(1)) * f(0.5) - f(1e-3)); b = np.floor(((f(1) - lo) * f(H) - f(1)) * f(0.5) + f(1e-3))
        a, b = np.maximum(a, 0), np.minimum(b, H - 1)
        wh = np.where(ok[:, None] & np.isfinite(a) & np.isfinite(b), np.maximum(b - a + 1, 0), 0).astype(np.int64)
    return wh[:, 0], wh[:, 1]
