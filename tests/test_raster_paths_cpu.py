"""The scenes of tests/_raster_scenes.py reach the launch paths of csrc/raster.hip they are built for, and the two references agree on
them: what keeps the GPU comparisons of tests/test_raster_paths_gpu.py honest.  No GPU is needed here.

References and the comparable set: tests/_raster_refs.py.  In every scene at most MAX_LEFT_OUT (1 %) of the pixels may fall outside the
comparable set; a scene that exceeds it has to change, not the cap."""
import numpy as np

import _raster_scenes as rs
from _raster_refs import MAX_LEFT_OUT, mesh_reference, mesh_scene, point_reference, point_scene
from oracle import raster_oracle as ro


def _report(kind, name, what, ref):
    print("%s %-14s %s; left out of the comparison %.4f %%" % (kind, name, what, 100 * ref["left_out"]))
    assert ref["left_out"] <= MAX_LEFT_OUT, ref["left_out"]


# ------------------------------------------------------------------------------------------------ point silhouette
def test_points_select_queue_has_more_queued_pixels_than_select_waves():
    """ps_select's wave-stride loop (raster.hip:149) runs a second time only with more than 2 048 queued pixels."""
    s, ref = point_scene("select_queue"), point_reference("select_queue", 2)
    over = int((ref["count"] > 2).sum())
    assert over > rs.SELECT_WAVES and over == 64 * 64
    _report("points", "select_queue", "%d pixels over K, largest coverage %d" % (over, ref["count"].max()), ref)
    assert (s["z"] > 0).all()


def test_points_deep_pixel_sits_on_the_resolve_boundary_with_ties_across_rank_k():
    """ps_resolve queues a pixel when n > K (raster.hip:105): K = 300 is n == K (not queued), K = 299 is n == K + 1 and drops exactly the
    farthest point; the bucket (300 keys) is longer than a wave; equal depths straddle the ranks 1, 64 and 299 and are split by index."""
    s = point_scene("deep_pixel")
    order, (row, col) = s["order"], rs.DEEP_PIXEL
    z = s["z"][0]
    assert len(rs.DEEP_TIES) * 2 == 20 and all(z[order[r]] == z[order[r + 1]] and order[r] < order[r + 1] for r in rs.DEEP_TIES)
    assert {0, 63, 298} <= set(rs.DEEP_TIES)                           # ranks K - 1 and K (0-based) tie for K = 1, 64, 299
    assert (np.diff(z[order]) >= 0).all() and rs.DEEP_N > 64
    for K in s["Ks"]:
        ref = point_reference("deep_pixel", K)
        n = (ref["idx"][0] >= 0).sum(-1)
        assert n[row, col] == min(K, rs.DEEP_N) and n.sum() == n[row, col]              # one covered pixel, the 5 points behind the camera not on it
        assert np.array_equal(ref["idx"][0, row, col, :min(K, rs.DEEP_N)], order[:K])   # the oracle's selection IS the (z, index) order
        _report("points", "deep_pixel", "K = %d keeps %d of %d, mask %.4f" % (K, n[row, col], rs.DEEP_N, ref["mask"][0, row, col]), ref)
    m = {K: point_reference("deep_pixel", K)["mask"][0, row, col] for K in s["Ks"]}
    assert m[300] - m[299] > 1e-3 and 0.5 < m[300] < 0.95              # the dropped point is visible in the mask, the composite is not saturated
    g299 = point_reference("deep_pixel", 299)["grad"][0]
    assert not g299[order[-1]].any() and np.abs(g299[order[:-1]]).min() > 0 and not g299[rs.DEEP_N:].any()


def test_points_second_pass_has_live_points_on_both_sides_of_the_capped_launch():
    """ps_accumulate, ps_gather and ps_backward (raster.hip:71, :121, :186) stop at 2 048 x 256 work items and stride on."""
    s, ref = point_scene("second_pass"), point_reference("second_pass", 8)
    live = np.nonzero(s["z"].ravel() >= 0)[0]
    assert s["z"].size > rs.STREAM_PASS and (live < rs.STREAM_PASS).sum() == 37 and (live >= rs.STREAM_PASS).sum() == 4098
    assert (s["z"][0] >= 0).any() and (live[live < rs.STREAM_PASS] >= s["z"].shape[1]).any()       # ... in both images before the boundary
    covered, over = int((ref["count"] > 0).sum()), int((ref["count"] > 8).sum())
    assert covered >= 5000 and over >= 2000
    assert (ref["count"][0] > 8).any() and (ref["count"][1] > 8).any()
    _report("points", "second_pass", "%d covered pixels, %d over K" % (covered, over), ref)


def test_points_many_pixels_queues_pixels_past_the_capped_launch():
    """ps_resolve (raster.hip:96) reaches pixels of flat index 524 288 and up only in its second grid-stride pass."""
    s, ref = point_scene("many_pixels"), point_reference("many_pixels", 4)
    flat = np.nonzero(((ref["count"] > 4) & ref["comparable"]).ravel())[0]          # queued pixels the GPU test does compare
    assert ref["count"].size > rs.STREAM_PASS and (flat >= rs.STREAM_PASS).sum() >= 100 and (flat < rs.STREAM_PASS).sum() >= 100
    _report("points", "many_pixels", "%d compared queued pixels, %d of them past flat index %d" % (flat.size, (flat >= rs.STREAM_PASS).sum(), rs.STREAM_PASS), ref)


def test_points_wide_discs_are_clamped_on_every_side_and_fit_the_layout():
    """point_box (raster.hip:40-41) clamps on all four sides; ps_layout (:218-219) sizes the buckets for boxes of 21 x 21 pixels."""
    s = point_scene("wide_discs")
    raw, clamped = rs.point_boxes(s["xy"][0], s["radius"], s["H"])
    side = rs.layout_box_side(s["radius"], s["H"])
    assert side == 21 and (raw[:, 1] - raw[:, 0] + 1).max() <= side and (raw[:, 3] - raw[:, 2] + 1).max() <= side
    assert (raw[:, 1] - raw[:, 0] + 1).max() >= side - 1                # the boxes do come within a pixel of the capacity
    assert all((raw[:, k] != clamped[:, k]).sum() >= 3 for k in range(4))
    outside = (np.abs(s["xy"][0]) > 1).any(1)
    assert outside.sum() == 12 and (np.abs(s["xy"][0]).max(1)[outside] < 1 + s["radius"]).all()
    for K in s["Ks"]:
        ref = point_reference("wide_discs", K)
        _report("points", "wide_discs", "K = %d: coverage up to %d, %d pixels over K" % (K, ref["count"].max(), (ref["count"] > K).sum()), ref)
    assert point_reference("wide_discs", 50)["count"].max() <= 50 and (point_reference("wide_discs", 5)["count"] > 5).mean() > 0.3


def test_points_largest_k_quantisation_stays_below_the_mask_tolerance():
    """ps_frac_bits(65 536) (raster.hip:57-62) leaves 21 fractional bits: a rounding of at most 2^-22 per term of log(1 - a)."""
    s, ref = point_scene("largest_k"), point_reference("largest_k", rs.LARGEST_K)
    ib = 1
    while (1 << (ib - 1)) <= 14 * rs.LARGEST_K:                         # ps_frac_bits, restated
        ib += 1
    assert 64 - 22 - ib == 21
    assert ref["count"].max() == rs.LARGEST_K_COVER                     # (the witness's count of covering points, not capped by K)
    assert rs.LARGEST_K_COVER * 2.0 ** -22 < 3.82e-6 < 3e-5             # 16 half steps; |d mask| <= |d log T|: well inside atol 3e-5
    _report("points", "largest_k", "%d points, coverage up to %d" % (s["z"].size, ref["count"].max()), ref)


# ------------------------------------------------------------------------------------------------ mesh rasteriser
def _boxes(s, n):
    w, h = rs.face_boxes(s["xy"][n], s["faces"], s["H"])
    return w, h, w * h


def test_mesh_queue_overflow_has_more_large_faces_than_the_queue_holds():
    """rm_pass1 queues at most N H W = 64 large faces (raster.hip:357-358); boxes of exactly RASTER_SMALL = 32 stay with their lane (:356)."""
    s, ref = mesh_scene("queue_overflow"), mesh_reference("queue_overflow")
    w, h, area = _boxes(s, 0)
    large = int((area > rs.RASTER_SMALL).sum())
    assert large > s["H"] * s["H"] and (area == rs.RASTER_SMALL).sum() >= 1 and ((area >= 33) & (area <= 40)).sum() >= 1
    winners = np.unique(ref["face"][ref["face"] >= 0])
    assert winners.size >= 20 and (area[winners] > rs.RASTER_SMALL).any() and (area[winners] <= rs.RASTER_SMALL).any()
    _report("mesh", "queue_overflow", "%d large faces for a queue of %d, %d boxes of exactly 32, %d of 33-40, %d distinct winners" % (
        large, s["H"] ** 2, (area == 32).sum(), ((area >= 33) & (area <= 40)).sum(), winners.size), ref)


def test_mesh_queue_batch_has_large_faces_of_both_orientations_in_every_image():
    """rm_pass1b decodes img = i / F, f = i % F (raster.hip:373) and walks rows or columns (:389)."""
    s, ref = mesh_scene("queue_batch"), mesh_reference("queue_batch")
    for n in range(3):
        w, h, area = _boxes(s, n)
        big = area > rs.RASTER_SMALL
        assert big.sum() >= 20 and (big & (h > w)).sum() >= 3 and (big & (w > h)).sum() >= 3
        assert (ref["face"][n] >= 0).mean() > 0.3
    assert sum(int((_boxes(s, n)[2] > rs.RASTER_SMALL).sum()) for n in range(3)) <= 3 * s["H"] ** 2          # no overflow here: every large face is queued
    assert not np.array_equal(ref["face"][0], ref["face"][1]) and not np.array_equal(ref["face"][1], ref["face"][2])
    _report("mesh", "queue_batch", "large faces per image %s" % [int((_boxes(s, n)[2] > 32).sum()) for n in range(3)], ref)


def test_mesh_second_pass_decodes_its_live_faces_past_the_capped_launch():
    """rm_pass1 (raster.hip:349-350) reaches work items 524 288 and up in its second pass; every other row falls to load_tri's rules."""
    s, ref = mesh_scene("second_pass"), mesh_reference("second_pass")
    F, faces, live = len(s["faces"]), s["faces"], s["live"]
    assert 2 * F > rs.STREAM_PASS and live.min() >= rs.MESH_SECOND_PASS_LIVE_FROM and F + live.min() >= rs.STREAM_PASS and live.size == 160
    dead = np.ones(F, bool); dead[live] = False
    neg = faces.min(1) < 0
    for n in range(2):
        zf = s["z"][n][np.where(neg[:, None], 0, faces)]
        t = s["xy"][n][np.where(neg[:, None], 0, faces)].astype(np.float64)
        area = (t[:, 0, 0] - t[:, 1, 0]) * (t[:, 2, 1] - t[:, 1, 1]) - (t[:, 0, 1] - t[:, 1, 1]) * (t[:, 2, 0] - t[:, 1, 0])
        behind, flat = zf.max(1) < 0, np.abs(area) <= 1e-8
        assert (neg | behind | flat)[dead].all() and not (neg | behind | flat)[live].any()
        assert neg.sum() > 1000 and (behind & ~neg).sum() > 1000 and (flat & ~neg & (area == 0)).sum() > 1000 and (flat & (area != 0)).sum() > 1000
        won = ref["face"][n][ref["face"][n] >= 0]
        assert np.isin(won, live).all() and np.unique(won).size >= 50 and (ref["face"][n] >= 0).mean() > 0.5
    assert not np.array_equal(ref["face"][0], ref["face"][1])
    # the large-face queue borrows pix_to_face[0 .. queued) and bary[0..1] (:446-448): empty, compared pixels lie inside that scratch,
    # pixel 0 (queue slot 0 and the counter) among them -- where the -1 fills of pass 2 show that the scratch was overwritten
    queued = sum(int((np.multiply(*rs.face_boxes(s["xy"][n], faces, s["H"]))[live] > rs.RASTER_SMALL).sum()) for n in range(2))
    scratch = ((ref["face"] < 0) & ref["comparable"]).ravel()[:queued]
    assert queued >= 200 and scratch[0] and scratch.sum() >= 5
    _report("mesh", "second_pass", "%d faces, live ones from %d, %d distinct winners in image 1" % (F, live.min(), np.unique(ref["face"][1]).size - 1), ref)


def test_mesh_many_pixels_covers_half_of_an_image_longer_than_the_capped_launch():
    """rm_pass2 (raster.hip:420, :425-426) reaches pixels of flat index 524 288 and up in its second pass."""
    s, ref = mesh_scene("many_pixels"), mesh_reference("many_pixels")
    cover = (ref["face"] >= 0).mean()
    assert ref["face"].size > rs.STREAM_PASS and cover >= 0.5
    tail = ref["face"].ravel()[rs.STREAM_PASS:]
    assert (tail >= 0).sum() > 100 and (tail < 0).sum() > 100           # covered and empty pixels in the second pass
    _report("mesh", "many_pixels", "%.1f %% covered" % (100 * cover), ref)


def _edge_area(xy, tri):
    t = xy[tri].astype(np.float32)                                       # load_tri's area, in float32
    return (t[0, 0] - t[1, 0]) * (t[2, 1] - t[1, 1]) - (t[0, 1] - t[1, 1]) * (t[2, 0] - t[1, 0])


def test_mesh_skip_rules_change_the_winner():
    """load_tri (raster.hip:289, :294, :296) and the |coordinate| < 8 rule (:355).  The reference here is the oracle WITHOUT the face that
    has a coordinate of 8.1: dropping it is the kernels' documented deviation from pytorch3d, which would draw it.

    Three rules can change a winner, and each is shown to: the -1 row (the face behind it would be drawn), the 8.1 face (the oracle draws
    it), and the area rule -- the tiny face (area 4.9e-9) contains a pixel centre and is dropped, the same face with area 1.1e-8 is drawn
    at that pixel.  That pixel is ambiguous to the witness (a nearly degenerate face), so it is held to the oracle alone.  The collinear
    face, the face behind the camera and the NaN face are rejected by the pixel test as well (strict b > 0, pz >= 0, NaN comparisons):
    no wrong early-out could draw them, they are in the scene to be survived."""
    s, ref = mesh_scene("skip_rules"), mesh_reference("skip_rules")
    k, face, H = rs.SKIP_FACES, ref["face"][0], s["H"]
    assert (face >= 0).all()                                             # the backdrop fills the image
    drawn = np.unique(face)
    assert set(drawn) == {k["backdrop"], k["inside_8"]} and (face == k["inside_8"]).sum() > 30
    verts = np.concatenate([s["xy"], s["z"][..., None]], -1)
    with_it = ro.rasterize_meshes(verts, s["faces"], H, H)[0][0, ..., 0]
    assert (with_it == k["beyond_8"]).sum() > 30                         # pytorch3d's arithmetic WOULD draw the 8.1 face: the deviation is visible
    plain = s["faces"].copy(); plain[k["minus_one"], 1] = 4              # the face behind the -1 row, had its index been read
    assert (ro.rasterize_meshes(verts, plain, H, H)[0] == k["minus_one"]).sum() > 30
    assert np.abs(s["xy"][0][s["faces"][k["inside_8"]]]).max() == np.float32(7.9) and np.abs(s["xy"][0][s["faces"][k["beyond_8"]]]).max() == np.float32(8.1)
    # the area rule, on both sides of 1e-8, at a pixel centre the face contains
    tiny, pix = s["faces"][k["tiny"]], rs.SKIP_TINY_PIXEL
    assert 4e-9 < _edge_area(s["xy"][0], tiny) < 6e-9 and face[pix] == k["backdrop"]
    w, h = rs.face_boxes(s["xy"][0], s["faces"], H)
    assert w[k["tiny"]] == 1 and h[k["tiny"]] == 1                       # its box is that one pixel: the rule, not an empty box, drops it
    above = rs.mesh_skip_rules(tiny_leg=1.05e-4)
    assert 1.0e-8 < _edge_area(above["xy"][0], tiny) < 1.2e-8
    drawn_above = ro.rasterize_meshes(np.concatenate([above["xy"], above["z"][..., None]], -1), above["faces_expected"], H, H)[0][0, ..., 0]
    assert drawn_above[pix] == k["tiny"] and (drawn_above == k["tiny"]).sum() == 1 and np.array_equal(drawn_above != k["tiny"], face == drawn_above)
    assert not ref["comparable"][0][pix] and (~ref["comparable"]).sum() == 1     # the witness leaves out exactly that pixel
    _report("mesh", "skip_rules", "drawn faces %s, tiny face dropped at pixel %s" % (drawn.tolist(), pix), ref)
