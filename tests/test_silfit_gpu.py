"""The silhouette term on the GPU (csrc/silfit.hip behind ops.edt / contour_flags / silhouette_energy and smpl_fit) against its
restatement (tests/_silfit_ref.py).

The distance transform, the samples and the counts are integers: bit for bit.

Energy and gradient.  The GPU's match must lie within 1e-3 px of the restatement's minimum distance; the restatement is then evaluated
with the GPU's matches.  Bound: 4 x the error of the same formulas evaluated in float32 torch on the CPU against float64 (code that is
not under test).  An error is the largest absolute difference over an array divided by the array's largest float64 magnitude; the basis
of the bound is the largest such float32 ratio over the whole family of cases, because a case of one vertex or one sample holds a
single number whose float32 error lies by chance anywhere between zero and an ulp.  The inputs keep their float64 pixel fractions 1e-3
away from an integer, so that float32 and float64 agree on the cell; the test asserts that of every point.  Measured on an MI355X
(profiles/silhouette_fit.md): basis e_in 1.06e-6, e_cov 9.99e-6, g_in 4.87e-6, g_cov 5.62e-6; the GPU's largest ratios 1.06e-6,
3.55e-6, 5.26e-6, 4.07e-6.

The fit, from the float64 keypoint-only result with the arms blind: 11.96 px mean 2-D vertex error before the silhouette rounds,
6.85 px after them on the GPU, 6.86 px for the float64 restatement and 6.85 px for the float32 one.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import _silfit_ref as ref
import _smplfit_scene as base
from selfreconcode_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
EH, EW = 67, 70                                           # the canvas of the energy cases
FACTOR = 4.0


# ---------------------------------------------------------------------------------------------- distance transform
def _edt_cases():
    yy, xx = np.mgrid[0:67, 0:70]
    corner = np.zeros((1, 67, 70), np.uint8)
    corner[0, 66, 0] = 1
    wide = np.zeros((1, 3, 300), np.uint8)
    wide[0, 1, 7] = wide[0, 0, 290] = 1
    rng = np.random.RandomState(11)
    three = np.stack([rng.rand(37, 53) < 0.01, np.zeros((37, 53), bool), (xx[:37, :53] - 20) ** 2 + (yy[:37, :53] - 18) ** 2 <= 64]).astype(np.uint8)
    line = np.zeros((1, 1, 70), np.uint8)
    line[0, 0, 5] = line[0, 0, 60] = 1
    return {"1x1_set": np.ones((1, 1, 1), np.uint8), "1x1_unset": np.zeros((1, 1, 1), np.uint8), "1x70": line, "corner_67x70": corner,
            "all_set": np.ones((1, 67, 70), np.uint8), "none_set": np.zeros((1, 67, 70), np.uint8),
            "checkerboard": ((yy + xx) % 2 == 0).astype(np.uint8)[None], "row_of_300": wide, "three_frames": three}


@pytest.mark.parametrize("name", sorted(_edt_cases()))
def test_distance_transform_bit_equal(name):
    from selfreconcode_amd import smpl_fit as sf
    masks = _edt_cases()[name]
    want = ref.edt_two_pass(masks)
    if masks.shape[1] * masks.shape[2] <= 67 * 70:
        for f in range(masks.shape[0]):
            assert np.array_equal(want[f], ref.edt_brute(masks[f]))
    got = sf.distance_transform(torch.from_numpy(masks).to(DEV))
    assert got.dtype == torch.int32 and got.shape == masks.shape and got.is_cuda
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    if name == "none_set":
        assert (got == ops.EDT_EMPTY).all()
    if name == "corner_67x70":
        assert int(got.max()) == 66 * 66 + 69 * 69
    as_bool = sf.distance_transform(masks.astype(bool), device=DEV)               # host bool in, the same field out
    assert torch.equal(as_bool, got)


def test_distance_transform_of_a_scene_mask():
    s = ref.scene()
    got = ops.edt(torch.from_numpy(s["masks"][4:5]).to(DEV))
    assert np.array_equal(got.cpu().numpy().astype(np.int64), s["d2"][4:5])


def test_distance_transform_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError):
        ops.edt(torch.zeros((1, 2, 8193), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.edt(torch.zeros((2, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.edt(torch.zeros((1, 2, 8), dtype=torch.float32, device=DEV))


# ---------------------------------------------------------------------------------------------- contour samples
def _blobs(F, checker=False):
    yy, xx = np.mgrid[0:EH, 0:EW]
    masks = np.zeros((F, EH, EW), np.uint8)
    for t in range(F):
        if checker:
            masks[t] = ((yy + xx + t) % 2 == 0) & (yy >= 2) & (xx >= 3)
        else:
            masks[t] = ((xx - 22 - 5 * t) ** 2 + (yy - 25) ** 2 <= 81) | ((xx - 44) ** 2 + (yy - 40 + 3 * t) ** 2 <= 144) | ((xx >= 60) & (yy >= 50))
    return masks


def test_samples_and_counts_equal_the_restatement():
    from selfreconcode_amd import smpl_fit as sf
    masks = np.concatenate([_blobs(3), np.zeros((1, EH, EW), np.uint8), np.ones((1, EH, EW), np.uint8), _blobs(9, checker=True)[:7]])
    n = ref.contour_samples(masks, 1)[1]
    assert n[3] == 0 and n[4] == 0 and n[0] > 64 and n[5] > 2048
    flags = ops.contour_flags(torch.from_numpy(masks).to(DEV))
    assert np.array_equal(flags.cpu().numpy() != 0, ref.contour(masks))
    for S in (1, 64, int(n[0]), int(n[0]) + 1, 300, 2100, int(n[5]) - 1):          # n below, equal to and above S, F beyond one prefix-sum batch
        want_s, want_n = ref.contour_samples(masks, S)
        got_s, got_n = sf.contour_samples(torch.from_numpy(masks).to(DEV), S)
        assert got_s.dtype == torch.int32 and got_n.dtype == torch.int32 and got_s.shape == (masks.shape[0], S, 2)
        assert np.array_equal(got_n.cpu().numpy(), want_n), S
        assert np.array_equal(got_s.cpu().numpy(), want_s), S
    field = sf.silhouette_field(masks, 64, device=DEV)
    assert np.array_equal(field.d2.cpu().numpy().astype(np.int64), ref.edt_two_pass(masks)) and np.array_equal(field.counts.cpu().numpy(), n)


# ---------------------------------------------------------------------------------------------- energy and gradient
def _camera():
    from selfreconcode_amd import smpl_fit as sf
    return sf.make_camera(sf.quat_to_matrix([0.95, 0.1, -0.2, 0.15]), [0.1, -0.2, 0.3], 60., 55., 34.3, 33.1)


EXACT = {'R': np.eye(3), 'T': np.zeros(3), 'fx': 1., 'fy': 1., 'cx': 0., 'cy': 0.}          # p = (-x, -y, 1) projects to (x, y) exactly


def _points_at(xy, z, cam):
    """float32 world points whose projection under `cam` is xy [..,2] at depth z [..] (up to the rounding to float32)."""
    pc = np.stack([(cam['cx'] - xy[..., 0]) * z / cam['fx'], (cam['cy'] - xy[..., 1]) * z / cam['fy'], z], -1)
    return ((pc - cam['T']) @ cam['R'].T).astype(np.float32)


def _random_points(F, V, cam, seed):
    rng = np.random.RandomState(seed)
    xy = np.stack([rng.randint(0, EW - 1, (F, V)), rng.randint(0, EH - 1, (F, V))], -1) + rng.uniform(0.02, 0.98, (F, V, 2))
    return _points_at(xy, rng.uniform(2., 3., (F, V)), cam)


def _cells_agree(points, cam):
    """The condition on the inputs: every point that takes part has its float64 pixel fractions >= 1e-3 away from an integer or lies
    exactly on one (the special points); -> the number of points that would have to be left out (asserted to be 0)."""
    xy, front = ref.project(torch.from_numpy(points.astype(np.float64)), cam)
    xy = xy.numpy()[front.numpy()]
    frac = np.abs(xy - np.rint(xy))
    return int(((frac < 1e-3) & (frac != 0)).any(-1).sum())


def _case(V, F, S, checker=False, seed=0):
    masks = _blobs(F, checker)
    samples, counts = ref.contour_samples(masks, S)
    return {"points": _random_points(F, V, _camera(), 100 * V + 10 * F + S + seed), "d2": ref.edt_two_pass(masks), "samples": samples, "counts": counts,
            "camera": _camera(), "sigma": 20., "margin": 1.5}


def _special_case():
    """The exact camera.  Points on integer pixels, on x = W-1 and y = H-1, just outside the image, behind the camera, NaN; the rest random."""
    masks = _blobs(2)
    samples, counts = ref.contour_samples(masks, 64)
    rng = np.random.RandomState(5)
    V = 257
    xy = np.stack([rng.randint(0, EW - 1, (2, V)), rng.randint(0, EH - 1, (2, V))], -1) + rng.uniform(0.02, 0.98, (2, V, 2))
    z = rng.uniform(2., 3., (2, V))
    special = [(0, 0), (EW - 1, EH - 1), (EW - 1, 10), (12, EH - 1), (30, 30), (5, 60), (69, 0), (0, 66), (44, 40), (22, 25),
               (-0.0078125, 10), (10, -0.0078125), (EW - 1 + 0.0078125, 10), (10, EH - 1 + 0.0078125), (-3, -4), (200, 10)]
    for i, (a, b) in enumerate(special):
        xy[:, i] = (a, b)
        z[:, i] = 1.0
    points = _points_at(xy, z, EXACT)
    n = len(special)
    points[:, n] = (-10., -10., -1.)                      # behind the camera
    points[:, n + 1] = (-10., -10., 0.)                   # on the camera's plane
    points[:, n + 2] = (np.nan, 1., 1.)
    points[:, n + 3] = (1., 1., np.nan)
    points[1, n + 4] = (np.inf, 0., 1.)
    return {"points": points, "d2": ref.edt_two_pass(masks), "samples": samples, "counts": counts, "camera": EXACT, "sigma": 20., "margin": 1.5,
            "outside": 6 + 4 + (np.arange(2) == 1)}


FAMILY = [(V, F, S) for V in (1, 63, 200, 257) for F in (1, 3) for S in (1, 64, 300)]


def _ratios(got, want):
    """The four error ratios of (e_in, e_cov, g_in, g_cov) `got` against the float64 `want`."""
    out = []
    for g, w in zip(got, want):
        scale = float(np.abs(w).max())
        out.append(float(np.abs(np.asarray(g, np.float64) - w).max()) / scale if scale > 0 else float(np.abs(g).max()))
    return out


@functools.lru_cache(maxsize=None)
def _basis():
    """The largest float32-against-float64 ratio of each quantity over the family and the special case, on the CPU, with the
    restatement's own matches."""
    worst = np.zeros(4)
    for c in [_case(*k) for k in FAMILY] + [_special_case(), _case(1100, 1, 2100, checker=True)]:
        p64 = torch.from_numpy(c["points"].astype(np.float64))
        matches, _ = ref.match(p64, c["samples"], c["counts"], c["camera"])
        args = (c["d2"], c["samples"], c["counts"], matches, c["camera"], c["sigma"], c["margin"])
        w64 = ref.energy_and_gradient(c["points"].astype(np.float64), *args)
        w32 = ref.energy_and_gradient(c["points"], *args, dtype=torch.float32)
        worst = np.maximum(worst, _ratios([w32[0], w32[1], w32[3], w32[4]], [w64[0], w64[1], w64[3], w64[4]]))
    return worst


def _run(c):
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)          # noqa: E731
    args = (dev(c["points"], torch.float32), dev(c["d2"], torch.int32), dev(c["samples"], torch.int32), dev(c["counts"], torch.int32),
            _floats(c["camera"]), c["sigma"], c["margin"])
    first, second = ops.silhouette_energy(*args), ops.silhouette_energy(*args)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)      # equal bits
    return [t.cpu().numpy() for t in first]


def _floats(cam):
    from selfreconcode_amd import smpl_fit as sf
    return sf.camera_floats(cam)


def _check(c, label):
    assert _cells_agree(c["points"], c["camera"]) == 0                            # no point had to be left out for a cell switch
    e_in, e_cov, outside, g, gpu_match = _run(c)
    p64 = torch.from_numpy(c["points"].astype(np.float64))
    want_match, want_dist = ref.match(p64, c["samples"], c["counts"], c["camera"])
    assert np.array_equal(gpu_match >= 0, want_match >= 0)
    chosen = ref.distances_to(p64, c["samples"], gpu_match.astype(np.int64), c["camera"])
    used = want_match >= 0
    assert (chosen[used] <= want_dist[used] + 1e-3).all()
    w = ref.energy_and_gradient(c["points"].astype(np.float64), c["d2"], c["samples"], c["counts"], gpu_match.astype(np.int64), c["camera"], c["sigma"], c["margin"])
    assert np.array_equal(outside, w[2])
    got = _ratios([e_in, e_cov, g[0], g[1]], [w[0], w[1], w[3], w[4]])
    basis = _basis()
    print(f"{label}: error ratios e_in {got[0]:.2e} e_cov {got[1]:.2e} g_in {got[2]:.2e} g_cov {got[3]:.2e}; float32 basis " + " ".join(f"{b:.2e}" for b in basis))
    assert np.isfinite(g).all()
    for name, r, b in zip(("e_in", "e_cov", "g_in", "g_cov"), got, basis):
        assert r <= FACTOR * b, (label, name, r, b)
    return e_in, e_cov, outside, g, w


@pytest.mark.parametrize("V,F,S", FAMILY)
def test_energy_and_gradient_against_float64(V, F, S):
    c = _case(V, F, S)
    _, _, _, _, w = _check(c, f"V={V} F={F} S={S}")
    if V >= 63:
        assert w[0].min() > 0 and np.abs(w[3]).max() > 0                          # the case has work to do
    if V >= 63 and S >= 64:
        assert w[1].max() > 0 and np.abs(w[4]).max() > 0


def test_energy_beyond_one_tile_of_vertices_and_of_samples():
    c = _case(1100, 1, 2100, checker=True)
    assert c["counts"][0] > 2048                                                  # more than one LDS tile of samples, more than 1024 vertices
    _check(c, "V=1100 F=1 S=2100")


def test_energy_at_the_special_points():
    c = _special_case()
    e_in, e_cov, outside, g, w = _check(c, "special points")
    assert np.array_equal(outside, c["outside"])
    n = 16
    xy, front = ref.project(torch.from_numpy(c["points"].astype(np.float64)), EXACT)
    assert np.array_equal(xy.numpy()[:, :10], np.broadcast_to(np.array([(0, 0), (EW - 1, EH - 1), (EW - 1, 10), (12, EH - 1), (30, 30), (5, 60), (69, 0), (0, 66),
                                                                       (44, 40), (22, 25)], np.float64), (2, 10, 2)))      # exact
    assert (g[0][:, 10:n] == 0).all()                                             # off the image: no inside term
    assert (g[:, :, n:n + 4] == 0).all() and (g[:, 1, n + 4] == 0).all()          # behind, on the plane, NaN, inf: nothing at all
    assert not front.numpy()[:, n:n + 4].any()


def test_empty_and_full_frames_take_no_part():
    masks = np.stack([np.zeros((EH, EW), np.uint8), np.ones((EH, EW), np.uint8), _blobs(1)[0]])
    samples, counts = ref.contour_samples(masks, 64)
    c = {"points": _random_points(3, 63, _camera(), 77), "d2": ref.edt_two_pass(masks), "samples": samples, "counts": counts, "camera": _camera(),
         "sigma": 20., "margin": 1.5}
    e_in, e_cov, outside, g, _ = _check(c, "empty, full, blob")
    assert (e_in[:2] == 0).all() and (e_cov[:2] == 0).all() and (g[:, :2] == 0).all() and e_in[2] > 0 and (outside == 0).all()


def test_autograd_face_weights_the_two_gradients():
    from selfreconcode_amd import smpl_fit as sf
    c = _case(200, 3, 64)
    field = sf.SilhouetteField(torch.from_numpy(c["d2"]).to(DEV, torch.int32), torch.from_numpy(c["samples"]).to(DEV), torch.from_numpy(c["counts"]).to(DEV))
    p = torch.from_numpy(c["points"]).to(DEV).requires_grad_(True)
    e_in, e_cov, outside = sf.silhouette_energy(p, field, _floats(c["camera"]), c["sigma"], c["margin"])
    assert not outside.requires_grad and outside.dtype == torch.int32
    w_in = torch.tensor([2., 0., -1.], device=DEV)
    ((w_in * e_in).sum() + 3. * e_cov.sum()).backward()
    _, _, _, g, _ = ops.silhouette_energy(p.detach(), field.d2, field.samples, field.counts, _floats(c["camera"]), c["sigma"], c["margin"])
    assert torch.equal(p.grad, torch.addcmul(g[0] * w_in.view(3, 1, 1), g[1], torch.full((3, 1, 1), 3., device=DEV)))
    with pytest.raises(ValueError):
        ops.silhouette_energy(p.detach(), field.d2[:, :1], field.samples, field.counts, _floats(c["camera"]), 20., 1.5)      # H < 2


# ---------------------------------------------------------------------------------------------- the fit
def _smpl():
    from selfreconcode_amd.smpl_pytorch import DifferentiableSMPL
    return DifferentiableSMPL(base.model(), obj_saveable=True).to(DEV)


SIL = {"sigma": ref.SIGMA, "margin": ref.MARGIN, "samples": ref.SAMPLES}


def test_fit_with_masks_like_its_float64_restatement():
    from selfreconcode_amd import smpl_fit as sf
    s = ref.scene()
    start = ref.keypoint_fit()
    before = ref.vertex_error(ref._state(start["poses"], start["shape"], start["trans"]))
    want64 = ref.vertex_error(ref.silhouette_fit()[0])
    want32 = ref.vertex_error(ref.silhouette_fit(torch.float32)[0])
    smpl = _smpl()
    init = {k: np.asarray(v, np.float32) for k, v in start.items()}
    kwargs = dict(init=init, stages=base.STAGES[:1], masks=s["masks"], silhouette=SIL, silhouette_stages=ref.SIL_STAGES)
    got = sf.fit_sequence(smpl, s["keypoints"], s["camera"], **kwargs)
    iters = sum(st[0] for st in ref.SIL_STAGES)
    assert got["history"].shape == (iters,) and np.isfinite(got["history"]).all() and got["history"][-1] < got["history"][0]
    after = ref.vertex_error(ref._state(got["poses"], got["shape"], got["trans"]))
    slack = max(0.25, FACTOR * abs(want32 - want64))
    print(f"mean 2-D vertex error: before {before:.3f} px; after GPU {after:.3f}, float64 {want64:.3f}, float32 on the CPU {want32:.3f} px; slack {slack:.3f}")
    assert after <= 0.75 * before
    assert after <= want64 + slack
    for key in ("sil_inside", "sil_cover"):
        assert got[key].shape == (base.F,) and np.isfinite(got[key]).all() and (got[key] >= 0).all()
    assert got["sil_outside"].shape == (base.F,) and not got["sil_outside"].any() and got["sil_empty"] == 0 and got["mask_error"] is None      # (not square)
    again = sf.fit_sequence(smpl, s["keypoints"], s["camera"], **kwargs)
    for key in ("poses", "shape", "trans", "reproj", "history", "behind", "sil_inside", "sil_cover", "sil_outside"):
        assert np.array_equal(again[key], got[key]), key                          # bit for bit


def test_fit_without_masks_is_unchanged_and_the_rounds_come_last():
    from selfreconcode_amd import smpl_fit as sf
    s = ref.scene()
    smpl = _smpl()
    stages = ((4, 0.05, 0., 0., 100.), (3, 0.01, 1., 1., 10.))
    plain = sf.fit_sequence(smpl, s["keypoints"], s["camera"], stages=stages)
    none = sf.fit_sequence(smpl, s["keypoints"], s["camera"], stages=stages, masks=None, silhouette={"margin": 3.}, silhouette_stages=((5, 0.01, 1., 1., 1., 1., 1.),))
    assert set(plain) == set(none) == {"poses", "shape", "trans", "reproj", "behind", "history", "start", "gender"}
    for key in ("poses", "shape", "trans", "reproj", "behind", "history"):
        assert np.array_equal(plain[key], none[key]) and plain[key].dtype == none[key].dtype, key
    assert plain["start"] == none["start"] and plain["gender"] == none["gender"]
    masks = s["masks"].copy()
    masks[2] = 0                                          # a frame without a mask pixel is skipped and counted
    with_masks = sf.fit_sequence(smpl, s["keypoints"], s["camera"], stages=stages, masks=torch.from_numpy(masks.astype(bool)).to(DEV), silhouette=SIL,
                                 silhouette_stages=((5, 0.004, 0.1, 0.1, 1., 10., 25.), (2, 0.002, 0.1, 0.1, 1., 10., 25.)))
    n = plain["history"].shape[0]
    assert with_masks["history"].shape == (n + 7,) and np.array_equal(with_masks["history"][:n], plain["history"]) and np.isfinite(with_masks["history"]).all()
    assert with_masks["sil_empty"] == 1 and with_masks["sil_inside"][2] == 0 and with_masks["sil_cover"][2] == 0
    with pytest.raises(ValueError):
        sf.fit_sequence(smpl, s["keypoints"], s["camera"], stages=stages, masks=masks[:3])
    with pytest.raises(ValueError):
        sf.fit_sequence(smpl, s["keypoints"], s["camera"], stages=stages, masks=masks, silhouette={"radius": 2})


# ---------------------------------------------------------------------------------------------- the command
def test_the_command_with_masks(tmp_path):
    from PIL import Image
    from gen_smpl_golden import write_model_txt
    from selfreconcode_amd import fit_smpl, smpl_fit as sf
    from selfreconcode_amd.dataset.dataset import SceneDataset
    import _smplgrad_ref as gtwin
    folder = tmp_path / "scene"
    F, H, W = 3, 192, 192                                 # a square canvas: the report carries mask_error
    for sub in ("imgs", "masks"):
        (folder / sub).mkdir(parents=True)
    np.savez(folder / "camera.npz", fx=150., fy=150., cx=96., cy=80., quat=np.array([1., 0., 0., 0.]), T=np.zeros(3))
    for f in range(F):
        Image.fromarray(np.full((H, W, 3), 40 * f, np.uint8)).save(folder / "imgs" / f"{f}.png")
    models = tmp_path / "models"
    models.mkdir()
    write_model_txt(base.model(), str(models / "neutral_smpl_with_cocoplus_reg"))
    cam = sf.read_camera(folder / "camera.npz")
    assert fit_smpl.count_frames(str(folder)) == F
    poses = np.zeros((F, 24, 3))
    poses[:, 0] = sf.default_starts(cam)[1]
    trans = np.tile((np.array([0., 0., 2.2]) - cam['T']) @ cam['R'].T, (F, 1))
    m = gtwin.Model(base.model())
    out = gtwin.forward(m, torch.zeros((F, 10), dtype=torch.float64), torch.from_numpy(poses))
    x, y, z = gtwin.project(out["joints"] + torch.from_numpy(trans)[:, None], cam)
    vx, vy, vz = gtwin.project(out["verts"] + torch.from_numpy(trans)[:, None], cam)
    assert float(z.min()) > 1.0 and float(vz.min()) > 1.0
    assert float(vx.min()) >= 5 and float(vx.max()) <= W - 6 and float(vy.min()) >= 5 and float(vy.max()) <= H - 6
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(F):                                    # masks: discs of radius 5 round the projected vertices, written where the folder keeps its masks
        mask = np.zeros((H, W), bool)
        for a, b in zip(vx[f].numpy(), vy[f].numpy()):
            mask |= (xx - a) ** 2 + (yy - b) ** 2 <= 25
        Image.fromarray((mask * 255).astype(np.uint8)).save(folder / "masks" / f"{f}.png")
    np.savez(tmp_path / "kp.npz", keypoints=np.stack([x.numpy(), y.numpy(), np.ones((F, 19))], -1))
    lines = []
    argv = ["--gpu-ids", "0", "--data", str(folder), "--keypoints", str(tmp_path / "kp.npz"), "--model-dir", str(models), "--masks",
            "--sil-samples", "256", "--sil-margin", "5", "--sil-sigma", "20", "--sil-weights", "10", "25"]
    result = fit_smpl.main(argv, out=lines.append)
    print(lines[0])
    assert len(lines) == 1 and "silhouette inside" in lines[0] and "mask error" in lines[0]
    report = json.loads((folder / "smpl_fit.json").read_text())
    assert len(report["frames"]) == F
    for frame in report["frames"]:
        assert np.isfinite(frame["sil_inside"]) and np.isfinite(frame["sil_cover"]) and frame["sil_outside"] == 0
        assert 0.0 <= frame["mask_error"] <= 1.0
    assert 0.0 <= report["summary"]["mask_error_mean"] <= 1.0 and report["summary"]["sil_empty"] == 0
    assert np.array_equal(result["mask_error"], np.array([fr["mask_error"] for fr in report["frames"]], np.float32))
    ds = SceneDataset(str(folder), device=DEV)
    assert ds.frame_num == F and torch.equal(ds.poses.cpu(), torch.from_numpy(result["poses"])) and torch.equal(ds.trans.cpu(), torch.from_numpy(result["trans"]))
