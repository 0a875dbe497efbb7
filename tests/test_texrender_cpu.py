"""The textured renderer without a GPU: the mip layout, the float64 restatement's own properties (tests/_texrender_ref.py is what the
GPU tests compare the kernels with), turntable_vertices, the command's parser and the three entries on both sides of the ABI."""
import os
import re

import numpy as np
import pytest
import torch

import _texrender_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mip_layout():
    from selfreconcode_amd.render_ops import mip_layout
    assert mip_layout(1) == ([1], [0])
    assert mip_layout(2) == ([2, 1], [0, 4])
    assert mip_layout(5) == ([5, 3, 2, 1], [0, 25, 34, 38])
    sides, offsets = mip_layout(1680)
    assert sides == [1680, 840, 420, 210, 105, 53, 27, 14, 7, 4, 2, 1]
    assert offsets[0] == 0 and all(b - a == s * s for a, b, s in zip(offsets, offsets[1:], sides))
    for R in (1, 2, 5, 64, 257, 1680):
        assert mip_layout(R) == ref.layout(R)
    for R in (0, -3, 32769):
        with pytest.raises(ValueError):
            mip_layout(R)


def _one_face_frags(uv):
    """One image of P pixels in a row, all on face 0 whose UV corners are (0,0), (1,0), (0,1): barycentrics that give `uv` [P,2]."""
    uv = np.asarray(uv, np.float64)
    bary = np.stack([1. - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], -1)[None, None]
    return np.zeros((1, 1, uv.shape[0]), np.int64), bary, np.array([[0, 1, 2]]), np.array([[0., 0.], [1., 0.], [0., 1.]])


@pytest.mark.parametrize("holes", [False, True])
def test_reference_constant_texture_renders_constant_at_every_lod(holes):
    rng = np.random.default_rng(3)
    R = 13
    colour = np.array([0.2, 0.55, 0.9])
    tex = np.broadcast_to(colour, (R, R, 3)).copy()
    valid = rng.random((R, R)) < 0.7 if holes else None
    levels = ref.mips(tex, valid)
    assert [lv.shape[0] for lv in levels] == ref.layout(R)[0]
    p2f, bary, ft, vt = _one_face_frags(rng.random((400, 2)) * 1.4 - 0.2)           # some uv outside [0, 1]: clamp to edge
    for lod in np.linspace(0., len(levels) - 1., 9):
        rgba, cov, covered = ref.shade(p2f, bary, ft, vt, levels, np.full((1, 1), lod))
        seen = cov[0, 0] > 0
        assert covered.all() and seen.sum() > 100 and (holes or seen.all())
        np.testing.assert_allclose(rgba[0, 0, seen, :3], np.broadcast_to(colour, (seen.sum(), 3)), rtol=0, atol=1e-12)
        assert (rgba[0, 0, ~seen, :3] == 0.5).all() and (rgba[..., 3] == 1.).all()
        if not holes:
            np.testing.assert_allclose(cov, 1., rtol=0, atol=1e-12)


def test_reference_texel_centre_returns_the_texel():
    rng = np.random.default_rng(4)
    R = 6
    tex = rng.random((R, R, 3))
    levels = ref.mips(tex)
    r, c = np.meshgrid(np.arange(R), np.arange(R), indexing='ij')
    uv = np.stack([(c.ravel() + 0.5) / R, 1. - (r.ravel() + 0.5) / R], -1)         # sr_uv_rasterize's texel centres
    p2f, bary, ft, vt = _one_face_frags(uv)                                        # (barycentrics may leave [0, 1]: the blend is affine)
    rgba, cov, _ = ref.shade(p2f, bary, ft, vt, levels, np.zeros((1, 1)))
    np.testing.assert_allclose(rgba[0, 0, :, :3], tex.reshape(-1, 3), rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov, 1., rtol=0, atol=1e-12)


def test_reference_affine_texture_is_reproduced_by_level_0_inside():
    R = 16
    r, c = np.meshgrid(np.arange(R), np.arange(R), indexing='ij')
    u, v = (c + 0.5) / R, 1. - (r + 0.5) / R
    coef = np.array([[0.3, 0.2, 0.1], [0.1, -0.05, 0.4], [0.25, 0.3, 0.2]])        # rows: per channel (a, b, c) of a u + b v + c
    tex = np.stack([a * u + b * v + k for a, b, k in coef], -1)
    rng = np.random.default_rng(5)
    uv = rng.random((300, 2)) * (1. - 1. / R) + 0.5 / R                            # between the outermost texel centres
    p2f, bary, ft, vt = _one_face_frags(uv)
    rgba, _, _ = ref.shade(p2f, bary, ft, vt, ref.mips(tex), np.zeros((1, 1)))
    want = np.stack([a * uv[:, 0] + b * uv[:, 1] + k for a, b, k in coef], -1)
    np.testing.assert_allclose(rgba[0, 0, :, :3], want, rtol=0, atol=1e-12)


def test_reference_mips_average_the_in_range_children():
    tex = np.arange(75, dtype=np.float64).reshape(5, 5, 3)
    lv = ref.mips(tex)
    np.testing.assert_allclose(lv[1][0, 0, :3], tex[:2, :2].reshape(4, 3).mean(0))
    np.testing.assert_allclose(lv[1][2, 1, :3], tex[4, 2:4].mean(0))               # one row in range: two children
    np.testing.assert_allclose(lv[1][2, 2, :3], tex[4, 4])                         # the corner: one child
    np.testing.assert_allclose(lv[-1][0, 0, 3], 1.)
    u8 = ref.mips(np.full((2, 2, 3), 51, np.uint8), np.array([[1, 0], [0, 0]]))
    assert u8[0][0, 0, 0] == float(np.float32(51) / np.float32(255)) and u8[1][0, 0, 3] == 0.25


def test_reference_face_lod_of_a_scaled_triangle():
    vt = np.array([[0.1, 0.1], [0.6, 0.1], [0.1, 0.6]])
    xy = np.array([[[10., 10.], [74., 10.], [10., 42.]]])                          # 0.5 uv over 64 px in x, over 32 px in y
    lod = ref.face_lod(xy, np.array([[0, 1, 2]]), vt, np.array([[0, 1, 2]]), 1024, 0., 11)
    np.testing.assert_allclose(lod, [[np.log2(1024 * 0.5 / 32.)]], atol=1e-12)
    assert ref.face_lod(xy, np.array([[0, 1, 2]]), vt, np.array([[0, 1, 2]]), 1024, 20., 11)[0, 0] == 10.
    assert ref.face_lod(xy, np.array([[0, 1, 2]]), vt, np.array([[0, 1, 2]]), 1024, -20., 11)[0, 0] == 0.
    assert ref.face_lod(xy, np.array([[0, 1, 3]]), vt, np.array([[0, 1, 2]]), 1024, 0., 11)[0, 0] == 10.
    assert ref.face_lod(xy[:, [0, 1, 1]], np.array([[0, 1, 2]]), vt, np.array([[0, 1, 2]]), 1024, 0., 11)[0, 0] == 10.


def test_turntable_vertices():
    from selfreconcode_amd.render import turntable_vertices
    rng = np.random.default_rng(6)
    v = torch.from_numpy(rng.standard_normal((50, 3)).astype(np.float32))
    out = turntable_vertices(v, 4)
    assert out.shape == (4, 50, 3) and out.dtype == torch.float32 and torch.equal(out[0], v)
    want = ref.turntable_vertices(v.numpy(), 4)
    np.testing.assert_array_equal(want[0], v.numpy().astype(np.float64))
    np.testing.assert_allclose(out.numpy(), want, rtol=0, atol=1e-5)
    c = v.numpy().astype(np.float64).mean(0)
    d = v.numpy() - c
    np.testing.assert_allclose(want[1] - c, np.stack([d[:, 2], d[:, 1], -d[:, 0]], 1), atol=1e-12)      # a quarter turn: x takes z, z takes -x
    np.testing.assert_allclose(want[2] - c, np.stack([-d[:, 0], d[:, 1], -d[:, 2]], 1), atol=1e-12)     # a half turn: x takes -x
    unit = ref.turntable_vertices(np.array([[1., 0., 0.], [-1., 0., 0.]]), 4)                           # R_y's first column: (cos, 0, -sin)
    np.testing.assert_allclose(unit[:3, 0], [[1., 0., 0.], [0., 0., -1.], [-1., 0., 0.]], atol=1e-12)
    with pytest.raises(ValueError):
        turntable_vertices(v, 0)


def test_parser_defaults_and_flags():
    from selfreconcode_amd.render import build_parser
    a = build_parser().parse_args([])
    assert (a.gpu_ids, a.batch_size, a.rec_root, a.frames, a.turntable, a.turntable_frame, a.C, a.lod_bias) == ([0], 1, None, -1, 0, None, False, 0.)
    a = build_parser().parse_args(['--gpu-ids', '2', '--rec-root', 'x/result', '--frames', '7', '--batch-size', '4', '--turntable', '36',
                                   '--turntable-frame', '5', '--C', '--lod-bias', '-0.5'])
    assert (a.gpu_ids, a.batch_size, a.rec_root, a.frames, a.turntable, a.turntable_frame, a.C, a.lod_bias) == ([2], 4, 'x/result', 7, 36, 5, True, -0.5)


def test_render_main_needs_a_rec_root_and_the_texture_stage(tmp_path):
    from selfreconcode_amd import render
    with pytest.raises(SystemExit):
        render.main([])
    with pytest.raises(SystemExit, match='run the texture command first'):
        render.main(['--rec-root', str(tmp_path)])
    assert os.listdir(tmp_path) == []


def test_entries_are_declared_on_both_sides():
    from selfreconcode_amd import _lib
    txt = open(os.path.join(ROOT, "include", "selfrecon_hip.h")).read()
    for name in ("sr_texture_mips", "sr_texture_face_lod", "sr_shade_textured"):
        assert name in _lib.SIGNATURES and re.search(r"^int %s\(" % name, txt, flags=re.M), name
    assert _lib.abi_version() == 3


def test_operators_refuse_cpu_tensors():
    from selfreconcode_amd.render_ops import TextureMips, texture_face_lod, texture_mips
    with pytest.raises(RuntimeError):
        texture_mips(torch.zeros(4, 4, 3))
    mips = TextureMips(torch.zeros(22, 4), 4, 3)
    with pytest.raises(RuntimeError):
        texture_face_lod(torch.zeros(1, 3, 2), torch.tensor([[0, 1, 2]]), torch.zeros(3, 2), torch.tensor([[0, 1, 2]]), mips)
