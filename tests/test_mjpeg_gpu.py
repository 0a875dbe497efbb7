"""JpegEncoder (selfreconcode_amd/video.py over csrc/mjpeg.hip) against the numpy restatement tests/_jpeg_ref.py: the arithmetic is
integer, so the comparison is byte for byte.  Sizes: one MCU, less than one, padding on one and both sides, ten MCU rows (the restart
counter wraps), and 129 MCUs in one row (774 blocks: more than three tiles of 256 in the entropy kernel's scans)."""
import math

import numpy as np
import pytest
import torch

import _jpeg_ref as jr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = ((16, 16), (1, 1), (8, 8), (17, 33), (40, 56), (147, 24), (16, 2064))          # H x W


def noise(h, w):
    return np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def white(h, w):
    return np.full((h, w, 3), 255, np.uint8)


def black(h, w):
    return np.zeros((h, w, 3), np.uint8)


def basis77(h, w):
    """Grey 128 + 100 cos((2x + 1) 7 pi / 16) cos((2y + 1) 7 pi / 16), tiled: of a whole luminance block only coefficient 63 survives
    quality 50 (F(7,7) = 400 against a divisor of 99; the rounding of the samples leaves every other |F| below half its divisor)."""
    c = [math.cos((2 * x + 1) * 7 * math.pi / 16) for x in range(8)]
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.array([[128 + int(round(100 * c[y] * c[x])) for x in range(8)] for y in range(8)], np.uint8)[yy % 8, xx % 8]
    return np.stack([g, g, g], axis=2)


def checker(h, w):
    """Saturated red / blue at 1-pixel pitch: every chroma sample is an average of two reds and two blues, luminance swings hard."""
    yy, xx = np.mgrid[0:h, 0:w]
    red = ((yy + xx) % 2 == 0)[..., None]
    return np.where(red, np.array([255, 0, 0], np.uint8), np.array([0, 0, 255], np.uint8)).astype(np.uint8)


def square4(h, w):
    """Black / white with the signs of cos((2x + 1) 4 pi / 16): at quality 100 coefficient (0, 4) is 1020, the largest an AC
    coefficient gets (category 10)."""
    _, xx = np.mgrid[0:h, 0:w]
    g = np.where(np.isin(xx % 8, (0, 3, 4, 7)), 255, 0).astype(np.uint8)
    return np.stack([g, g, g], axis=2)


def body(h, w):
    """The workload's kind of picture: a shaded, slightly textured figure on white."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = (xx + .5) / w * 2 - 1, (yy + .5) / h * 2 - 1
    inside = (u / .45) ** 2 + (v / .9) ** 2 < 1.
    shade = np.clip(.75 - .4 * u + .2 * v, 0., 1.)
    tex = np.random.default_rng(7).integers(-6, 7, (h, w))
    img = np.full((h, w, 3), 255, np.uint8)
    for c, base in enumerate((205, 160, 140)):
        img[..., c] = np.where(inside, np.clip(base * shade + tex, 0, 255), 255).astype(np.uint8)
    return img


CONTENTS = {"noise": (noise, 100), "white": (white, 90), "black": (black, 90), "basis77": (basis77, 50), "checker": (checker, 75), "square4": (square4, 100),
            "body": (body, 90)}
_REF = {}


def reference(name, h, w, stats=None):
    """The restatement's stream of one case, computed once per session and never modified."""
    key = (name, h, w)
    if key not in _REF or stats is not None:
        make, quality = CONTENTS[name]
        _REF[key] = jr.encode(make(h, w), quality, stats)
    return _REF[key]


def gpu_encode(img, quality):
    from selfreconcode_amd.video import JpegEncoder
    frames = torch.from_numpy(np.ascontiguousarray(img)).to(DEV)
    if frames.dim() == 3:
        frames = frames[None]
    return JpegEncoder(frames.shape[1], frames.shape[2], quality, DEV).encode(frames)


def _first_difference(a, b):
    n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return f"lengths {len(a)} / {len(b)}, first difference at byte {n}"


@pytest.mark.parametrize("name", list(CONTENTS))
def test_encoder_equals_the_restatement_byte_for_byte(name):
    make, quality = CONTENTS[name]
    for h, w in SIZES:
        want = reference(name, h, w)
        got = gpu_encode(make(h, w), quality)
        assert len(got) == 1 and got[0] == want, (name, h, w, _first_difference(got[0], want))


def test_the_cases_exercise_what_they_are_for():
    """On the restatement: noise at quality 100 stuffs bytes; white and black are DC and EOB only; a basis77 luminance block is three
    ZRL, one code and no EOB; square4 reaches the largest AC magnitude."""
    for h, w in SIZES[3:]:
        assert b"\xff\x00" in b"".join(jr.parse(reference("noise", h, w))[1])
    for name in ("white", "black"):
        stats = []
        reference(name, 40, 56, stats)
        assert stats and all(s == (0, 1) for s in stats)
    stats = []
    reference("basis77", 16, 16, stats)
    assert stats == [(3, 0)] * 4 + [(0, 1)] * 2
    Y = jr.planes(square4(16, 16))[0]
    assert max(jr.fdct_quant(Y[:8, :8], jr.dct_matrix(), [1] * 64)) == 1020
    _, intervals, rst = jr.parse(reference("noise", 147, 24))
    assert len(intervals) == 10 and rst == [0, 1, 2, 3, 4, 5, 6, 7, 0]


def test_a_batch_equals_single_encodes_and_repeats_exactly():
    from selfreconcode_amd.video import JpegEncoder
    h, w = 40, 56
    imgs = [noise(h, w), body(h, w), checker(h, w)]
    singles = [gpu_encode(img, 90)[0] for img in imgs]
    enc = JpegEncoder(h, w, 90, DEV)
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    batch = enc.encode(frames)                                             # (the workspace grows from 1 frame to 3 here)
    assert batch == singles and len(set(batch)) == 3
    assert enc.encode(frames) == batch
    assert enc.encode(frames[1:2]) == singles[1:2]
    assert [jr.encode(img, 90) for img in imgs[1:]] == singles[1:]


def test_encode_video_is_the_encoder_and_the_writer_together(tmp_path):
    import _avi
    from selfreconcode_amd.video import encode_video
    h, w = 17, 33
    imgs = [noise(h, w), body(h, w)] * 5                                   # ten frames: more than one batch of eight
    path = str(tmp_path / "clip.avi")
    assert encode_video(path, torch.from_numpy(np.stack(imgs)).to(DEV), fps=24., quality=75) == 10
    assert _avi.frames(path) == [gpu_encode(img, 75)[0] for img in imgs[:2]] * 5


def test_refusals():
    from selfreconcode_amd import video_ops
    from selfreconcode_amd.video import JpegEncoder
    enc = JpegEncoder(16, 16, 90, DEV)
    with pytest.raises(RuntimeError):
        enc.encode(torch.zeros((1, 16, 16, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        video_ops.jpeg_transform(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), enc.qtab)
    with pytest.raises(RuntimeError):
        JpegEncoder(16, 16, 90, "cpu")
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((1, 16, 16, 3), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device=DEV))
    for quality in (0, 101, -5):
        with pytest.raises(ValueError):
            JpegEncoder(16, 16, quality, DEV)
    with pytest.raises(ValueError):
        JpegEncoder(0, 16, 90, DEV)
    with pytest.raises(ValueError):
        JpegEncoder(16, 65536, 90, DEV)


def test_capacity_is_checked_before_anything_is_launched():
    """A workspace one frame too small is SR_ENOSPC on the host side: nothing is written past a buffer."""
    from selfreconcode_amd import _lib, video_ops
    from selfreconcode_amd.video import JpegEncoder
    enc = JpegEncoder(16, 16, 90, DEV)
    frames = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=DEV)
    coef = video_ops.jpeg_transform(frames, enc.qtab)
    ws = video_ops.JpegWorkspace(1, 16, 16, DEV)
    ws.B = 2                                                               # claims room for two, holds one
    with pytest.raises(_lib.SrError, match="SR_ENOSPC"):
        video_ops.jpeg_entropy(coef, 16, 16, enc.huff, ws)
    with pytest.raises(_lib.SrError, match="SR_ENOSPC"):
        video_ops.jpeg_gather(2, ws)
