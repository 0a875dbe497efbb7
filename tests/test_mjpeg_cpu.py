"""The Motion-JPEG pieces that need no GPU: the numpy restatement of the encoder (tests/_jpeg_ref.py) held to libjpeg through PIL, the
structure of its streams, the AVI writer walked by an independent RIFF reader, and the commands' parsers."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import _jpeg_ref as jr
from _avi import riff as _riff

H, W = 40, 56
QUALITIES = (50, 90, 100)
PSNR_MARGIN_DB = 0.05
LENGTH_MARGIN = 0.10


def _half_gradient_half_noise():
    img = np.zeros((H, W, 3), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    img[..., 0], img[..., 1], img[..., 2] = xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + yy) * 255 // (H + W - 2)
    img[:, W // 2:] = np.random.default_rng(0).integers(0, 256, (H, W - W // 2, 3))
    return img


def _psnr(a, b):
    return 10. * np.log10(255. ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def _tables(stream, marker):
    """{table id: bytes} of the DQT (0xDB) or DHT (0xC4) segments of a stream, however the tables are spread over segments."""
    out = {}
    for m, body in jr.parse(stream)[0]:
        pos = 0
        while m == marker and pos < len(body):
            n = 64 if marker == 0xDB else 16 + sum(body[pos + 1:pos + 17])
            out[body[pos]] = body[pos + 1:pos + 1 + n]
            pos += 1 + n
    return out


@pytest.mark.parametrize("quality", QUALITIES)
def test_restatement_against_libjpeg(quality):
    """Measured on the 40 x 56 half gradient, half noise image, restatement against PIL (libjpeg-turbo) at the same quality, 4:2:0,
    standard tables:
        quality    PSNR - PIL's PSNR    length - PIL's length - 3 bytes per MCU row
          50          -0.0018 dB            +114 bytes = 9.1 % of PIL's 1258
          90          +0.0026 dB            +171 bytes = 8.2 % of PIL's 2075
         100          -0.0027 dB            +194 bytes = 4.8 % of PIL's 4017
    The two round differently (tenths of a dB at most: here thousandths).  The length gap is not rounding: libjpeg codes the blocks
    that lie wholly in the padding (here the sixth row of luminance blocks, rows 40..47) as `dummy blocks` -- the previous DC and no AC
    -- while this encoder pads the picture by repeating its last row and codes what that gives, which under noise costs whole blocks;
    6 more bytes are headers (615 against 609: the DRI segment and one segment per table).  On a 48 x 64 picture of the same kind,
    which needs no padding, the same gap is +0.7 %, +0.4 % and -1.1 %.  Bounds: the measured gap plus a small allowance -- 0.05 dB, and 10 % of PIL's length."""
    img = _half_gradient_half_noise()
    mine = jr.encode(img, quality)
    decoded = Image.open(io.BytesIO(mine))
    decoded.load()
    assert decoded.size == (W, H) and decoded.mode == "RGB"
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    pil = buf.getvalue()
    assert _tables(mine, 0xDB) == _tables(pil, 0xDB)
    assert _tables(mine, 0xC4) == _tables(pil, 0xC4)
    gap_db = _psnr(np.asarray(decoded), img) - _psnr(np.asarray(Image.open(io.BytesIO(pil))), img)
    rows = (H + 15) // 16
    extra = len(mine) - len(pil) - 3 * rows
    print(f"quality {quality}: PSNR gap {gap_db:+.4f} dB, length {len(mine)} vs {len(pil)} (+{extra} beyond the restart overhead)")
    assert gap_db >= -PSNR_MARGIN_DB
    assert extra <= LENGTH_MARGIN * len(pil)


def test_stream_structure():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (147, 24, 3), dtype=np.uint8)              # 10 MCU rows of 2 MCUs: the restart counter wraps
    stream = jr.encode(img, 100)
    segs, intervals, rst = jr.parse(stream)
    assert [m for m, _ in segs] == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA, 0xD9]
    bodies = dict((m, b) for m, b in segs)
    assert struct.unpack(">H", bodies[0xDD])[0] == 2
    assert struct.unpack(">BHHB", bodies[0xC0][:6]) == (8, 147, 24, 3) and bodies[0xC0][6:] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert len(intervals) == 10 and rst == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    assert b"\xff\x00" in b"".join(intervals)
    for chunk in intervals:
        assert chunk and all(chunk[i + 1] == 0 for i in range(len(chunk) - 1) if chunk[i] == 0xFF) and chunk[-1] != 0xFF
    decoded = Image.open(io.BytesIO(stream))
    decoded.load()
    assert decoded.size == (24, 147)
    for h, w in ((1, 1), (8, 8), (17, 33)):
        s = jr.encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 90)
        sof = dict(jr.parse(s)[0])[0xC0]
        assert struct.unpack(">BHHB", sof[:6]) == (8, h, w, 3)
        assert Image.open(io.BytesIO(s)).size == (w, h)


def _check_avi(path, frames, w, h, fps):
    blob = open(path, "rb").read()
    avi = _riff(blob)
    avih = struct.unpack("<14I", avi["avih"])
    assert avih[0] == round(1e6 / fps) and avih[3] & 0x10 and avih[4] == len(frames) and avih[6] == 1 and avih[8:10] == (w, h)
    strh = struct.unpack("<4s4sIHHIIIIIIII4H", avi["strh"])
    assert strh[:2] == (b"vids", b"MJPG") and strh[7] / strh[6] == pytest.approx(fps) and strh[9] == len(frames) and strh[-2:] == (w, h)
    strf = struct.unpack("<IiiHH4sIiiII", avi["strf"])
    assert strf[:6] == (40, w, h, 1, 24, b"MJPG")
    assert [p for _, p in avi["movi"]] == list(frames)
    assert len(avi["idx1"]) == len(frames)
    movi = blob.index(b"movi")
    for (tag, flags, off, n), frame in zip(avi["idx1"], frames):
        assert tag == b"00dc" and flags & 0x10
        at = movi + off
        assert blob[at:at + 4] == b"00dc" and struct.unpack("<I", blob[at + 4:at + 8])[0] == n == len(frame) and blob[at + 8:at + 8 + n] == frame
        assert Image.open(io.BytesIO(frame)).size == (w, h)
    return avi


def test_avi_writer(tmp_path, monkeypatch):
    from selfreconcode_amd import video
    rng = np.random.default_rng(2)
    w, h = 24, 17
    frames = [jr.encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), q) for q in (30, 75, 100)]
    assert len({len(f) for f in frames}) == 3 and any(len(f) % 2 for f in frames)        # an odd length: the pad byte is exercised
    path = str(tmp_path / "three.avi")
    with video.MjpegWriter(path, w, h, fps=25.) as avi:
        for f in frames:
            avi.write(f)
    _check_avi(path, frames, w, h, 25.)
    empty = str(tmp_path / "empty.avi")
    video.MjpegWriter(empty, w, h).close()
    assert _check_avi(empty, [], w, h, 30.)["movi"] == []
    # the size guard: room for two of the three frames; the file is closed, valid, and the error says how many it holds
    guarded = str(tmp_path / "guarded.avi")
    two = len(open(path, "rb").read()) - (8 + len(frames[2]) + len(frames[2]) % 2) - 16
    monkeypatch.setattr(video, "AVI_MAX_BYTES", two + 20)
    writer = video.MjpegWriter(guarded, w, h, fps=25.)
    writer.write(frames[0])
    writer.write(frames[1])
    with pytest.raises(video.AviSizeError) as err:
        writer.write(frames[2])
    assert err.value.frames == 2 and "2 frames" in str(err.value)
    _check_avi(guarded, frames[:2], w, h, 25.)
    with pytest.raises(ValueError):
        writer.write(frames[0])


def test_headers_of_the_product_are_the_restatement_s():
    from selfreconcode_amd import video_ops
    for h, w, q in ((1, 1, 1), (40, 56, 50), (1080, 1920, 90), (65535, 65535, 100)):
        assert video_ops.jfif_headers(h, w, q) == jr.headers(h, w, q)
    for q in (0, 101, 50.5):
        with pytest.raises(ValueError):
            video_ops.quant_tables(q)


def test_parsers():
    from selfreconcode_amd import infer, render
    args = infer.parse_args(infer.build_parser(), ["--rec-root", "x", "--video", "--fps", "24", "--video-quality", "80", "--nI"])
    assert args.video and args.fps == 24. and args.video_quality == 80 and args.nI
    plain = infer.parse_args(infer.build_parser(), ["--rec-root", "x"])
    assert not plain.video and plain.fps == 30. and plain.video_quality == 90
    for bad in (["--video", "--nV"], ["--nI"], ["--nI", "--nV"], ["--video", "--video-quality", "0"]):
        with pytest.raises(SystemExit) as err:
            infer.parse_args(infer.build_parser(), ["--rec-root", "x"] + bad)
        assert err.value.code == 2
    args = render.build_parser().parse_args(["--rec-root", "x", "--video", "--fps", "12.5", "--video-quality", "70", "--turntable", "8"])
    assert args.video and args.fps == 12.5 and args.video_quality == 70 and args.turntable == 8
