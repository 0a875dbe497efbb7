"""Operators of the Motion-JPEG encoder (csrc/mjpeg.hip): GPU tensors only, no autograd.  `video.py` is the public
interface.  The tables of ITU-T T.81 Annex K live here once: the DQT / DHT segments and the kernels' tables come from the same arrays."""
import struct

import torch

from . import _lib

BLOCK_BYTES = _lib.SR_JPEG_BLOCK_BYTES   # the code of one block before stuffing, worst case

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# Annex K.1, K.2 (natural order)
QUANT_LUMINANCE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
QUANT_CHROMINANCE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Annex K.3: (BITS, HUFFVAL)
DC_LUMINANCE = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMINANCE = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMINANCE = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
AC_CHROMINANCE = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
HUFFMAN = ((0x00, DC_LUMINANCE), (0x10, AC_LUMINANCE), (0x01, DC_CHROMINANCE), (0x11, AC_CHROMINANCE))     # (Tc << 4 | Th, table), DHT order


def jpeg_quality(quality):
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"JPEG quality must be an integer in [1, 100], got {quality!r}")
    return int(quality)


def quant_tables(quality):
    """(luminance, chrominance) divisors in natural order: the Annex K tables under the IJG scaling -- scale = 5000 // q below 50,
    200 - 2 q from 50 on, entry (base * scale + 50) // 100 clamped to [1, 255]."""
    q = jpeg_quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(max((b * scale + 50) // 100, 1), 255) for b in base) for base in (QUANT_LUMINANCE, QUANT_CHROMINANCE))


def huffman_codes(bits, vals):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) table (T.81 Annex C)."""
    out, code, i = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[i]] = (code, length)
            code, i = code + 1, i + 1
        code <<= 1
    return out


def device_tables(quality, device):
    """(qtab [2,64] int16 holding the divisors in zigzag order, huff [4,256] int32 holding code | length << 16 for the DC luminance, DC
    chrominance, AC luminance and AC chrominance tables) as sr_jpeg_transform / sr_jpeg_entropy read them."""
    qtab = torch.tensor([[t[n] for n in ZIGZAG] for t in quant_tables(quality)], dtype=torch.int16, device=device)
    rows = []
    for table in (DC_LUMINANCE, DC_CHROMINANCE, AC_LUMINANCE, AC_CHROMINANCE):
        row = [0] * 256
        for sym, (code, length) in huffman_codes(*table).items():
            row[sym] = code | length << 16
        rows.append(row)
    return qtab, torch.tensor(rows, dtype=torch.int32, device=device)


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def jfif_headers(H, W, quality):
    """SOI, APP0 (JFIF 1.1, no density), DQT x 2, SOF0, DHT x 4, DRI (one MCU row) and SOS: everything in front of the scan data."""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, bytes([0]) + bytes(ql[n] for n in ZIGZAG)) + _segment(0xDB, bytes([1]) + bytes(qc[n] for n in ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tcth, (bits, vals) in HUFFMAN:
        out += _segment(0xC4, bytes([tcth]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", (W + 15) // 16))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def geometry(H, W):
    """(R, M): MCU rows and MCUs per row of an H x W picture."""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"JPEG: H and W must lie in [1, 65535], got {H} x {W}")
    return (H + 15) // 16, (W + 15) // 16


def capacities(B, H, W):
    """(coef int16 elements, bits dwords, rowbuf bytes, out bytes) that hold B frames of H x W whatever they show: a block's code is
    at most BLOCK_BYTES before stuffing and twice that after it."""
    R, M = geometry(H, W)
    bits_stride = (6 * M * BLOCK_BYTES // 4 + 31) // 32 * 32
    row_stride = 12 * M * BLOCK_BYTES
    return B * R * M * 384, B * R * bits_stride, B * R * row_stride, B * (R * row_stride + 2 * (R - 1))


def frames_u8(frames, what):
    _lib.require_gpu(frames)
    if frames.dtype != torch.uint8:
        raise ValueError(f"{what}: uint8 frames expected, got {frames.dtype}")
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] == 0:
        raise ValueError(f"{what}: frames [B,H,W,3] expected, got {tuple(frames.shape)}")
    return frames.detach().contiguous()


def jpeg_transform(frames, qtab):
    """coef [B, R M, 6, 64] int16 (sr_jpeg_transform): the quantised DCT coefficients of frames [B,H,W,3] uint8 (RGB), per MCU the
    blocks Y00 Y01 Y10 Y11 Cb Cr, each in zigzag order."""
    frames = frames_u8(frames, "jpeg_transform")
    _lib.require_gpu(qtab)
    B, H, W = frames.shape[:3]
    R, M = geometry(H, W)
    if B > 65535 or tuple(qtab.shape) != (2, 64) or qtab.dtype != torch.int16:
        raise ValueError(f"jpeg_transform: at most 65535 frames and qtab [2,64] int16, got {B} and {tuple(qtab.shape)} {qtab.dtype}")
    coef = torch.empty((B, R * M, 6, 64), dtype=torch.int16, device=frames.device)
    _lib.launch("sr_jpeg_transform", frames, frames, B, H, W, qtab.contiguous(), coef)
    return coef


class JpegWorkspace:
    """The buffers of sr_jpeg_entropy / sr_jpeg_gather for up to B frames of H x W, sized by `capacities`."""

    def __init__(self, B, H, W, device):
        self.B, self.H, self.W = int(B), int(H), int(W)
        self.R, self.M = geometry(H, W)
        _, nbits, nrow, nout = capacities(self.B, H, W)
        buf = torch.empty((nbits + 64,), dtype=torch.int32, device=device)                    # (bits: 128-byte aligned)
        off = (-buf.data_ptr()) % 256 // 4
        self.bits = buf[off:off + nbits]
        self.rowbuf = torch.empty((nrow,), dtype=torch.uint8, device=device)
        self.row_len = torch.empty((self.B * self.R,), dtype=torch.int32, device=device)
        self.row_start = torch.empty((self.B * self.R,), dtype=torch.int64, device=device)
        self.out = torch.empty((nout,), dtype=torch.uint8, device=device)
        self.offsets = torch.empty((self.B + 1,), dtype=torch.int64, device=device)


def jpeg_entropy(coef, H, W, huff, ws):
    """Codes the intervals of coef [B, R M, 6, 64] into ws.rowbuf / ws.row_len (sr_jpeg_entropy)."""
    _lib.require_gpu(coef, huff)
    B = coef.shape[0]
    R, M = geometry(H, W)
    if coef.dtype != torch.int16 or tuple(coef.shape) != (B, R * M, 6, 64) or not coef.is_contiguous() or not 1 <= B <= ws.B or (ws.H, ws.W) != (H, W):
        raise ValueError(f"jpeg_entropy: coef {tuple(coef.shape)} {coef.dtype} for {H} x {W} and a workspace of {ws.B} x {ws.H} x {ws.W}")
    if tuple(huff.shape) != (4, 256) or huff.dtype != torch.int32:
        raise ValueError(f"jpeg_entropy: huff [4,256] int32 expected, got {tuple(huff.shape)} {huff.dtype}")
    _lib.launch("sr_jpeg_entropy", coef, coef, B, H, W, huff.contiguous(), ws.bits, ws.bits.numel(), ws.rowbuf, ws.rowbuf.numel(), ws.row_len)


def jpeg_gather(B, ws):
    """ws.out = the scan data of frames 0 .. B - 1 back to back, ws.offsets[:B + 1] their bounds (sr_jpeg_gather)."""
    if not 1 <= B <= ws.B:
        raise ValueError(f"jpeg_gather: {B} frames for a workspace of {ws.B}")
    _lib.launch("sr_jpeg_gather", ws.rowbuf, ws.rowbuf, ws.row_len, B, ws.H, ws.W, ws.row_start, ws.out, ws.out.numel(), ws.offsets)
