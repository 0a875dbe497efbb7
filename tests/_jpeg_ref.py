"""The Motion-JPEG encoder of DESIGN 3.17 restated in numpy, from RGB to bytes: integer arrays and plain loops over blocks, written
from the stated arithmetic and ITU-T T.81 Annex K, not from the kernel.  `encode(rgb, quality)` is a complete JFIF file; `parse`
splits a stream into its segments and restart intervals; `encode(..., stats=[])` also counts the ZRL / EOB symbols per block."""
import math
import struct

import numpy as np

# T.81 Annex K.1 / K.2: the luminance and chrominance quantisation tables, in natural (row-major) order
Q_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
Q_CHR = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL of the four tables
DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4"
    "c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
HUFF = ((0x00, DC_LUM), (0x10, AC_LUM), (0x01, DC_CHR), (0x11, AC_CHR))          # (Tc << 4 | Th, table) in the DHT's order


def zigzag():
    """natural index of each zigzag position, walked along the anti-diagonals (T.81 figure 5)."""
    order = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += [y * 8 + x for y, x in (cells if s % 2 else reversed(cells))]
    return order


def quant_table(base, quality):
    """IJG scaling: scale = 5000 / q below 50, 200 - 2 q from 50 on; entry = (base * scale + 50) / 100 clamped to [1, 255]."""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [min(max((b * scale + 50) // 100, 1), 255) for b in base]


def dct_matrix():
    """C[u][x] = round(8192 * c(u) / 2 * cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt 2: seven magnitudes and 2896."""
    k = [int(round(4096 * math.cos(j * math.pi / 16))) for j in range(8)]          # 4096, 4017, 3784, 3406, 2896, 2276, 1567, 799
    C = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            if u == 0:
                C[u, x] = k[4]
                continue
            j = ((2 * x + 1) * u) % 32                                              # cos(j pi / 16), folded into the first quadrant
            sign = 1
            if j > 16:
                j = 32 - j
            if j > 8:
                j, sign = 16 - j, -1
            C[u, x] = sign * k[j] if j < 8 else 0
    return C


def huff_codes(bits, vals):
    """{symbol: (code, length)} by T.81 Annex C: codes of one length count up, a longer length appends a zero."""
    out, code, i = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[i]] = (code, length)
            code += 1
            i += 1
        code <<= 1
    return out


def planes(rgb):
    """(Y [16R,16M], Cb [8R,8M], Cr [8R,8M]) int64, level-shifted by -128, of rgb [H,W,3] padded to whole MCUs by repeating the last
    column and row; chroma is computed per pixel and averaged 2 x 2 with (a + b + c + d + 2) >> 2."""
    a = np.asarray(rgb).astype(np.int64)
    H, W = a.shape[:2]
    a = np.pad(a, ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge")
    R, G, B = a[..., 0], a[..., 1], a[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    half = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return Y - 128, half(Cb) - 128, half(Cr) - 128


def fdct_quant(block, C, qnat):
    """Quantised coefficients in natural order of one 8 x 8 block of samples: rows first, (sum + 2^10) >> 11, then columns,
    (sum + 2^14) >> 15; quantised by sign(F) ((|F| + (Q >> 1)) / Q), AC clamped to +-1023."""
    T = np.zeros((8, 8), np.int64)
    for y in range(8):
        for u in range(8):
            T[y, u] = (int(np.dot(C[u], block[y])) + 1024) >> 11
    out = [0] * 64
    for v in range(8):
        for u in range(8):
            F = (int(np.dot(C[v], T[:, u])) + 16384) >> 15
            Q = qnat[v * 8 + u]
            q = (abs(F) + (Q >> 1)) // Q
            q = -q if F < 0 else q
            if v or u:
                q = min(max(q, -1023), 1023)
            out[v * 8 + u] = q
    return out


def _category(v):
    return int(abs(v)).bit_length()


def _value_bits(v, cat):
    return (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def block_bits(zz, pred, dc, ac, stats=None):
    """The code string ('0' / '1') of one block of zigzag-ordered coefficients after DC prediction `pred`."""
    s = []
    diff = zz[0] - pred
    cat = _category(diff)
    code, n = dc[cat]
    s.append(format(code, "0%db" % n))
    if cat:
        s.append(format(_value_bits(diff, cat), "0%db" % cat))
    run, zrl, eob = 0, 0, 0
    for k in range(1, 64):
        if zz[k] == 0:
            run += 1
            continue
        while run >= 16:
            code, n = ac[0xF0]
            s.append(format(code, "0%db" % n))
            run -= 16
            zrl += 1
        cat = _category(zz[k])
        code, n = ac[(run << 4) | cat]
        s.append(format(code, "0%db" % n) + format(_value_bits(zz[k], cat), "0%db" % cat))
        run = 0
    if run:
        code, n = ac[0x00]
        s.append(format(code, "0%db" % n))
        eob = 1
    if stats is not None:
        stats.append((zrl, eob))
    return "".join(s)


def headers(H, W, quality):
    zz = zigzag()
    ql, qc = quant_table(Q_LUM, quality), quant_table(Q_CHR, quality)
    seg = lambda marker, body: bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xDB, bytes([0]) + bytes(ql[n] for n in zz)) + seg(0xDB, bytes([1]) + bytes(qc[n] for n in zz))
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tcth, (bits, vals) in HUFF:
        out += seg(0xC4, bytes([tcth]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, struct.pack(">H", (W + 15) // 16))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(rgb, quality, stats=None):
    """The JFIF file of rgb [H,W,3] uint8.  `stats`: a list that receives (ZRL count, EOB count) per block in stream order."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W = rgb.shape[:2]
    Y, Cb, Cr = planes(rgb)
    C, zz = dct_matrix(), zigzag()
    ql, qc = quant_table(Q_LUM, quality), quant_table(Q_CHR, quality)
    dcl, acl, dcc, acc = (huff_codes(*t) for t in (DC_LUM, AC_LUM, DC_CHR, AC_CHR))
    rows, mpr = (H + 15) // 16, (W + 15) // 16
    out = [headers(H, W, quality)]
    for r in range(rows):
        pred = [0, 0, 0]
        bits = []
        for m in range(mpr):
            blocks = [(0, Y[16 * r + 8 * j:16 * r + 8 * j + 8, 16 * m + 8 * i:16 * m + 8 * i + 8]) for j in (0, 1) for i in (0, 1)]
            blocks += [(1, Cb[8 * r:8 * r + 8, 8 * m:8 * m + 8]), (2, Cr[8 * r:8 * r + 8, 8 * m:8 * m + 8])]
            for comp, blk in blocks:
                nat = fdct_quant(blk, C, qc if comp else ql)
                z = [nat[n] for n in zz]
                bits.append(block_bits(z, pred[comp], dcc if comp else dcl, acc if comp else acl, stats))
                pred[comp] = z[0]
        s = "".join(bits)
        s += "1" * (-len(s) % 8)
        raw = int(s, 2).to_bytes(len(s) // 8, "big")
        out.append(raw.replace(b"\xff", b"\xff\x00"))
        if r != rows - 1:
            out.append(bytes([0xFF, 0xD0 + r % 8]))
    out.append(b"\xff\xd9")
    return b"".join(out)


def parse(stream):
    """-> (segments, intervals, rst): segments [(marker, body)] from SOI to SOS in order (SOI and EOI with empty bodies, EOI last),
    intervals the entropy-coded byte strings between the restart markers (still stuffed), rst the m of each RSTm met."""
    assert stream[:2] == b"\xff\xd8"
    segs, pos = [(0xD8, b"")], 2
    while True:
        assert stream[pos] == 0xFF, pos
        marker = stream[pos + 1]
        n = struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        segs.append((marker, stream[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if marker == 0xDA:
            break
    intervals, rst, start = [], [], pos
    while True:
        i = stream.index(b"\xff", pos)
        nxt = stream[i + 1]
        if nxt == 0x00:
            pos = i + 2
        elif 0xD0 <= nxt <= 0xD7:
            intervals.append(stream[start:i])
            rst.append(nxt - 0xD0)
            start = pos = i + 2
        else:
            assert nxt == 0xD9 and i + 2 == len(stream), (i, nxt)
            intervals.append(stream[start:i])
            segs.append((0xD9, b""))
            return segs, intervals, rst
