"""A PNG decoder for the export tests (8-bit grey / RGB / RGBA, non-interlaced, all five row filters): zlib and struct only."""
import struct
import zlib

import numpy as np


def read_png(path):
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(blob):
        n, tag = struct.unpack(">I4s", blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat += data
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    assert depth == 8 and interlace == 0
    c = {0: 1, 2: 3, 6: 4}[ctype]
    raw = zlib.decompress(idat)
    stride = w * c
    out = np.zeros((h, stride), np.int32)
    for r in range(h):
        ft, line = raw[r * (stride + 1)], np.frombuffer(raw, np.uint8, stride, r * (stride + 1) + 1).astype(np.int32)
        prev = out[r - 1] if r else np.zeros(stride, np.int32)
        cur = out[r]
        for i in range(stride):
            a = cur[i - c] if i >= c else 0
            b, d = prev[i], prev[i - c] if i >= c else 0
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            else:
                p = a + b - d
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - d)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else d)
            cur[i] = (line[i] + pred) & 0xFF
    img = out.astype(np.uint8).reshape(h, w, c)
    return img[:, :, 0] if c == 1 else img
