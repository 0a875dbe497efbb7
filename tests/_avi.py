"""An AVI (RIFF) reader for the video tests, independent of the writer under test: struct only."""
import struct


def riff(blob):
    """An AVI file as {'avih', 'strh', 'strf', 'movi': [(offset of the chunk relative to the 'movi' fourcc, payload)], 'idx1': [...]},
    asserting sizes and word alignment on the way."""
    out = {"movi": [], "idx1": []}
    assert blob[:4] == b"RIFF" and blob[8:12] == b"AVI " and struct.unpack("<I", blob[4:8])[0] == len(blob) - 8

    def walk(start, end, movi_at):
        pos = start
        while pos < end:
            assert pos % 2 == 0, pos
            tag, n = blob[pos:pos + 4], struct.unpack("<I", blob[pos + 4:pos + 8])[0]
            assert pos + 8 + n <= end, (tag, pos, n)
            if tag == b"LIST":
                kind = blob[pos + 8:pos + 12]
                walk(pos + 12, pos + 8 + n, pos + 8 if kind == b"movi" else None)
            elif tag == b"00dc":
                assert movi_at is not None
                out["movi"].append((pos - movi_at, blob[pos + 8:pos + 8 + n]))
            elif tag == b"idx1":
                out["idx1"] = [struct.unpack("<4sIII", blob[pos + 8 + 16 * i:pos + 24 + 16 * i]) for i in range(n // 16)]
            else:
                out[tag.decode()] = blob[pos + 8:pos + 8 + n]
            pos += 8 + n + (n & 1)
        assert pos == end
    walk(12, len(blob), None)
    return out


def frames(path):
    """The payloads of the 00dc chunks of the AVI at `path`, in file order."""
    with open(path, "rb") as fh:
        return [p for _, p in riff(fh.read())["movi"]]
