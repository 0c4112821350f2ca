"""A by-hand PNG / APNG reader for the render tests: chunks with their CRCs checked, the zlib streams inflated, filter type 0 only
(what ``render.write_png`` / ``write_apng`` emit), 8-bit RGB."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"


def read_chunks(path):
    """[(type, data)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND."""
    raw = open(path, "rb").read()
    assert raw[:8] == SIG, "not a PNG signature"
    pos, chunks = 8, []
    while pos < len(raw):
        (n,) = struct.unpack(">I", raw[pos:pos + 4])
        kind, data = raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(kind + data) & 0xFFFFFFFF), f"bad CRC in {kind}"
        chunks.append((kind, data))
        pos += 12 + n
    assert pos == len(raw) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    return chunks


def _image(stream: bytes, h: int, w: int) -> np.ndarray:
    rows = np.frombuffer(zlib.decompress(stream), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any(), "a row uses a filter other than 0"
    return rows[:, 1:].reshape(h, w, 3).copy()


def decode(path):
    """(frames (T,H,W,3) uint8, info) with info = {"animated", "num_frames", "num_plays", "delays": [(num, den)]}.  For a plain PNG
    T = 1.  Checks the APNG structure: acTL before IDAT, one fcTL per frame, sequence numbers 0, 1, 2, ... over fcTL and fdAT, frame 0
    in IDAT (the default image), full-size frames at offset 0."""
    chunks = read_chunks(path)
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    kinds = [k for k, _ in chunks]
    idat = b"".join(d for k, d in chunks if k == b"IDAT")
    if b"acTL" not in kinds:
        assert b"fcTL" not in kinds and b"fdAT" not in kinds
        return _image(idat, h, w)[None], {"animated": False, "num_frames": 1, "num_plays": 0, "delays": []}
    assert kinds.index(b"acTL") < kinds.index(b"IDAT")
    num_frames, num_plays = struct.unpack(">II", chunks[kinds.index(b"acTL")][1])
    seq, delays, streams = 0, [], []
    for k, d in chunks:
        if k == b"fcTL":
            s, fw, fh, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", d)
            assert (s, fw, fh, x, y, dispose, blend) == (seq, w, h, 0, 0, 0, 0)
            seq += 1
            delays.append((num, den))
            streams.append(b"")
        elif k == b"IDAT":
            assert len(streams) == 1, "IDAT must be frame 0, behind the first fcTL"
            streams[0] += d
        elif k == b"fdAT":
            assert struct.unpack(">I", d[:4])[0] == seq and len(streams) >= 2
            seq += 1
            streams[-1] += d[4:]
    assert len(streams) == num_frames == len(delays)
    frames = np.stack([_image(s, h, w) for s in streams])
    return frames, {"animated": True, "num_frames": num_frames, "num_plays": num_plays, "delays": delays}
