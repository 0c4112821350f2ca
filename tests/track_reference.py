"""Independent restatements and shared cases for the box track and the per-frame-box crop op (INTEGRATION.md section AA).

* ``walker``            2D joints of a subject walking across the image, fp32 with fractional coordinates.
* ``boxes_unsmoothed``  the definition with ``smooth=1``: ``square_crop_from_2d`` of each frame's shifted window.
* ``boxes_smoothed``    the definition with smoothing, the sums in ``fractions.Fraction`` (exact), one rounding to fp64, the division in
                        fp64, one rounding to fp32.
* ``ragged_case``       7 images of different sizes at byte offsets congruent to 0, 1, 2, 3 mod 4 in one buffer, with the boxes the issue
                        lists; the last image ends the buffer off a dword boundary and its box ends at the last byte, so the byte-wise
                        tail read runs (``src_bytes % 4`` = 1, 2 or 3: one branch each).
"""
from fractions import Fraction

import numpy as np
import torch


def walker(n=97, img_h=120, img_w=200, joints=17, seed=0, x_from=60.0, x_to=120.0, half=(4.0, 10.0), bob=4.0, wobble=0.5):
    """(n, joints, 2) fp32 (x, y): a body of about ``2 half`` pixels whose centre walks from ``x_from`` to ``x_to`` at mid height and bobs
    vertically.  The defaults keep 1.6 x the extent of the WHOLE walk below the image's 120 rows, so that every window's square fits the
    image: a square larger than the image is what ``square_crop_from_2d`` leaves sticking out (tests/test_track_cpu.py pins that too)."""
    rng = np.random.default_rng(seed)
    body = rng.uniform(-1.0, 1.0, (joints, 2)) * np.asarray(half)
    t = np.linspace(0.0, 1.0, n)
    cx = x_from + t * (x_to - x_from)
    cy = img_h / 2 + bob * np.sin(t * 9.0)
    noise = rng.normal(0.0, wobble, (n, joints, 2))
    return (body[None] + np.stack([cx, cy], axis=-1)[:, None] + noise).astype(np.float32)


def window_start(i, n, window):
    s = i - window // 2
    if s > n - window:
        s = n - window
    return max(s, 0)


def boxes_unsmoothed(joints2d, img_h, img_w, window, scale=1.6):
    from implementation_phd_lab_vision_amd.frames import square_crop_from_2d
    n = joints2d.shape[0]
    j = torch.from_numpy(joints2d)
    return torch.stack([square_crop_from_2d(j[window_start(i, n, window):window_start(i, n, window) + window], img_h, img_w, scale)
                        for i in range(n)])


def _mean32(values, s, e):
    total = sum((Fraction(float(v)) for v in values[s:e]), Fraction(0))
    return np.float32(float(total) / (e - s))          # float(Fraction) rounds correctly: the correctly rounded sum, then fp64 division


def boxes_smoothed(joints2d, img_h, img_w, window, smooth, scale=1.6):
    from implementation_phd_lab_vision_amd.frames import square_crop_from_extent
    n = joints2d.shape[0]
    lo, hi = np.empty((n, 2), np.float32), np.empty((n, 2), np.float32)
    for i in range(n):
        s = window_start(i, n, window)
        pts = joints2d[s:s + window].reshape(-1, 2)
        lo[i], hi[i] = pts.min(axis=0), pts.max(axis=0)
    out = []
    for i in range(n):
        s = window_start(i, n, smooth)
        e = min(n, s + smooth)
        lo_i = np.array([_mean32(lo[:, a], s, e) for a in (0, 1)], np.float32)
        hi_i = np.array([_mean32(hi[:, a], s, e) for a in (0, 1)], np.float32)
        out.append(square_crop_from_extent(torch.from_numpy(lo_i), torch.from_numpy(hi_i), img_h, img_w, scale))
    return torch.stack(out)


RAGGED_SIZES = [(64, 80), (33, 47), (17, 29), (64, 64), (5, 7), (40, 31), (21, 23)]
RAGGED_RESIDUES = [0, 1, 2, 3, 2, 1]          # of the first six images; the last image's residue is ``tail - 1``
TAILS = (1, 2, 3)


def ragged_case(out_size, tail=1, seed=0):
    """dict(buf (src_bytes,) uint8, images [(H, W, 3) uint8 copies], offsets, sizes, boxes, src_bytes) for ``out_size`` 8 or 224.
    ``src_bytes % 4 == tail`` (1, 2 or 3): the last image (21 x 23 x 3 = 1449 bytes, 1 mod 4) starts at a byte offset of residue
    ``tail - 1`` and ends the buffer, and the last box ends at the buffer's last byte, so in a 4-byte aligned buffer the last staged
    dword of that box's last row holds ``tail`` bytes of the buffer and 4 - ``tail`` bytes past its end: the kernel has to read it byte
    by byte, one branch of that read per ``tail``."""
    assert tail in TAILS
    residues = RAGGED_RESIDUES + [tail - 1]
    g = torch.Generator().manual_seed(100 + seed)
    offsets, cursor = [], 0
    for (h, w), r in zip(RAGGED_SIZES, residues):
        while cursor % 4 != r:
            cursor += 1
        offsets.append(cursor)
        cursor += 3 * h * w
    src_bytes = cursor                                   # the last image ends the buffer
    buf = torch.randint(0, 256, (src_bytes,), generator=g, dtype=torch.uint8)
    images = [buf[o:o + 3 * h * w].view(h, w, 3).clone() for o, (h, w) in zip(offsets, RAGGED_SIZES)]
    boxes = [[3, 5, 40, out_size if out_size <= 80 else 61],      # ww == out at out = 8 (float mode's identity), hh != ww
             [0, 0, 33, 1],                                       # ww = 1
             [4, 2, 1, 20],                                       # hh = 1
             [10, 7, 50, 13],                                     # ww > 8, hh != ww
             [2, 3, 1, 1],                                        # a single pixel
             [0, 0, 40, 31],                                      # the whole image
             [21 - 6, 23 - 5, 6, 5]]                              # the last rows and columns of the last image: ww < 8
    assert [o % 4 for o in offsets] == residues and set(residues) == {0, 1, 2, 3} and offsets[-1] + 3 * 21 * 23 == src_bytes
    assert src_bytes % 4 == tail, "the buffer must end off a dword boundary, or the byte-wise tail read never runs"
    top, left, hh, ww = boxes[-1]
    assert offsets[-1] + ((top + hh - 1) * 23 + left + ww) * 3 == src_bytes, "the last box ends at the buffer's last byte"
    return dict(buf=buf, images=images, offsets=np.asarray(offsets, np.int64), sizes=np.asarray(RAGGED_SIZES, np.int64),
                boxes=np.asarray(boxes, np.int64), src_bytes=src_bytes)
