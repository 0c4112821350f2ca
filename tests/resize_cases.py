"""The one case list of the crop + resize domain tests (tests/test_resize_oracle_cpu.py on the host, tests/test_frames_domain_gpu.py on
the MI355X).  No GPU import: the CPU tests pin the oracle on exactly the cases the kernels are then held to.

``OUTS``        4 is the smallest legal output size; 12 is no multiple of 8; 344 gives ``quads * 3 = 258`` items a row, so the second
                round of the kernels' item loop holds 2 items; 448 gives a second round of 80.
``SOURCES(out)`` crop sizes ``(hh, ww)``: the identity on exactly one axis, up-scaling on one axis with down-scaling on the other,
                one-pixel rows and columns, and sizes whose two fixed-point weight precisions differ.
``image``       a deterministic ``(T, hh, ww, 3)`` crop, seeded from ``(hh, ww, out)``; frame 0 has one saturated and one zero channel.
``embed``       places a crop inside a larger ``(T, H, W, 3)`` clip of other noise and returns the clip and its box.
``placements``  two placements per crop, both with odd ``W`` (``3 W`` is odd, so the crop's rows start at every residue mod 4):
                ``inner`` has clip pixels on all four sides; ``tail`` has none behind, ``H`` is odd too and ``T = 3``, so the box of the
                last frame ends at the clip's last byte and ``T H W 3`` is odd: the last staged dword of that row reaches past the
                tensor and is read byte by byte.
"""
import numpy as np
import torch

OUTS = (4, 8, 12, 224, 344, 448)
T = 3


def SOURCES(out):
    return [(1, 1), (1, 7), (7, 1), (2, 3), (40, 8), (8, 40), (out, 37), (37, out), (out + 1, out - 1), (3 * out, 2 * out + 1), (63, 79),
            (500, 131), (131, 500), (1000, 3), (23, 76)]


CASES = [(hh, ww, out) for out in OUTS for hh, ww in SOURCES(out)]
assert len(CASES) == 15 * len(OUTS) == len(set(CASES))


def case_id(case):
    return "%dx%d_to_%d" % tuple(case)


def image(hh, ww, out, t=T):
    """(t, hh, ww, 3) uint8.  Frame 0: channel 0 saturated, channel 1 zero (clamping and rounding at both ends of the range)."""
    g = torch.Generator().manual_seed((hh * 4099 + ww) * 8191 + out)
    img = torch.randint(0, 256, (t, hh, ww, 3), generator=g, dtype=torch.uint8)
    img[0, :, :, 0] = 255
    img[0, :, :, 1] = 0
    return img


def embed(img, top, left, pad_bottom, pad_right):
    """``img`` (T, hh, ww, 3) inside a clip (T, top + hh + pad_bottom, left + ww + pad_right, 3) of other noise -> (clip, box)."""
    t, hh, ww, _ = img.shape
    h, w = top + hh + pad_bottom, left + ww + pad_right
    g = torch.Generator().manual_seed(h * 65537 + w * 17 + t)
    clip = torch.randint(0, 256, (t, h, w, 3), generator=g, dtype=torch.uint8)
    clip[:, top:top + hh, left:left + ww] = img
    return clip, [top, left, hh, ww]


def placements(hh, ww):
    """((name, top, left, pad_bottom, pad_right), ..): see the module docstring."""
    inner = ("inner", 3, 5, 2, 2 if ww % 2 == 0 else 3)
    tail = ("tail", 1 if hh % 2 == 0 else 2, 1 if ww % 2 == 0 else 2, 0, 0)
    for _name, top, left, pb, pr in (inner, tail):
        assert (left + ww + pr) % 2 == 1
    assert (tail[1] + hh) % 2 == 1 and T % 2 == 1
    return inner, tail


def ends_at_the_last_byte(clip, box):
    """The box of the last frame ends at the clip's last byte, and the clip ends off a dword boundary."""
    t, h, w, _ = clip.shape
    top, left, hh, ww = box
    return top + hh == h and left + ww == w and (t * h * w * 3) % 4 != 0


def crop_nchw(img):
    """(T, hh, ww, 3) -> the (T, 3, hh, ww) numpy view the oracle's resize functions take."""
    return np.transpose(img.numpy(), (0, 3, 1, 2))


def packed_table(out, tail, sources=None):
    """The images of ``SOURCES(out)`` (or ``sources``), one frame each, packed back to back into one byte buffer for
    ``r50_op_crop_resize_boxes_u8``: row ``k`` is frame ``k % T`` of ``image(hh, ww, out)`` under its ``inner`` placement (the last row
    under its ``tail`` placement) and starts at a byte offset of residue ``k % 4`` (the gaps hold other noise).  The last image starts at
    the residue that makes the buffer end ``tail`` (1, 2 or 3) bytes past a dword boundary, and its box ends at the buffer's last byte.
    -> dict(buf (src_bytes,) uint8, offsets, sizes, boxes (int64 numpy), frames [(source, frame index)], src_bytes, max_w)."""
    assert tail in (1, 2, 3)
    sources = SOURCES(out) if sources is None else list(sources)
    offsets, sizes, boxes, frames, pieces, cursor = [], [], [], [], [], 0
    for k, (hh, ww) in enumerate(sources):
        last = k == len(sources) - 1
        _name, top, left, pb, pr = placements(hh, ww)[1 if last else 0]
        clip, box = embed(image(hh, ww, out), top, left, pb, pr)
        h, w = int(clip.shape[1]), int(clip.shape[2])
        residue = (tail - 3 * h * w) % 4 if last else k % 4
        gap = (residue - cursor) % 4
        if gap:
            pieces.append(torch.full((gap,), 0x5A + k, dtype=torch.uint8))
            cursor += gap
        offsets.append(cursor)
        sizes.append([h, w])
        boxes.append(box)
        frames.append(((hh, ww), k % T))
        pieces.append(clip[k % T].reshape(-1))
        cursor += 3 * h * w
    buf = torch.cat(pieces)
    assert buf.numel() == cursor and cursor % 4 == tail
    top, left, hh, ww = boxes[-1]
    assert offsets[-1] + ((top + hh - 1) * sizes[-1][1] + left + ww) * 3 == cursor, "the last box ends at the buffer's last byte"
    if len(sources) >= 4:
        assert {o % 4 for o in offsets} == {0, 1, 2, 3}
    return dict(buf=buf, offsets=np.asarray(offsets, np.int64), sizes=np.asarray(sizes, np.int64), boxes=np.asarray(boxes, np.int64),
                frames=frames, src_bytes=cursor, max_w=max(s[1] for s in sizes))
