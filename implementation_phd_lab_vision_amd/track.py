"""A crop box per frame that follows the person, and the op that crops and resizes with one box per output frame
(INTEGRATION.md section AA; C ABI: include/r50_track.h).

A feature cache gives every 40-frame clip its own box, ``frames.square_crop_from_2d`` over the clip's joints, so the person fills about
1/1.6 of the crop.  ``predict`` with one box for the whole video gives a subject who walks across the frame the square around
everything they ever touched.  Here every frame gets the box of the clip the cache would hold around it, optionally smoothed along time:

* ``track_boxes``             2D joints -> one ``[top, left, side, side]`` per frame (host; a few dozen flops per frame).
* ``TrackSettings``           ``window`` / ``smooth`` / ``scale`` of ``predict(track=...)`` and ``--track``.
* ``BoxTable``                the checked table of ``r50_op_crop_resize_boxes_u8``: checked on the host, the kernel trusts it.
* ``crop_resize_boxes_u8``    the ctypes wrapper of the op.  There is no CPU fallback.

Boxes with sub-pixel origins and padding outside the image are not offered: the reference pushes a box back inside the image, and so
does this (a square larger than the image cannot be pushed inside: it sticks out, as upstream, and is refused before any launch).
"""
from __future__ import annotations

import functools
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import frames as F

TABLE_COLS = 9                   # offset, H, W, top, left, hh, ww, px, py (include/r50_track.h)
MAX_OUT_SIZE = 4096
MAX_WW = (160 * 1024 - 12) // 6  # two dword-padded source rows of the widest crop fit the 160 KB of LDS


# ---- the box track ------------------------------------------------------------------------------------------------------------------
def shifted_window(i: int, n: int, window: int) -> int:
    """Start ``s`` of frame ``i``'s window ``[s, s + window) ∩ [0, n)``: centred on the frame, shifted (not truncated) at the ends of the
    video -- the clip a cache would hold around that frame."""
    return min(max(int(i) - int(window) // 2, 0), max(0, int(n) - int(window)))


def _windowed_mean(series: np.ndarray, window: int) -> np.ndarray:
    """fp32 series -> per element the mean over its shifted window: the correctly rounded sum (``math.fsum``) divided by the count in
    fp64, rounded once to fp32.  No dependence on a summation order; a constant series stays bit-constant."""
    n = int(series.shape[0])
    values = [float(v) for v in series]
    out = np.empty(n, dtype=np.float32)
    for i in range(n):
        s = shifted_window(i, n, window)
        e = min(n, s + window)
        out[i] = np.float32(math.fsum(values[s:e]) / (e - s))
    return out


def track_boxes(joints2d, img_h: int, img_w: int, window: int = 40, smooth: Optional[int] = None, scale: float = 1.6) -> torch.Tensor:
    """``joints2d`` (n, J, 2) fp32 pixels -> (n, 4) int64 ``[top, left, side, side]``.  A box lies inside the image whenever ``scale`` x
    the larger extent fits into it; a larger square sticks out, exactly as ``square_crop_from_2d`` leaves it, and ``check_boxes`` (so
    ``predict``) refuses it before any launch.  The extent of frame
    ``i`` is the exact per-axis minimum and maximum of the joints of its ``shifted_window``; with ``smooth > 1`` (default: ``window``)
    each of the four extent series is replaced by its ``_windowed_mean``; the box is ``frames.square_crop_from_extent`` of the extent.
    So with ``smooth=1`` box ``i`` is ``square_crop_from_2d(joints2d[s:s + window])``, and with ``window >= n`` every box is the one
    box ``predict.choose_box`` makes from all frames."""
    j = torch.as_tensor(np.asarray(joints2d), dtype=torch.float32)
    if j.dim() != 3 or j.shape[2] != 2 or j.shape[0] < 1 or j.shape[1] < 1:
        raise ValueError(f"joints2d must be (n, J, 2) with n, J >= 1, got {tuple(j.shape)}")
    window = int(window)
    smooth = window if smooth is None else int(smooth)
    if window < 1 or smooth < 1:
        raise ValueError(f"window and smooth must be >= 1, got {window} and {smooth}")
    if int(img_h) < 1 or int(img_w) < 1:
        raise ValueError(f"the image must be at least 1 x 1, got {img_h} x {img_w}")
    n = int(j.shape[0])
    lo_f, hi_f = (v.numpy() for v in torch.aminmax(j, dim=1))             # (n, 2) each: per frame
    lo, hi = np.empty((n, 2), dtype=np.float32), np.empty((n, 2), dtype=np.float32)
    for i in range(n):
        s = shifted_window(i, n, window)
        lo[i], hi[i] = lo_f[s:s + window].min(axis=0), hi_f[s:s + window].max(axis=0)
    if smooth > 1:
        for series in (lo, hi):
            for axis in (0, 1):
                series[:, axis] = _windowed_mean(series[:, axis], smooth)
    lo_t, hi_t = torch.from_numpy(lo), torch.from_numpy(hi)
    return torch.stack([F.square_crop_from_extent(lo_t[i], hi_t[i], int(img_h), int(img_w), scale) for i in range(n)])


class TrackSettings:
    """``window``: frames of the clip around a frame whose joints give its box (``predict --track-window``, default the head's window);
    ``smooth``: frames of the mean over the extents (None: ``window``; 1: none); ``scale``: the square's edge over the larger extent."""

    def __init__(self, window: int = 40, smooth: Optional[int] = None, scale: float = 1.6):
        if int(window) != window or int(window) < 1:
            raise ValueError(f"window must be an integer >= 1, got {window}")
        if smooth is not None and (int(smooth) != smooth or int(smooth) < 1):
            raise ValueError(f"smooth must be an integer >= 1, got {smooth}")
        if not (math.isfinite(float(scale)) and float(scale) > 0.0):
            raise ValueError(f"scale must be finite and > 0, got {scale}")
        self.window, self.smooth, self.scale = int(window), (None if smooth is None else int(smooth)), float(scale)

    def __eq__(self, other):
        return isinstance(other, TrackSettings) and (self.window, self.smooth, self.scale) == (other.window, other.smooth, other.scale)

    def describe(self) -> str:
        return f"window={self.window} smooth={self.window if self.smooth is None else self.smooth} scale={self.scale:g}"

    def boxes(self, joints2d, img_h: int, img_w: int) -> torch.Tensor:
        return track_boxes(joints2d, img_h, img_w, self.window, self.smooth, self.scale)


def check_boxes(boxes, n: int, img_h: int, img_w: int) -> np.ndarray:
    """``boxes`` as (n, 4) int64 ``[top, left, hh, ww]``, each inside the ``img_h`` x ``img_w`` image; anything else is refused."""
    host = np.asarray(boxes.detach().cpu().numpy() if isinstance(boxes, torch.Tensor) else boxes)
    if host.ndim != 2 or host.shape != (int(n), 4) or host.dtype.kind not in "iu":
        raise ValueError(f"boxes must be ({n}, 4) integers [top, left, hh, ww], got {host.dtype} {host.shape}")
    host = host.astype(np.int64)
    top, left, hh, ww = host.T
    bad = (top < 0) | (left < 0) | (hh < 1) | (ww < 1) | (top + hh > int(img_h)) | (left + ww > int(img_w))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f"box {host[i].tolist()} of frame {i} does not lie inside a {img_h} x {img_w} image")
    return host


# ---- the table of the op ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight_precision(size: int, out_size: int) -> int:
    """``r50_track_weight_precision``: the fixed-point weight precision of one axis, the library's one definition, cached per pair."""
    return int(_lib.load_library().r50_track_weight_precision(int(size), int(out_size)))


class BoxTable:
    """The (t, 9) int64 table of ``r50_op_crop_resize_boxes_u8``, one row per output frame, checked on the host -- the kernel trusts it:
    ``offsets`` (t,) byte offsets of the images in a buffer of ``src_bytes`` bytes, ``sizes`` (t, 2) or (2,) their ``H, W``, ``boxes``
    (t, 4) ``[top, left, hh, ww]``.  Every box lies inside its image with ``hh, ww >= 1``, every image inside ``[0, src_bytes)``, and in
    fixed mode both weight precisions are >= 1.  ``host`` is the table, ``max_ww`` the widest crop (it sizes the kernel's LDS).  With
    ``device`` the table is uploaded once (``table``); without, the caller uploads ``host`` itself (``predict`` sends it in the same
    copy as the pixels) and passes that tensor to ``crop_resize_boxes_u8``."""

    def __init__(self, offsets, sizes, boxes, src_bytes: int, out_size: int = 224, mode: int = F.RESIZE_FLOAT, device=None):
        def as_int(name, v, shape_ok):
            host = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
            if host.dtype.kind not in "iu" or not shape_ok(host.shape):
                raise ValueError(f"{name}: unexpected {host.dtype} {host.shape}")
            return host.astype(np.int64)
        off = as_int("offsets must be (t,) integers with t >= 1", offsets, lambda s: len(s) == 1 and s[0] >= 1)
        t = int(off.shape[0])
        size = as_int(f"sizes must be ({t}, 2) or (2,) integers", sizes, lambda s: s in ((t, 2), (2,)))
        size = np.broadcast_to(size, (t, 2))
        box = as_int(f"boxes must be ({t}, 4) integers", boxes, lambda s: s == (t, 4))
        out_size, mode, src_bytes = int(out_size), int(mode), int(src_bytes)
        if mode not in (F.RESIZE_FLOAT, F.RESIZE_FIXED):
            raise ValueError(f"unknown resize mode {mode}")
        if out_size < 4 or out_size % 4 or out_size > MAX_OUT_SIZE:
            raise ValueError(f"out_size must be a multiple of 4 in [4, {MAX_OUT_SIZE}], got {out_size}")
        if t * out_size >= 1 << 31:
            raise ValueError(f"t * out_size = {t * out_size} does not fit the grid")
        h, w = size[:, 0], size[:, 1]
        top, left, hh, ww = box.T
        if (h < 1).any() or (w < 1).any():
            raise ValueError("every image must be at least 1 x 1")
        bad = (top < 0) | (left < 0) | (hh < 1) | (ww < 1) | (top + hh > h) | (left + ww > w)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise ValueError(f"row {i}: box {box[i].tolist()} does not lie inside its {int(h[i])} x {int(w[i])} image")
        bad = (off < 0) | (off + 3 * h * w > src_bytes)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise ValueError(f"row {i}: the {int(h[i])} x {int(w[i])} image at byte {int(off[i])} does not lie inside [0, {src_bytes})")
        if int(ww.max()) > MAX_WW:
            raise ValueError(f"a crop of {int(ww.max())} columns is too wide (at most {MAX_WW})")
        host = np.empty((t, TABLE_COLS), dtype=np.int64)
        host[:, 0], host[:, 1], host[:, 2], host[:, 3:7] = off, h, w, box
        host[:, 7:9] = 1
        if mode == F.RESIZE_FIXED:
            host[:, 7] = [weight_precision(int(v), out_size) for v in ww]
            host[:, 8] = [weight_precision(int(v), out_size) for v in hh]
            if int(host[:, 7:9].min()) < 1:
                raise ValueError("degenerate fixed-point weights")
        self.host, self.t, self.max_ww = host, t, int(ww.max())
        self.src_bytes, self.out_size, self.mode = src_bytes, out_size, mode
        self.table = torch.from_numpy(host).to(device) if device is not None else None


def crop_resize_boxes_u8(src: torch.Tensor, table: BoxTable, out: Optional[torch.Tensor] = None, out_flip: Optional[torch.Tensor] = None,
                         flip: bool = False, table_dev: Optional[torch.Tensor] = None):
    """One ``r50_op_crop_resize_boxes_u8`` launch: ``src`` a contiguous uint8 tensor on an MI355X holding the images ``table`` names
    (``table.src_bytes`` bytes, 4-byte aligned) -> ``out`` (t, 3, out, out) uint8: frame ``i`` is the resized box of table row ``i``, the
    bits ``frames.crop_and_resize_video_uint8`` gives for that image and box.  With ``flip`` (or an ``out_flip``) the same launch also
    writes the frames mirrored along the width, what the ``hflip=True`` call gives, and ``(out, out_flip)`` is returned.  ``table_dev``:
    a (t, 9) int64 device tensor the caller has filled with ``table.host`` (default: ``table.table``).  Fully asynchronous; everything
    is checked on the host before the launch.  There is no CPU fallback."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError("crop_resize_boxes_u8: need a contiguous uint8 tensor on the GPU: there is no CPU fallback")
    if int(src.numel()) != table.src_bytes:
        raise ValueError(f"crop_resize_boxes_u8: the table was checked against {table.src_bytes} bytes, src has {int(src.numel())}")
    dev_table = table.table if table_dev is None else table_dev
    if dev_table is None:
        raise ValueError("crop_resize_boxes_u8: the table was made without a device, and no table_dev was given")
    if dev_table.dtype != torch.int64 or tuple(dev_table.shape) != (table.t, TABLE_COLS) or not dev_table.is_contiguous() \
            or dev_table.device != src.device:
        raise ValueError(f"crop_resize_boxes_u8: the device table must be a contiguous ({table.t}, {TABLE_COLS}) int64 tensor on src's device")
    shape = (table.t, 3, table.out_size, table.out_size)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    if out_flip is None and flip:
        out_flip = torch.empty(shape, dtype=torch.uint8, device=src.device)
    for name, v in (("out", out), ("out_flip", out_flip)):
        if v is not None and (tuple(v.shape) != shape or v.dtype != torch.uint8 or not v.is_contiguous() or v.device != src.device):
            raise ValueError(f"crop_resize_boxes_u8: `{name}` must be a contiguous {shape} uint8 tensor on src's device")
    with torch.cuda.device(src.device):
        rc = _lib.load_library().r50_op_crop_resize_boxes_u8(src.data_ptr(), table.src_bytes, dev_table.data_ptr(), table.t, table.max_ww,
                                                             out.data_ptr(), None if out_flip is None else out_flip.data_ptr(),
                                                             table.out_size, table.mode, torch.cuda.current_stream(src.device).cuda_stream)
    _lib.check(rc, None, "r50_op_crop_resize_boxes_u8")
    return out if out_flip is None else (out, out_flip)
