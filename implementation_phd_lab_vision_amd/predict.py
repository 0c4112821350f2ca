"""Decoded video in, one 3D pose per frame out: the backbone and the lifting head run as one pass.

Every other entry point of the head (``results``, ``evaluate_dense``, ``rollout``, ``render``) reads a Human3.6M feature cache with
ground truth.  This one takes the frames of any video and a trained ``best.pt``:

    host:    one crop box for the whole video; per chunk the box region of the frames, sliced on the host and uploaded pinned
    device:  crop_and_resize_video_uint8 -> features_u8          every frame through the backbone ONCE -> feats (N, 2048) fp32
             joints_windows (r50_op_gather_window_rows + head)   the head's windows (40 frames, stride 5) are views of feats
             [flip TTA: the same on the mirrored crops, then r50_op_merge_mirrored_poses]
             stitch_poses                                        the overlapping windows fused into one pose per frame
             rollout                                             optionally, poses beyond the last frame

A feature cache holds a frame once per clip that covers it, each time under that clip's own crop box; here there is ONE box per video
(given, or from the 2D joints of all kept frames, or the centred square), so the features of a frame do not depend on the window it
is read through.  That is a stated deviation from the cache.  ``--track`` (track.py, INTEGRATION.md section AA) narrows it: a box per
FRAME, that of the clip the cache would hold around the frame, still with every frame through the backbone once.  ``--resample STEP``
(resample.py, INTEGRATION.md section AB) adds, after every other stage, poses every STEP video frames interpolated from the kept ones.

* ``window_starts``            where the windows begin (host).
* ``merge_mirrored_poses``     the ctypes wrapper of the merge op; ``gather_window_rows`` (model.py) is the other new op.
* ``VideoPredictor``           ``features`` / ``poses`` / ``forecast`` / ``predict``.
* ``python -m implementation_phd_lab_vision_amd.predict --frames clip.npy --model_path best.pt --weights resnet50.pth --out DIR``

Video decoding and person detection stay upstream: the input is decoded uint8 frames.  No CPU fallback.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from . import frames as F
from .model import gather_window_rows  # noqa: F401  (the pass's other op, re-exported beside merge_mirrored_poses)
from .protocols import MAX_JOINTS
from .sequences import FUSE_MODES, SequenceTable, StitchIndex, stitch_poses

FEATURE_DIM = 2048
OUT_SIZE = 224
UPLOAD_BYTES = 64 << 20          # pinned staging buffer: the box regions travel in pieces of at most this many bytes
RESIZE_MODES = {"float": F.RESIZE_FLOAT, "fixed": F.RESIZE_FIXED}


# ---- windows ------------------------------------------------------------------------------------------------------------------------
def window_starts(n: int, seq_len: int, stride: int) -> np.ndarray:
    """Starts (int32) of the windows over ``n`` frames: ``0, stride, 2 stride, ...`` while a whole window of ``seq_len`` frames fits,
    plus ``n - seq_len`` if that is not the last of them already, so every frame is covered.  A video shorter than ``seq_len`` is one
    window of its ``n`` frames (start 0; the window length is ``min(n, seq_len)``)."""
    n, seq_len, stride = int(n), int(seq_len), int(stride)
    if n < 1 or seq_len < 1 or stride < 1:
        raise ValueError(f"need n, seq_len, stride >= 1 (got {n}, {seq_len}, {stride})")
    if n <= seq_len:
        return np.zeros(1, dtype=np.int32)
    starts = list(range(0, n - seq_len + 1, stride))
    if starts[-1] != n - seq_len:
        starts.append(n - seq_len)
    return np.asarray(starts, dtype=np.int32)


def window_clips(starts: Sequence[int], t: int, name: str = "video") -> List[dict]:
    """The windows as index entries of one sequence, what ``SequenceTable.from_clips`` reads."""
    return [{"subject": 0, "action": str(name), "cam": "0", "start": int(s), "end": int(s) + int(t)} for s in starts]


# ---- flip test-time augmentation: the merge ---------------------------------------------------------------------------------------------
def flip_perm(joints: int, pairs: Sequence[Tuple[int, int]] = F.H36M_FLIP_PAIRS) -> np.ndarray:
    """The left/right swap as a permutation of ``joints`` indices (int32): the identity with every pair exchanged."""
    perm = np.arange(int(joints), dtype=np.int32)
    for l_idx, r_idx in pairs:
        if not (0 <= l_idx < joints and 0 <= r_idx < joints):
            raise ValueError(f"flip pair ({l_idx}, {r_idx}) does not fit a skeleton of {joints} joints")
        perm[l_idx], perm[r_idx] = r_idx, l_idx
    return perm


class MirrorPerm:
    """A joint permutation checked on the host -- the kernel trusts it -- and uploaded once: 1-D, at most ``MAX_JOINTS`` entries, every
    entry in range, and its own inverse (``perm[perm[j]] == j``: swapping left and right twice changes nothing)."""

    def __init__(self, perm, device):
        host = np.asarray(perm.detach().cpu().numpy() if isinstance(perm, torch.Tensor) else perm)
        if host.ndim != 1 or host.dtype.kind not in "iu" or not 1 <= host.size <= MAX_JOINTS:
            raise ValueError(f"perm must be a 1-D integer sequence of 1 .. {MAX_JOINTS} joints, got {host.dtype} {host.shape}")
        host = host.astype(np.int64)
        if int(host.min()) < 0 or int(host.max()) >= host.size:
            raise ValueError(f"every perm entry must lie in [0, {host.size}), got [{int(host.min())}, {int(host.max())}]")
        if not np.array_equal(host[host], np.arange(host.size)):
            raise ValueError("perm must be its own inverse (perm[perm[j]] == j): a left/right swap")
        self.joints = int(host.size)
        self.perm = torch.from_numpy(host.astype(np.int32)).to(device)


def merge_mirrored_poses(a: torch.Tensor, b_mirrored: torch.Tensor, perm: Union[MirrorPerm, Sequence[int]],
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``r50_op_merge_mirrored_poses`` launch: ``a`` (R, J, 3) fp32 poses of the frames, ``b_mirrored`` (R, J, 3) the poses of the
    mirrored frames -> ``0.5 * (a + M(b_mirrored))`` with ``M`` = negate x, swap left and right (``perm``: a ``MirrorPerm`` or the
    sequence to make one from): the inverse of ``frames.aug_hflip_annotations``.  The bits of that torch expression.  ``out`` may be
    ``a``.  Everything is checked on the host before the launch.  There is no CPU fallback."""
    if a.dim() != 3 or a.shape[2] != 3 or tuple(b_mirrored.shape) != tuple(a.shape) or a.dtype != torch.float32 \
            or b_mirrored.dtype != torch.float32 or a.shape[0] < 1:
        raise ValueError(f"a and b_mirrored (R,J,3) fp32 with R >= 1 expected, got {tuple(a.shape)} {a.dtype}, "
                         f"{tuple(b_mirrored.shape)} {b_mirrored.dtype}")
    if not isinstance(perm, MirrorPerm):
        perm = MirrorPerm(perm, a.device)
    rows, joints = int(a.shape[0]), int(a.shape[1])
    if perm.joints != joints:
        raise ValueError(f"perm has {perm.joints} joints, the poses {joints}")
    if out is None:
        out = torch.empty_like(a)
    every = (a, b_mirrored, out)
    if tuple(out.shape) != tuple(a.shape) or out.dtype != torch.float32:
        raise ValueError(f"out must be {tuple(a.shape)} fp32, got {tuple(out.shape)} {out.dtype}")
    if a.device.type != "cuda" or any(v.device != a.device for v in every) or perm.perm.device != a.device:
        raise ValueError("a, b_mirrored, out and perm must be on one GPU: there is no CPU fallback")
    if not all(v.is_contiguous() for v in every):
        raise ValueError("a, b_mirrored and out must be contiguous")
    with torch.cuda.device(a.device):
        rc = _lib.load_library().r50_op_merge_mirrored_poses(a.data_ptr(), b_mirrored.data_ptr(), rows, joints, perm.perm.data_ptr(),
                                                             out.data_ptr(), torch.cuda.current_stream(a.device).cuda_stream)
    _lib.check(rc, None, "r50_op_merge_mirrored_poses")
    return out


# ---- the crop box -------------------------------------------------------------------------------------------------------------------------
def centred_square(img_h: int, img_w: int) -> torch.Tensor:
    """``[top, left, side, side]`` int64: the centred square of the shorter side."""
    side = min(int(img_h), int(img_w))
    return torch.tensor([(int(img_h) - side) // 2, (int(img_w) - side) // 2, side, side], dtype=torch.int64)


def choose_box(img_h: int, img_w: int, box=None, joints2d=None) -> torch.Tensor:
    """The video's one crop box ``[top, left, hh, ww]`` int64, in order of precedence: ``box`` as given (it must lie inside the image);
    ``frames.square_crop_from_2d`` over ``joints2d`` (the 2D joints of all kept frames); the centred square of the shorter side."""
    if box is not None:
        out = torch.as_tensor(box.tolist() if isinstance(box, (torch.Tensor, np.ndarray)) else list(box), dtype=torch.int64).reshape(-1)
        if out.numel() != 4:
            raise ValueError(f"box must be [top, left, hh, ww], got {out.tolist()}")
        top, left, hh, ww = out.tolist()
        if top < 0 or left < 0 or hh < 1 or ww < 1 or top + hh > img_h or left + ww > img_w:
            raise ValueError(f"box {out.tolist()} does not lie inside a {img_h} x {img_w} image")
        return out
    if joints2d is not None:
        return F.square_crop_from_2d(torch.as_tensor(np.asarray(joints2d), dtype=torch.float32), int(img_h), int(img_w))
    return centred_square(img_h, img_w)


# ---- the pass ---------------------------------------------------------------------------------------------------------------------------------
class VideoPredictor:
    """``backbone``: a ``ResNet50Backbone`` and ``head``: a ``PHDFor3DJoints``, both on one MI355X.  ``seq_len`` / ``stride``: the head's
    windows (the features CLI's defaults, what heads are trained on); ``fuse``: how ``stitch_poses`` weighs a frame's windows
    (``context`` with ramp ``1 + 4 * head.number_blocks``, as ``evaluate_dense``); ``frame_batch`` frames per backbone call,
    ``window_batch`` windows per head call; ``flip_tta``: every frame a second time mirrored, the two poses merged.  ``stats`` counts
    what the last ``predict`` (or the calls since construction) sent through: ``backbone_frames``, ``windows``, ``head_rows``."""

    def __init__(self, backbone, head, seq_len: int = 40, stride: int = 5, fuse: str = "context", frame_batch: int = 256,
                 window_batch: int = 256, resize_mode: int = F.RESIZE_FLOAT, flip_tta: bool = False):
        if fuse not in FUSE_MODES:
            raise ValueError(f"fuse must be one of {sorted(FUSE_MODES)}, got {fuse!r}")
        if int(seq_len) < 1 or int(stride) < 1 or int(frame_batch) < 1 or int(window_batch) < 1:
            raise ValueError("seq_len, stride, frame_batch and window_batch must be >= 1")
        if head._device is None or backbone._device != head._device:
            raise ValueError(f"backbone ({backbone._device}) and head ({head._device}) must be on one GPU")
        if int(frame_batch) > backbone._max_batch:
            raise ValueError(f"frame_batch {frame_batch} exceeds the backbone's max_batch {backbone._max_batch}")
        self.backbone, self.head, self.device = backbone, head, head._device
        self.seq_len, self.stride, self.fuse = int(seq_len), int(stride), fuse
        self.frame_batch, self.window_batch = int(frame_batch), int(window_batch)
        self.resize_mode, self.flip_tta = int(resize_mode), bool(flip_tta)
        self.ramp = 1 + 4 * int(head.number_blocks)
        self._perm = MirrorPerm(flip_perm(head.joints_num), self.device) if self.flip_tta else None
        self._pinned: Optional[torch.Tensor] = None
        self._uploaded: Optional[torch.cuda.Event] = None
        self.stats: Dict[str, int] = {"backbone_frames": 0, "windows": 0, "head_rows": 0}

    # ---- frames -> crops -> features -----------------------------------------------------------------------------------------------
    def _upload_region(self, frames, s: int, m: int, box) -> torch.Tensor:
        """The box region of ``frames[s:s+m]`` on the device, (m, hh, ww, 3) uint8: sliced on the host into one pinned buffer (only
        these frames of a memory-mapped file are read), one asynchronous copy."""
        top, left, hh, ww = box
        if self._uploaded is not None:
            self._uploaded.synchronize()                                    # the last copy out of the buffer has finished
        if self._pinned is None or self._pinned.numel() < m * hh * ww * 3:
            self._pinned = torch.empty(m * hh * ww * 3, dtype=torch.uint8).pin_memory()
        stage = self._pinned[: m * hh * ww * 3].view(m, hh, ww, 3)
        piece = frames[s:s + m, top:top + hh, left:left + ww]
        if isinstance(piece, torch.Tensor):
            stage.copy_(piece)
        else:
            np.copyto(stage.numpy(), piece)
        region = stage.to(self.device, non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(torch.cuda.current_stream(self.device))
        return region

    def _crops(self, frames, s: int, m: int, box, dst: torch.Tensor, dst_flip: Optional[torch.Tensor]) -> None:
        """The resized crops of ``frames[s:s+m]`` into ``dst`` (m, 3, 224, 224) uint8, and mirrored into ``dst_flip``."""
        hh, ww = box[2], box[3]
        step = max(1, min(m, UPLOAD_BYTES // (hh * ww * 3)))
        for o in range(0, m, step):
            k = min(step, m - o)
            region = self._upload_region(frames, s + o, k, box)
            F.crop_and_resize_video_uint8(region, [0, 0, hh, ww], OUT_SIZE, self.resize_mode, out=dst[o:o + k])
            if dst_flip is not None:
                F.crop_and_resize_video_uint8(region, [0, 0, hh, ww], OUT_SIZE, self.resize_mode, hflip=True, out=dst_flip[o:o + k])

    def _crops_tracked(self, frames, s: int, m: int, boxes: np.ndarray, dst: torch.Tensor, dst_flip: Optional[torch.Tensor]) -> None:
        """``_crops`` with a box per frame (INTEGRATION.md section AA): ``boxes[s:s+m]`` (int64 ``[top,left,hh,ww]``, checked) are the boxes
        of ``frames[s:s+m]``.  Per chunk of at most ``UPLOAD_BYTES`` of pixels the host packs each frame's own box region back to back
        behind the chunk's table rows in the pinned buffer; one asynchronous copy carries both, one launch resizes the chunk into ``dst``
        and, mirrored, into ``dst_flip``.  Nothing waits but the next chunk's packing, on the upload event, as in ``_upload_region``."""
        from . import track as TR
        o = 0
        while o < m:
            k, nbytes = 0, 0
            while o + k < m:
                need = 3 * int(boxes[s + o + k, 2]) * int(boxes[s + o + k, 3])
                if k and nbytes + need > UPLOAD_BYTES:
                    break
                nbytes, k = nbytes + need, k + 1
            box = boxes[s + o:s + o + k]
            sizes = 3 * box[:, 2] * box[:, 3]
            offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
            local = np.stack([np.zeros(k, np.int64), np.zeros(k, np.int64), box[:, 2], box[:, 3]], axis=1)   # each region is its own image
            table = TR.BoxTable(offsets, box[:, 2:4], local, nbytes, OUT_SIZE, self.resize_mode)
            head = k * TR.TABLE_COLS * 8                                    # the table rows lead: the pixels start 8-byte aligned
            if self._uploaded is not None:
                self._uploaded.synchronize()                                # the last copy out of the buffer has finished
            if self._pinned is None or self._pinned.numel() < head + nbytes:
                self._pinned = torch.empty(head + nbytes, dtype=torch.uint8).pin_memory()
            stage = self._pinned[:head + nbytes]
            stage[:head].view(torch.int64).view(k, TR.TABLE_COLS).copy_(torch.from_numpy(table.host))
            for i in range(k):
                top, left, hh, ww = (int(v) for v in box[i])
                piece = frames[s + o + i, top:top + hh, left:left + ww]
                region = stage[head + int(offsets[i]):head + int(offsets[i]) + int(sizes[i])].view(hh, ww, 3)
                if isinstance(piece, torch.Tensor):
                    region.copy_(piece)
                else:
                    np.copyto(region.numpy(), piece)
            chunk = stage.to(self.device, non_blocking=True)
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(torch.cuda.current_stream(self.device))
            TR.crop_resize_boxes_u8(chunk[head:], table, out=dst[o:o + k], out_flip=None if dst_flip is None else dst_flip[o:o + k],
                                    table_dev=chunk[:head].view(torch.int64).view(k, TR.TABLE_COLS))
            o += k

    @staticmethod
    def _check_frames(frames) -> Tuple[int, int, int]:
        if len(frames.shape) != 4 or frames.shape[3] != 3 or frames.shape[0] < 1 or str(frames.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"frames must be (N,H,W,3) uint8 with N >= 1, got {frames.dtype} {tuple(frames.shape)}")
        if isinstance(frames, torch.Tensor) and frames.device.type != "cpu":
            raise ValueError("frames must be on the host: the box region is uploaded chunk by chunk")
        return int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])

    @torch.no_grad()
    def features(self, frames, box, boxes=None):
        """``frames``: host (N,H,W,3) uint8 array or tensor (a memory-mapped ``.npy`` is read chunk by chunk), ``box`` ``[top,left,hh,ww]``
        inside the image -> ``feats`` (N, 2048) fp32 on the device; with ``flip_tta`` ``(feats, feats_flipped)``.  Every frame goes
        through the backbone once (twice with ``flip_tta``), in calls of ``frame_batch`` frames.  With ``boxes`` (N, 4), one box per
        frame, each inside the image, ``box`` is not used and the crops come from ``_crops_tracked``."""
        n, h, w = self._check_frames(frames)
        if boxes is not None:
            from .track import check_boxes
            boxes = check_boxes(boxes, n, h, w)
        else:
            box = [int(v) for v in choose_box(h, w, box=box).tolist()]
        fb = min(self.frame_batch, n)
        with torch.cuda.device(self.device):
            feats = torch.empty((n, FEATURE_DIM), dtype=torch.float32, device=self.device)
            flipped = torch.empty_like(feats) if self.flip_tta else None
            u8 = torch.empty((fb, 3, OUT_SIZE, OUT_SIZE), dtype=torch.uint8, device=self.device)
            u8_flip = torch.empty_like(u8) if self.flip_tta else None
            for s in range(0, n, fb):
                m = min(fb, n - s)
                if boxes is not None:
                    self._crops_tracked(frames, s, m, boxes, u8[:m], u8_flip[:m] if self.flip_tta else None)
                else:
                    self._crops(frames, s, m, box, u8[:m], u8_flip[:m] if self.flip_tta else None)
                self.backbone.features_u8(u8[:m], out=feats[s:s + m])
                self.stats["backbone_frames"] += m
                if self.flip_tta:
                    self.backbone.features_u8(u8_flip[:m], out=flipped[s:s + m])
                    self.stats["backbone_frames"] += m
        return (feats, flipped) if self.flip_tta else feats

    # ---- features -> windows -> one pose per frame -----------------------------------------------------------------------------------
    @torch.no_grad()
    def poses(self, feats: torch.Tensor, feats_flipped: Optional[torch.Tensor] = None, name: str = "video"):
        """``feats`` (N, 2048) fp32 on the device [and the mirrored frames' ``feats_flipped``] -> ``(joints3d (N, J, 3) fp32, spread (N,)
        fp32, count (N,) int32)`` on the device: ``head.joints_windows`` over ``window_starts`` in batches of ``window_batch`` [merged
        with the mirrored pass], then one ``stitch_poses`` launch.  ``count`` = how many windows cover a frame, ``spread`` = how far
        their poses lie apart (0 where ``count`` is 1)."""
        if self.flip_tta != (feats_flipped is not None):
            raise ValueError("feats_flipped goes with flip_tta, and only with it")
        if feats.dim() != 2 or (feats_flipped is not None and tuple(feats_flipped.shape) != tuple(feats.shape)):
            raise ValueError("feats [and feats_flipped] must be (N, 2048)")
        n = int(feats.shape[0])
        starts = window_starts(n, self.seq_len, self.stride)
        t, w, joints = min(n, self.seq_len), int(starts.size), int(self.head.joints_num)
        table = SequenceTable.from_clips(window_clips(starts, t, name), t)
        with torch.cuda.device(self.device):
            pred = torch.empty((w, t, joints, 3), dtype=torch.float32, device=self.device)
            for s in range(0, w, self.window_batch):
                st = starts[s:s + self.window_batch]
                p = self.head.joints_windows(feats, st, t)
                self.stats["head_rows"] += int(st.size) * t
                if feats_flipped is not None:
                    q = self.head.joints_windows(feats_flipped, st, t)
                    self.stats["head_rows"] += int(st.size) * t
                    merge_mirrored_poses(p.view(-1, joints, 3), q.view(-1, joints, 3), self._perm,
                                         out=pred[s:s + st.size].view(-1, joints, 3))
                else:
                    pred[s:s + st.size] = p
            self.stats["windows"] += w
            # the stitch op wants a ground truth beside the prediction: the prediction itself, so gt_gap is 0 by construction
            fused, _, spread, _ = stitch_poses(pred, pred, StitchIndex(table.offsets, table.src, w * t, self.device), self.fuse, self.ramp)
            count = torch.from_numpy(np.diff(table.offsets).astype(np.int32)).to(self.device)
        return fused, spread, count

    @torch.no_grad()
    def forecast(self, feats: torch.Tensor, input_len: int = 15, pred_len: int = 25) -> torch.Tensor:
        """(P, J, 3) fp32 poses of the ``pred_len`` frames after the video's last: ``head.rollout`` on its last ``input_len`` frames."""
        n = int(feats.shape[0])
        if n < int(input_len):
            raise ValueError(f"forecast needs at least input_len = {input_len} frames, the video has {n}")
        return self.head.rollout(feats[None, n - int(input_len):n], int(input_len), int(pred_len))[1][0]

    @torch.no_grad()
    def predict(self, frames, box=None, joints2d=None, cam: Optional[dict] = None, frame_skip: int = 1, input_len: int = 15,
                pred_len: int = 0, name: str = "video", post=None, refine=None, conf2d=None, track=None, boxes=None,
                resample=None) -> Dict[str, object]:
        """The whole pass over every ``frame_skip``-th frame.  ``box``: see ``choose_box`` (``joints2d`` (N, J, 2) pixels of the whole
        frames, of ALL frames; the kept ones are used).  Returns host numpy arrays: ``joints3d`` (n, J, 3), ``spread`` (n,), ``count``
        (n,), ``frame_idx`` (n,) the original frame numbers, ``box`` (4,), ``future3d`` (P, J, 3) if ``pred_len > 0``, ``K`` (3, 3) of
        the resized crop if ``cam`` = ``{"f": .., "c": ..}`` was given, and ``stats``.  With ``post`` (a ``smooth.PostProcess``;
        INTEGRATION.md section W) the fused poses go through it as one sequence of one segment: ``joints3d`` holds the processed poses,
        ``joints3d_raw`` what it would hold without, ``post`` the settings and ``post_short_rows`` the frames a FIR window longer than
        the video left as they were; ``future3d`` is left as it is.  With ``refine`` (a ``refine.RefineSettings``; INTEGRATION.md
        section Z; it needs ``joints2d`` and ``cam``, and reads ``conf2d`` (N, J) if given) the fused poses are first fitted to the 2D
        joints as one sequence of one segment: ``joints3d`` holds the fitted poses (the input of ``post``, if any), ``joints3d_unrefined``
        what it would hold without, ``refine`` the settings, ``refine_energy_before`` / ``refine_energy_after`` (1, 6) the energy op's
        terms.  Without ``refine`` every launch and key is what it was.  With ``track`` (a ``track.TrackSettings``; INTEGRATION.md section
        AA) every kept frame gets its own box, ``track.track_boxes`` over the kept frames' ``joints2d``; ``boxes`` (N, 4), one box per
        frame of the whole video from a person detector, is used as given instead, each inside the image, and takes precedence over
        ``joints2d``.  Either way the crops come from one ``r50_op_crop_resize_boxes_u8`` launch per chunk, and the result gains
        ``boxes`` (n, 4) and ``track`` (the settings); ``box`` stays what ``choose_box`` gives the untracked pass (from ``joints2d`` that
        may be a square larger than the image, which the untracked pass would refuse and the tracked pass does not use), and ``K`` is
        (n, 3, 3), one per frame.  ``refine`` is untouched by it: its rays come from full-image pixels.  Without ``track`` and ``boxes`` every
        launch and key is what it was.  With ``resample`` (a ``resample.ResampleSettings``; INTEGRATION.md section AB) the poses the
        file holds (after ``refine`` and ``post``) are also interpolated at the times ``0, step, 2 step, .. <= frame_idx[-1]`` in video
        frames, as one sequence with ``max_gap = frame_skip``: the result gains ``resampled3d`` (m, J, 3), ``resampled_time`` (m,) fp64,
        ``resampled_flags`` (m,) and ``resample`` (the settings); ``joints3d`` stays aligned with ``frame_idx``.  Interpolated positions
        shorten bones between knots: where ``post`` fixes the bone lengths, ``resampled3d`` goes through ``smooth.fix_bone_lengths``
        once more; otherwise the result gains ``bone_std_mm`` and ``resampled_bone_std_mm`` (``smooth.bone_stats`` over the H36M edges, a
        17-joint head only), the spread of the bone lengths over time at the knots and after resampling.  Without ``resample`` every
        launch and key is what it was."""
        total, h, w = self._check_frames(frames)
        if track is not None and boxes is None and joints2d is None:
            raise ValueError("a box track needs boxes or joints2d")
        if refine is not None and (joints2d is None or cam is None):
            raise ValueError("the 2D fit needs joints2d and the camera's f and c")
        if int(frame_skip) < 1:
            raise ValueError(f"frame_skip must be >= 1, got {frame_skip}")
        frame_idx = np.arange(0, total, int(frame_skip), dtype=np.int64)
        kept = frames[::int(frame_skip)] if int(frame_skip) > 1 else frames
        if joints2d is not None:
            joints2d = np.asarray(joints2d)
            if joints2d.shape[0] != total:
                raise ValueError(f"joints2d covers {joints2d.shape[0]} frames, the video has {total}")
            joints2d = joints2d[frame_idx]
        if refine is not None:
            from . import refine as R
            rays = R.video_rays(joints2d, cam, int(self.head.joints_num))          # refused here, before any launch, if they do not fit
            if conf2d is not None:
                conf2d = np.asarray(conf2d)
                if conf2d.shape[0] != total:
                    raise ValueError(f"conf2d covers {conf2d.shape[0]} frames, the video has {total}")
                conf2d = conf2d[frame_idx]
        box_t = choose_box(h, w, box=box, joints2d=joints2d)
        if boxes is not None:
            from .track import check_boxes
            boxes = check_boxes(boxes, total, h, w)[frame_idx]
        elif track is not None:
            boxes = track.boxes(joints2d, h, w).numpy()
        self.stats = {"backbone_frames": 0, "windows": 0, "head_rows": 0}
        got = self.features(kept, box_t, boxes) if boxes is not None else self.features(kept, box_t)
        feats, flipped = got if self.flip_tta else (got, None)
        joints3d, spread, count = self.poses(feats, flipped, name)
        unrefined = None
        if refine is not None:
            with torch.cuda.device(self.device):
                unrefined, (joints3d, fit) = joints3d, R.refine_video(joints3d, rays, conf2d, refine)
        out: Dict[str, object] = {"joints3d": joints3d.cpu().numpy(), "spread": spread.cpu().numpy(), "count": count.cpu().numpy(),
                                  "frame_idx": frame_idx, "box": box_t.numpy().copy()}
        if refine is not None:
            out["joints3d_unrefined"], out["refine"] = unrefined.cpu().numpy(), np.array(refine.describe())
            out["refine_energy_before"], out["refine_energy_after"] = fit["energy_before"].cpu().numpy(), fit["energy_after"].cpu().numpy()
        if post is not None:
            n = int(joints3d.shape[0])
            with torch.cuda.device(self.device):
                processed, info = post.apply(joints3d, (np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32)))
            out["joints3d_raw"], out["joints3d"] = out["joints3d"], processed.cpu().numpy()
            out["post"], out["post_short_rows"] = np.array(post.describe()), np.int64(info["short_rows"][0].item())
            joints3d = processed
        if resample is not None:
            out.update(self._resampled(joints3d, frame_idx, int(frame_skip), resample, post))
        if int(pred_len) > 0:
            out["future3d"] = self.forecast(feats, input_len, pred_len).cpu().numpy()
        if boxes is not None:
            out["boxes"], out["track"] = boxes.copy(), np.array("boxes as given" if track is None else track.describe())
        if cam is not None and boxes is not None:
            out["K"] = np.stack([F.adjust_camera_after_crop_and_resize(cam, torch.from_numpy(b), OUT_SIZE).numpy() for b in boxes])
        elif cam is not None:
            out["K"] = F.adjust_camera_after_crop_and_resize(cam, box_t, OUT_SIZE).numpy()
        out["stats"] = dict(self.stats)
        return out

    def _resampled(self, joints3d: torch.Tensor, frame_idx: np.ndarray, frame_skip: int, settings, post) -> Dict[str, object]:
        """The keys ``predict`` gains with ``resample``: see there."""
        from . import resample as RS
        from . import smooth
        with torch.cuda.device(self.device):
            y, flags, tau = RS.resample_video(joints3d, frame_idx, frame_skip, settings)
            m, joints = int(y.shape[0]), int(y.shape[1])
            one = lambda rows: (np.array([0, rows], dtype=np.int32), np.arange(rows, dtype=np.int32))          # noqa: E731
            extra: Dict[str, object] = {}
            if post is not None and post.fix_bones:
                y, _ = smooth.fix_bone_lengths(y, smooth.DeviceTables(*one(m), self.device), post.edges)
            elif int(np.max(smooth.H36M_EDGES)) < joints:
                for key, poses in (("bone_std_mm", joints3d), ("resampled_bone_std_mm", y)):
                    rows = int(poses.shape[0])
                    stats = smooth.bone_stats(poses.contiguous(), smooth.DeviceTables(*one(rows), self.device)).cpu().numpy()
                    extra[key] = np.float64(smooth.bone_std_mm(stats, np.array([rows]), np.array([0]), 1)[1])
            return {"resampled3d": y.cpu().numpy(), "resampled_time": tau, "resampled_flags": flags.cpu().numpy(),
                    "resample": np.array(settings.describe()), **extra}

    @torch.no_grad()
    def crops(self, frames, box, first: int, count: int, step: int = 1, boxes=None) -> torch.Tensor:
        """The resized crops of the frames ``first, first + step, ..`` (``count`` of them) as pictures: (count, 224, 224, 3) uint8 on the
        device (what ``render`` draws on).  The frames are a strided slice, so they travel in the same few pieces as in ``features``.
        ``boxes`` (count, 4): one box per picture instead of ``box``."""
        total, h, w = self._check_frames(frames)
        first, count, step = int(first), int(count), int(step)
        if count < 1 or step < 1 or first < 0 or first + (count - 1) * step >= total:
            raise ValueError(f"frames {first}, {first + step}, .. ({count} of them) do not lie inside a video of {total} frames")
        if boxes is not None:
            from .track import check_boxes
            boxes = check_boxes(boxes, count, h, w)
        else:
            box = [int(v) for v in choose_box(h, w, box=box).tolist()]
        with torch.cuda.device(self.device):
            chw = torch.empty((count, 3, OUT_SIZE, OUT_SIZE), dtype=torch.uint8, device=self.device)
            if boxes is not None:
                self._crops_tracked(frames[first:first + (count - 1) * step + 1:step], 0, count, boxes, chw, None)
            else:
                self._crops(frames[first:first + (count - 1) * step + 1:step], 0, count, box, chw, None)
            return chw.permute(0, 2, 3, 1).contiguous()


# ---- command line ---------------------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser("Decoded video frames in, one 3D pose per frame out (backbone + lifting head on one MI355X)")
    p.add_argument("--frames", type=str, nargs="+", required=True, metavar="FILE",
                   help=".npy of (N,H,W,3) uint8 frames (memory-mapped), or .npz with `frames` and optionally `box` [top,left,hh,ww], "
                        "`boxes` (N,4) for --track, `joints2d` (N,J,2) and the camera's `f`, `c`")
    p.add_argument("--model_path", type=str, required=True, help="head checkpoint (its dimensions are read from it)")
    p.add_argument("--weights-from", choices=("auto", "model", "ema"), default="auto",
                   help="which weights of --model_path to use: auto = the EMA weights when the checkpoint has them, else the raw ones")
    p.add_argument("--weights", type=str, default=None, help="local torchvision-layout ResNet-50 checkpoint")
    p.add_argument("--synthetic-weights", action="store_true", help="seeded RANDOM backbone weights: for benchmarks / tests only")
    p.add_argument("--weights-seed", type=int, default=0)
    p.add_argument("--precision", choices=["bf16", "fp16", "bf16w2", "fp32x", "fp8"], default="bf16", help="backbone precision")
    p.add_argument("--head-precision", choices=("fp16", "bf16"), default="fp16", help="16-bit type of the head's GEMMs")
    p.add_argument("--seq-len", type=int, default=40, help="frames per head window")
    p.add_argument("--stride", type=int, default=5, help="frames between window starts")
    p.add_argument("--frame-skip", type=int, default=2, help="every this-many-th frame is used: the cadence heads are trained at")
    p.add_argument("--fuse", choices=sorted(FUSE_MODES), default="context", help="how a frame's windows are fused")
    p.add_argument("--flip-tta", action="store_true", help="flip test-time augmentation: every frame also mirrored, the poses merged")
    p.add_argument("--input-len", type=int, default=15, help="observed frames of the forecast")
    p.add_argument("--pred-len", type=int, default=0, help="poses to forecast beyond the last frame (0: none)")
    p.add_argument("--box", type=int, nargs=4, default=None, metavar=("TOP", "LEFT", "H", "W"), help="crop box (overrides the file's)")
    p.add_argument("--resize-mode", choices=sorted(RESIZE_MODES), default="float", help="bilinear resize arithmetic")
    p.add_argument("--frame-batch", type=int, default=256, help="frames per backbone call")
    p.add_argument("--window-batch", type=int, default=256, help="windows per head call")
    p.add_argument("--out", type=str, required=True, metavar="DIR", help="one NAME_poses.npz per input")
    p.add_argument("--render", action="store_true", help="also NAME_render/: an APNG and a contact sheet of the last frames")
    p.add_argument("--render-frames", type=int, default=120, help="how many of the last frames to render")
    p.add_argument("--render-fps", type=float, default=10.0)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--smooth", choices=("gauss", "savgol", "one_euro"), default=argparse.SUPPRESS,
                   help="filter the fused poses along time on the device before they are written and rendered (INTEGRATION.md section W); "
                        "the file keeps the unprocessed poses as joints3d_raw")
    p.add_argument("--fix-bones", action="store_true", default=argparse.SUPPRESS,
                   help="give every bone its mean length over the video, after the filter (INTEGRATION.md section W)")
    from .smooth import add_parameter_flags
    add_parameter_flags(p)
    p.add_argument("--bvh", action="store_true", default=argparse.SUPPRESS,
                   help="also joint rotations on a rigid skeleton (INTEGRATION.md section Y): NAME.bvh beside NAME_poses.npz, which gains "
                        "the rotations, the rest offsets and the rigid reconstruction")
    from .kinematics import add_bvh_flags
    add_bvh_flags(p)
    p.add_argument("--refine-2d", action="store_true", default=argparse.SUPPRESS,
                   help="fit the fused poses to the input's 2D joints under a temporal prior before --smooth / --fix-bones / --bvh "
                        "(INTEGRATION.md section Z); the .npz input must hold `joints2d` and the camera's `f`, `c` (`conf2d` (N,J) is "
                        "read if present); the file keeps the unfitted poses as joints3d_unrefined")
    from .refine import add_parameter_flags as add_refine_flags
    add_refine_flags(p)
    p.add_argument("--track", action="store_true", default=argparse.SUPPRESS,
                   help="a crop box per frame that follows the person (INTEGRATION.md section AA): the .npz input's `boxes` (N,4) as "
                        "given, else the box of the clip around each frame from its `joints2d`; the file gains `boxes` and a K per frame")
    p.add_argument("--track-window", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="frames of the clip around a frame whose joints give its box (default: --seq-len); needs --track")
    p.add_argument("--track-smooth", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="frames of the running mean over the boxes' extents (default: the track window; 1: none); needs --track")
    from .resample import add_video_flags
    add_video_flags(p)
    return p


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    """``build_parser().parse_args`` plus the check that a filter's parameter flags come with that filter (``--smooth``)."""
    p = build_parser()
    args = p.parse_args(argv)
    video_post(args, p.error)
    from .kinematics import bvh_options
    for flag in ("bvh_fps", "bvh_scale"):
        if hasattr(args, flag) and not hasattr(args, "bvh"):
            p.error(f"--{flag.replace('_', '-')} needs --bvh")
    bvh_options(args, p.error)
    video_refine(args, p.error)
    video_track(args, p.error)
    video_resample(args, p.error)
    return args


def video_post(args: argparse.Namespace, error=None):
    """The ``smooth.PostProcess`` of parsed arguments, or None without ``--smooth`` / ``--fix-bones``."""
    from .smooth import post_from_args

    def raise_(msg):
        raise ValueError(msg)
    return post_from_args(args, getattr(args, "smooth", None), getattr(args, "fix_bones", False), error or raise_)


def video_refine(args: argparse.Namespace, error=None):
    """The ``refine.RefineSettings`` of parsed arguments, or None without ``--refine-2d``."""
    from .refine import settings_from_args

    def raise_(msg):
        raise ValueError(msg)
    return settings_from_args(args, hasattr(args, "refine_2d"), "--refine-2d", error or raise_)


def video_track(args: argparse.Namespace, error=None):
    """The ``track.TrackSettings`` of parsed arguments (the window defaults to ``--seq-len``), or None without ``--track``."""
    from .track import TrackSettings

    def raise_(msg):
        raise ValueError(msg)
    error = error or raise_
    for flag in ("track_window", "track_smooth"):
        if hasattr(args, flag) and not hasattr(args, "track"):
            error(f"--{flag.replace('_', '-')} needs --track")
    if not hasattr(args, "track"):
        return None
    try:
        return TrackSettings(getattr(args, "track_window", args.seq_len), getattr(args, "track_smooth", None))
    except ValueError as exc:
        error(f"--track: {exc}")


def video_resample(args: argparse.Namespace, error=None):
    """The ``resample.ResampleSettings`` of parsed arguments, or None without ``--resample``."""
    from .resample import settings_from_args

    def raise_(msg):
        raise ValueError(msg)
    return settings_from_args(args, error or raise_)


def load_input(path: str) -> Dict[str, object]:
    """``frames`` (memory-mapped for a ``.npy``) and whatever annotations the file holds: ``box``, ``boxes``, ``joints2d``, ``conf2d``,
    ``cam``."""
    if path.endswith(".npz"):
        z = np.load(path, allow_pickle=False)
        if "frames" not in z.files:
            raise ValueError(f"{path}: no `frames` array in the file (it holds {sorted(z.files)}); expected (N,H,W,3) uint8 frames")
        item: Dict[str, object] = {"frames": z["frames"]}
        for key in ("box", "boxes", "joints2d", "conf2d"):
            if key in z.files:
                item[key] = z[key]
        if ("f" in z.files) != ("c" in z.files):
            raise ValueError(f"{path}: the camera needs both `f` and `c`")
        if "f" in z.files:
            item["cam"] = {"f": z["f"], "c": z["c"]}
        return item
    if path.endswith(".npy"):
        return {"frames": np.load(path, mmap_mode="r")}
    raise ValueError(f"{path}: expected a .npy or .npz file")


def render_prediction(outdir: str, predictor: VideoPredictor, frames, res: Dict[str, object], n_frames: int, fps: float) -> List[str]:
    """The last ``n_frames`` kept frames with their poses, then the forecast (if any) on the plain background, through ``render``."""
    from . import render as R
    dev = predictor.device
    n = int(res["joints3d"].shape[0])
    r = max(1, min(int(n_frames), n))
    idx = res["frame_idx"]
    tracked = "boxes" in res
    pics = predictor.crops(frames, res["box"], int(idx[n - r]), r, int(idx[1] - idx[0]) if n > 1 else 1,
                           **({"boxes": res["boxes"][n - r:]} if tracked else {}))
    pred = torch.from_numpy(res["joints3d"][n - r:]).to(dev)
    future = None
    if "future3d" in res:
        future = torch.from_numpy(res["future3d"]).to(dev)[None]
        blank = torch.tensor(R._rgb_tuple(R.PANEL_BG_RGB), dtype=torch.uint8, device=dev).expand(future.shape[1], OUT_SIZE, OUT_SIZE, 3)
        pics = torch.cat([pics, blank])
        # placeholders, never drawn: render_panels puts future3d in the prediction layer of every frame t >= input_len = r
        pred = torch.cat([pred, torch.zeros_like(future[0])])
    k = torch.from_numpy(res["K"]).to(dev)[None] if "K" in res else None
    if k is not None and tracked:                # a K per frame, (1, T, 3, 3); the forecast's placeholders keep the last frame's
        k = k[:, n - r:]
        if future is not None:
            k = torch.cat([k, k[:, -1:].expand(1, int(future.shape[1]), 3, 3)], dim=1)
    return R.render_clips(outdir, pics[None], None, k, None, pred[None], future, r, None, fps)


def main(argv: Optional[List[str]] = None) -> List[str]:
    args = parse_args(argv)
    post = video_post(args)
    fit = video_refine(args)
    follow = video_track(args)
    again = video_resample(args)
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.R50Error("predict runs on an MI355X only; there is no CPU fallback")
    from .backbone import ResNet50Backbone
    from .preprocess_resnet_features import _resolve_weights
    from .results import build_head, load_head_state
    head_state = load_head_state(args.model_path, args.weights_from)
    bvh = hasattr(args, "bvh")
    if bvh:
        from . import kinematics
        from .results import infer_head_dims
        kinematics.skeleton_for(infer_head_dims(head_state)[1])    # another joint count has no built-in skeleton: refused before any launch
        bvh_fps, bvh_scale = kinematics.bvh_options(args, None)
    items = [load_input(p) for p in args.frames]
    if fit is not None:                      # refused before the backbone is built
        for path, item in zip(args.frames, items):
            if "joints2d" not in item or "cam" not in item:
                raise ValueError(f"{path}: --refine-2d needs `joints2d` and the camera's `f` and `c` in the input .npz")
    if follow is not None:                   # likewise
        for path, item in zip(args.frames, items):
            if "boxes" not in item and "joints2d" not in item:
                raise ValueError(f"{path}: --track needs `boxes` (N,4) or `joints2d` (N,J,2) in the input .npz")
    state_dict, source = _resolve_weights(args)
    print(f"backbone weights: {source}")
    backbone = ResNet50Backbone(state_dict=state_dict, max_batch=args.frame_batch, precision=args.precision).to(device).eval()
    head = build_head(head_state, backbone._device, args.head_precision)
    predictor = VideoPredictor(backbone, head, args.seq_len, args.stride, args.fuse, args.frame_batch, args.window_batch,
                               RESIZE_MODES[args.resize_mode], args.flip_tta)
    os.makedirs(args.out, exist_ok=True)
    written: List[str] = []
    for path, item in zip(args.frames, items):
        name = os.path.splitext(os.path.basename(path))[0]
        res = predictor.predict(item["frames"], box=args.box if args.box is not None else item.get("box"), joints2d=item.get("joints2d"),
                                cam=item.get("cam"), frame_skip=args.frame_skip, input_len=args.input_len, pred_len=args.pred_len, name=name,
                                **({} if post is None else {"post": post}),
                                **({} if fit is None else {"refine": fit, "conf2d": item.get("conf2d")}),
                                **({} if follow is None else {"track": follow, "boxes": item.get("boxes")}),
                                **({} if again is None else {"resample": again}))
        stats = res.pop("stats")
        out_path = os.path.join(args.out, name + "_poses.npz")
        rigid_note = ""
        if bvh:                              # after the optional --smooth / --fix-bones / --resample: the poses the file holds, as one sequence
            res.update(kinematics.video_rotations(res["joints3d" if again is None else "resampled3d"], device))
            rigid_note = (f", rigid skeleton: mean residual {float(res['rigid_residual'].mean()):.6f} "
                          f"({int(np.count_nonzero(res['rigid_flags']))} flagged frames)")
        np.savez(out_path, **res, **{k: np.int64(v) for k, v in stats.items()})
        written.append(out_path)
        print(f"{name}: {res['joints3d'].shape[0]} poses from {stats['backbone_frames']} backbone frames, {stats['windows']} windows "
              f"({stats['head_rows']} head rows) -> {out_path}" + rigid_note)
        if bvh:
            # resampled poses lie STEP video frames apart, the kept ones FRAME_SKIP: the frame time is STEP / (FRAME_SKIP * bvh_fps)
            fps = bvh_fps if again is None else bvh_fps * args.frame_skip / again.step
            written.append(kinematics.write_video_bvh(os.path.join(args.out, name + ".bvh"), res, None, fps, bvh_scale))
            print(f"{name}: BVH written to: {written[-1]}")
        if args.render:
            written += render_prediction(os.path.join(args.out, name + "_render"), predictor, item["frames"], res, args.render_frames,
                                         args.render_fps)
    backbone.close()
    return written


if __name__ == "__main__":
    main()
