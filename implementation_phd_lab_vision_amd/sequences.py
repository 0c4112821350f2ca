"""Dense evaluation: the overlapping clips of a feature cache stitched back into one pose per video frame.

The features CLI cuts each video into clips of ``seq_len`` sub-sampled frames at a stride smaller than ``seq_len``, so a video frame
lies in several clips, at another window position in each, and every clip-wise evaluation counts it once per clip and scores as many
different predictions of it.  Every index entry carries ``subject, action, cam, start, end`` in sub-sampled frame units, so
``(subject, action, cam, f)`` names a video frame and the clips that cover it are known on the host:

* ``SequenceTable.from_clips`` builds that table with numpy (no GPU): the sequences, their frames, and per frame the list of its
  contributors ``item * T + t`` in ascending clip ``start`` order;
* ``stitch_poses`` (``r50_op_stitch_poses``, gather form: one wave per output frame, no atomics) fuses the contributors of every
  frame into one pose -- ``mean``, ``context`` (a contributor at window position t weighs ``min(t + 1, ramp)``, ``ramp`` = f_movie's
  receptive field: a prediction that has seen more past counts more) or ``last`` (the contributor with the most past) -- and
  reports how far the contributors lie apart (``spread``) and whether their ground truths agree (``gt_gap``, 0 when the index is right);
* ``sequence_metrics`` (``r50_op_sequence_metrics``) sums P1, the velocity and acceleration errors and the spread per action over the
  stitched frames, every video frame once; P2 is the existing ``r50_op_pose_protocols`` on the stitched frames seen as clips of one
  frame;
* ``evaluate_dense`` runs the pass over a ``DeviceFeatureStore``.

A sequence is keyed ``(int(subject), str(action), str(cam))``: ``1`` and ``"1"`` name one camera, ``"cam_1"`` another.  Read as fp32,
computed in fp64, the same bits on every run.  No CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from . import protocols
from .protocols import MAX_JOINTS, ROOT_JOINT

FUSE_MODES = {"mean": 0, "context": 1, "last": 2}
METRIC_SLOTS = 8                              # r50_op_sequence_metrics: doubles per (block, group)
METRIC_BLOCK_ROWS = 256                       # frame rows per workgroup of the metrics launch


def sequence_key(clip: dict) -> Tuple[int, str, str]:
    return int(clip["subject"]), str(clip["action"]), str(clip["cam"])


@dataclass
class SequenceChunk:
    """A run of whole sequences: ``items`` (ascending item indices, the order of the chunk's pred buffer), the chunk's own table
    (``src`` counts rows of that buffer), and where the run starts in the full table (``seq0`` sequences, ``frame0`` frame rows)."""
    items: np.ndarray
    table: "SequenceTable"
    seq0: int
    frame0: int


@dataclass
class SequenceTable:
    """F frame rows of S sequences over N clips of T frames (all int32): ``seq`` (F,) and ``idx`` (F,) = a row's sequence and
    sub-frame index, ``seq_start`` (S+1,) = the rows of sequence s are ``seq_start[s]:seq_start[s+1]``, ``seq_keys`` [S] sorted
    ``(subject, action, cam)``, and the contributors of row r: ``src[offsets[r]:offsets[r+1]]``, each ``item * T + t``, in ascending
    clip ``start`` order (descending t; clips with one start by item index).  ``item_seq`` (N,) = a clip's sequence."""
    seq: np.ndarray
    idx: np.ndarray
    seq_start: np.ndarray
    seq_keys: List[Tuple[int, str, str]]
    offsets: np.ndarray
    src: np.ndarray
    item_seq: np.ndarray
    seq_len: int

    @property
    def frames(self) -> int:
        return int(self.seq.shape[0])

    @property
    def clips(self) -> int:
        return int(self.item_seq.shape[0])

    @classmethod
    def from_clips(cls, clips: Sequence[dict], seq_len: int) -> "SequenceTable":
        t = int(seq_len)
        n = len(clips)
        if t < 1 or n < 1:
            raise ValueError(f"need seq_len >= 1 and at least one clip (got {t}, {n})")
        if n * t >= 2 ** 31:
            raise ValueError(f"{n} clips of {t} frames exceed the int32 row index")
        starts = np.empty(n, dtype=np.int64)
        keys = []
        for i, c in enumerate(clips):
            s, e = int(c["start"]), int(c["end"])
            if e - s != t:
                raise ValueError(f"clip {i} covers frames [{s}, {e}), not seq_len = {t} of them")
            starts[i] = s
            keys.append(sequence_key(c))
        seq_keys = sorted(set(keys))
        pos = {k: s for s, k in enumerate(seq_keys)}
        item_seq = np.array([pos[k] for k in keys], dtype=np.int64)
        item = np.repeat(np.arange(n, dtype=np.int64), t)
        tt = np.tile(np.arange(t, dtype=np.int64), n)
        frame = starts[item] + tt
        sq = item_seq[item]
        order = np.lexsort((item, starts[item], frame, sq))                    # by sequence, frame, clip start, item
        sq, frame = sq[order], frame[order]
        new = np.ones(n * t, dtype=bool)
        new[1:] = (sq[1:] != sq[:-1]) | (frame[1:] != frame[:-1])
        first = np.flatnonzero(new)
        seq = sq[first]
        return cls(seq=seq.astype(np.int32), idx=frame[first].astype(np.int32),
                   seq_start=np.searchsorted(seq, np.arange(len(seq_keys) + 1)).astype(np.int32), seq_keys=seq_keys,
                   offsets=np.append(first, n * t).astype(np.int32), src=(item * t + tt)[order].astype(np.int32),
                   item_seq=item_seq.astype(np.int32), seq_len=t)

    def chunks(self, max_clips: int) -> List[SequenceChunk]:
        """Consecutive runs of whole sequences with at most ``max_clips`` clips each; a longer sequence is a run of its own."""
        if max_clips < 1:
            raise ValueError("max_clips must be >= 1")
        per_seq = np.bincount(self.item_seq, minlength=len(self.seq_keys))
        bounds, total = [0], 0
        for s, c in enumerate(per_seq):
            if total and total + c > max_clips:
                bounds.append(s)
                total = 0
            total += int(c)
        bounds.append(len(self.seq_keys))
        t = self.seq_len
        out = []
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            items = np.flatnonzero((self.item_seq >= s0) & (self.item_seq < s1))
            f0, f1 = int(self.seq_start[s0]), int(self.seq_start[s1])
            o0, o1 = int(self.offsets[f0]), int(self.offsets[f1])
            src = self.src[o0:o1].astype(np.int64)
            local = np.searchsorted(items, src // t) * t + src % t
            table = SequenceTable(seq=self.seq[f0:f1] - np.int32(s0), idx=self.idx[f0:f1].copy(),
                                  seq_start=self.seq_start[s0:s1 + 1] - np.int32(f0), seq_keys=self.seq_keys[s0:s1],
                                  offsets=self.offsets[f0:f1 + 1] - np.int32(o0), src=local.astype(np.int32),
                                  item_seq=self.item_seq[items] - np.int32(s0), seq_len=t)
            out.append(SequenceChunk(items=items, table=table, seq0=int(s0), frame0=f0))
        return out


class StitchIndex:
    """``offsets`` (F+1,) and ``src`` int32 host arrays checked on the host -- the kernel trusts them -- and uploaded once: offsets
    non-decreasing from 0 to ``len(src)``, every ``src`` in ``[0, rows)``."""

    def __init__(self, offsets, src, rows: int, device):
        offsets, src = np.asarray(offsets), np.asarray(src)
        if offsets.dtype != np.int32 or src.dtype != np.int32 or offsets.ndim != 1 or src.ndim != 1:
            raise ValueError(f"offsets and src must be 1-D int32 arrays, got {offsets.dtype} {offsets.shape}, {src.dtype} {src.shape}")
        if offsets.size < 2:
            raise ValueError("offsets needs at least one frame (two entries)")
        if offsets[0] != 0 or offsets[-1] != src.size or np.any(np.diff(offsets.astype(np.int64)) < 0):
            raise ValueError(f"offsets must be non-decreasing from 0 to len(src) = {src.size}")
        if src.size and (int(src.min()) < 0 or int(src.max()) >= rows):
            raise ValueError(f"every src must lie in [0, {rows}), got [{int(src.min())}, {int(src.max())}]")
        self.rows = int(rows)
        self.frames = int(offsets.size - 1)
        self.offsets = torch.from_numpy(np.ascontiguousarray(offsets)).to(device)
        self.src = torch.from_numpy(np.ascontiguousarray(src)).to(device) if src.size else torch.zeros(1, dtype=torch.int32, device=device)


def stitch_poses(pred: torch.Tensor, gt: torch.Tensor, index: Union[StitchIndex, Tuple[np.ndarray, np.ndarray]],
                 mode: Union[int, str] = "context", ramp: int = 1, out: Optional[Sequence[torch.Tensor]] = None):
    """One ``r50_op_stitch_poses`` launch: pred, gt (N, T, J, 3) fp32 on one GPU, ``index`` a ``StitchIndex`` over N*T rows or the
    host arrays ``(offsets, src)`` to make one from; ``mode`` 0 / 1 / 2 or ``mean`` / ``context`` / ``last``.  Returns ``(fused
    (F, J, 3), gt_out (F, J, 3), spread (F,), gt_gap (F,))`` fp32; ``out``: those four, contiguous, with at least F rows each (the
    first F are written).  Everything is checked on the host before the launch."""
    mode = FUSE_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if mode not in (0, 1, 2):
        raise ValueError(f"mode must be 0, 1, 2 or one of {sorted(FUSE_MODES)}, got {mode!r}")
    if int(ramp) < 1:
        raise ValueError(f"ramp must be >= 1, got {ramp}")
    if pred.dim() != 4 or pred.shape[3] != 3 or tuple(gt.shape) != tuple(pred.shape) or pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError(f"pred and gt (N,T,J,3) fp32 expected, got {tuple(pred.shape)} {pred.dtype}, {tuple(gt.shape)} {gt.dtype}")
    n, t, j, _ = pred.shape
    if not 1 <= j <= MAX_JOINTS or n < 1 or t < 1:
        raise ValueError(f"need N, T >= 1 and 1 <= J <= {MAX_JOINTS} (got N={n}, T={t}, J={j})")
    if pred.device.type != "cuda" or pred.device != gt.device:
        raise ValueError("pred and gt must be on one GPU: there is no CPU fallback")
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise ValueError("pred and gt must be contiguous")
    if not isinstance(index, StitchIndex):
        index = StitchIndex(index[0], index[1], n * t, pred.device)
    if index.rows != n * t or index.offsets.device != pred.device:
        raise ValueError(f"the index was checked for {index.rows} rows on {index.offsets.device}, pred has {n * t} on {pred.device}")
    f = index.frames
    shapes = ((f, j, 3), (f, j, 3), (f,), (f,))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=pred.device) for s in shapes)
    else:
        out = tuple(out)
        if len(out) != 4:
            raise ValueError("out must be (fused, gt_out, spread, gt_gap)")
        for o, s in zip(out, shapes):
            if (o.dtype != torch.float32 or o.device != pred.device or not o.is_contiguous() or o.dim() != len(s) or o.shape[0] < f
                    or tuple(o.shape[1:]) != s[1:]):
                raise ValueError(f"each of out must be contiguous fp32 on {pred.device} with at least {f} rows of {s[1:]}, got "
                                 f"{tuple(o.shape)} {o.dtype}")
    rc = _lib.load_library().r50_op_stitch_poses(pred.data_ptr(), gt.data_ptr(), n * t, j, index.offsets.data_ptr(), index.src.data_ptr(), f,
                                                 t, int(mode), int(ramp), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                 out[3].data_ptr(), torch.cuda.current_stream(pred.device).cuda_stream)
    _lib.check(rc, None, "r50_op_stitch_poses")
    return out


def sequence_metrics(fused: torch.Tensor, gt: torch.Tensor, spread: torch.Tensor, offsets: torch.Tensor, seq: torch.Tensor,
                     idx: torch.Tensor, group: torch.Tensor, n_groups: int, root: int = ROOT_JOINT,
                     n_blocks: Optional[int] = None) -> torch.Tensor:
    """One ``r50_op_sequence_metrics`` launch over F stitched frames: fused, gt (F, J, 3) and spread (F,) fp32, offsets (F+1,), seq, idx
    and group (F,) int32, all contiguous on one GPU; the group VALUES are the caller's to have checked.  Returns ``part`` (n_blocks,
    n_groups, 8) fp64 on the device, every slot written: ``part.sum(0)`` in block order is [frames, sum P1, velocity terms, sum velocity
    error, acceleration terms, sum acceleration error, sum spread, frames with >= 2 contributors] per group."""
    if fused.dim() != 3 or fused.shape[2] != 3 or tuple(gt.shape) != tuple(fused.shape) or fused.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError(f"fused and gt (F,J,3) fp32 expected, got {tuple(fused.shape)} {fused.dtype}, {tuple(gt.shape)} {gt.dtype}")
    f, j, _ = fused.shape
    if f < 1 or not 1 <= j <= MAX_JOINTS or not 0 <= root < j or n_groups < 1:
        raise ValueError(f"need F, n_groups >= 1, 1 <= J <= {MAX_JOINTS} and 0 <= root < J (got F={f}, J={j}, root={root}, n_groups={n_groups})")
    if spread.dtype != torch.float32 or tuple(spread.shape) != (f,):
        raise ValueError(f"spread must be ({f},) fp32, got {tuple(spread.shape)} {spread.dtype}")
    for name, v, size in (("offsets", offsets, f + 1), ("seq", seq, f), ("idx", idx, f), ("group", group, f)):
        if v.dtype != torch.int32 or tuple(v.shape) != (size,):
            raise ValueError(f"{name} must be ({size},) int32, got {tuple(v.shape)} {v.dtype}")
    every = (fused, gt, spread, offsets, seq, idx, group)
    if fused.device.type != "cuda" or any(v.device != fused.device for v in every):
        raise ValueError("every argument must be on one GPU: there is no CPU fallback")
    if not all(v.is_contiguous() for v in every):
        raise ValueError("every argument must be contiguous")
    n_blocks = (f + METRIC_BLOCK_ROWS - 1) // METRIC_BLOCK_ROWS if n_blocks is None else int(n_blocks)
    if n_blocks < 1:
        raise ValueError("n_blocks must be >= 1")
    part = torch.empty((n_blocks, int(n_groups), METRIC_SLOTS), dtype=torch.float64, device=fused.device)
    rc = _lib.load_library().r50_op_sequence_metrics(fused.data_ptr(), gt.data_ptr(), spread.data_ptr(), offsets.data_ptr(), seq.data_ptr(),
                                                     idx.data_ptr(), group.data_ptr(), f, j, int(root), int(n_groups), part.data_ptr(),
                                                     n_blocks, torch.cuda.current_stream(fused.device).cuda_stream)
    _lib.check(rc, None, "r50_op_sequence_metrics")
    return part


def sum_blocks(part: np.ndarray) -> np.ndarray:
    """(n_blocks, G, 8) -> (G, 8): the blocks added one after the other, in block order, in fp64."""
    total = np.zeros(part.shape[1:], dtype=np.float64)
    for b in range(part.shape[0]):
        total += part[b]
    return total


def _ratio(a, b):
    """a / b in fp64, NaN where b is 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)


def _defined_mean(v: np.ndarray) -> float:
    """The plain mean over the defined (non-NaN) entries; NaN where there is none."""
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float("nan")


def metric_values(sums: np.ndarray, p2_sums: np.ndarray) -> Dict[str, object]:
    """The per-group, ``_all`` and ``_mean`` values from the (G, 8) sums of ``r50_op_sequence_metrics`` and the (G,) P2 sums."""
    out: Dict[str, object] = {"frames": sums[:, 0].round().astype(np.int64), "frames_all": int(round(sums[:, 0].sum()))}
    tot = sums.sum(axis=0)
    for name, num, den, num_all, den_all in (("p1", sums[:, 1], sums[:, 0], tot[1], tot[0]),
                                             ("p2", p2_sums, sums[:, 0], p2_sums.sum(), tot[0]),
                                             ("mpjve", sums[:, 3], sums[:, 2], tot[3], tot[2]),
                                             ("accel", sums[:, 5], sums[:, 4], tot[5], tot[4]),
                                             ("spread", sums[:, 6], sums[:, 0], tot[6], tot[0])):
        out[name] = _ratio(num, den)
        out[name + "_all"] = float(_ratio(num_all, den_all))
        out[name + "_mean"] = _defined_mean(out[name])
    out["multi_frames"] = int(round(tot[7]))
    return out


@torch.no_grad()
def evaluate_dense(head, store, fuse: str = "context", batch_size: int = 256, chunk_clips: int = 8192,
                   keep_poses: bool = False, post=None) -> Dict[str, object]:
    """Every video frame of ``store`` (a ``DeviceFeatureStore`` without ``augment``) scored once: ``head.joints`` over every clip, the
    clips of each sequence fused per frame (``fuse``: ``mean``, ``context`` with ramp ``1 + 4 * head.number_blocks``, ``last``) and the
    fused frames scored per action.  Sequences are taken in runs of at most ``chunk_clips`` clips (a sequence is never split); per run
    ``store.get_batch`` / ``head.joints`` in batches of ``batch_size`` into one buffer, then one stitch, one metrics and one protocols
    launch; the sums are read once per pass.  Returns (metres, metres per frame, metres per frame^2; fp64), with M one of ``p1``,
    ``p2``, ``mpjve``, ``accel``, ``spread``::

        group_names [G], frames (G,) int64, frames_all, M (G,), M_all, M_mean (the plain mean over the groups where M is defined)
        clip_frames = clips * T, multi_frames (frames with >= 2 contributors), sequences, fuse, ramp
        position_p1 (T,), position_p2 (T,): the clip-wise errors by window position over all clips
        with keep_poses: seq_keys [S], seq_start (S+1,), frame_idx (F,), pred (F, J, 3), gt (F, J, 3), frame_spread (F,), count (F,)

    With ``post`` (a ``smooth.PostProcess``) each run's fused poses also go through ``post.apply`` -- a
    sequence is never split across runs, so this is exact -- and the processed poses are scored by the same metrics and protocols
    launches next to the raw ones; still one read of the sums per pass.  The result gains, for M in ``p1``, ``p2``, ``mpjve``, ``accel``::

        post_M (G,), post_M_all, post_M_mean, post (what was applied, whether it is causal and its look-ahead R)
        bone_std_raw, bone_std_post, bone_std_gt (G,) and *_all: the bone-length standard deviation over time in mm (smooth.bone_std_mm)
        post_short_rows, post_short_segments: frames the FIR copied because their segment is shorter than its window
        with keep_poses: pred_post (F, J, 3)

    Without ``post`` the pass is what it was: the same launches, the same bits.

    Raises ValueError if any frame's contributors disagree on the ground truth (a wrong index)."""
    if getattr(store, "augment", False):
        raise ValueError("dense evaluation takes variant 0 only: open the store without augment")
    if fuse not in FUSE_MODES:
        raise ValueError(f"fuse must be one of {sorted(FUSE_MODES)}, got {fuse!r}")
    if batch_size < 1 or chunk_clips < 1:
        raise ValueError("batch_size and chunk_clips must be >= 1")
    clips = store.item_clips()
    t = int(store.feats.shape[1])
    table = SequenceTable.from_clips(clips, t)
    group_names = sorted({protocols.action_name(k[1]) for k in table.seq_keys})
    gpos = {a: g for g, a in enumerate(group_names)}
    seq_group = np.array([gpos[protocols.action_name(k[1])] for k in table.seq_keys], dtype=np.int32)
    n_groups, joints, ramp = len(group_names), int(head.joints_num), 1 + 4 * int(head.number_blocks)
    dev = head._device
    parts, kept = [], []
    post_parts, post_stats, post_short = [], [], []
    if post is not None:
        from . import smooth
    chunks = table.chunks(chunk_clips)
    with torch.cuda.device(dev):
        acc_pos = torch.zeros(2 * t + 1, dtype=torch.float64, device=dev)             # the protocols op over the clips, one group
        acc_p2 = torch.zeros(3 * n_groups, dtype=torch.float64, device=dev)            # the protocols op over the stitched frames, P = 1
        gap = torch.zeros(1, dtype=torch.float64, device=dev)
        acc_p2_post = torch.zeros(3 * n_groups, dtype=torch.float64, device=dev) if post is not None else None
        for chunk in chunks:
            tbl, n = chunk.table, len(chunk.items)
            pred = torch.empty((n, t, joints, 3), dtype=torch.float32, device=dev)
            gt = torch.empty((n, t, joints, 3), dtype=torch.float32, device=dev)
            for s in range(0, n, batch_size):
                batch = store.get_batch(chunk.items[s:s + batch_size].tolist())
                pred[s:s + batch_size] = head.joints(batch[0])
                gt[s:s + batch_size] = batch[1].to(device=dev, dtype=torch.float32)
            index = StitchIndex(tbl.offsets, tbl.src, n * t, dev)
            fused, gt_out, spread, gt_gap = stitch_poses(pred, gt, index, FUSE_MODES[fuse], ramp)
            group = torch.from_numpy(seq_group[chunk.seq0 + tbl.seq]).to(dev)
            parts.append(sequence_metrics(fused, gt_out, spread, index.offsets, torch.from_numpy(tbl.seq).to(dev),
                                          torch.from_numpy(tbl.idx).to(dev), group, n_groups).reshape(-1))
            f = tbl.frames
            protocols._launch(fused.view(f, 1, joints, 3), gt_out.view(f, 1, joints, 3), 0, group, n_groups, acc_p2, ROOT_JOINT)
            protocols._launch(pred, gt, 0, torch.zeros(n, dtype=torch.int32, device=dev), 1, acc_pos, ROOT_JOINT)
            gap = torch.maximum(gap, gt_gap.max().to(torch.float64).reshape(1))     # a NaN stays
            fused_post = None
            if post is not None:
                fused_post, info = post.apply(fused, tbl)
                dt = info["tables"]
                post_parts.append(sequence_metrics(fused_post, gt_out, spread, index.offsets, torch.from_numpy(tbl.seq).to(dev),
                                                   torch.from_numpy(tbl.idx).to(dev), group, n_groups).reshape(-1))
                protocols._launch(fused_post.view(f, 1, joints, 3), gt_out.view(f, 1, joints, 3), 0, group, n_groups, acc_p2_post, ROOT_JOINT)
                post_stats.append(torch.stack([smooth.bone_stats(v, dt, post.edges) for v in (fused, fused_post, gt_out)]).reshape(-1))
                post_short.append(info["short_rows"].to(torch.float64))
            if keep_poses:
                kept.append((fused, gt_out, spread) + ((fused_post,) if post is not None else ()))
        n_part = sum(int(v.numel()) for v in parts)
        host = torch.cat([acc_pos, acc_p2, gap] + parts + ([acc_p2_post] + post_parts + post_stats + post_short if post is not None else [])
                         ).cpu().numpy()
        if keep_poses:
            poses = [torch.cat([k[i] for k in kept]).cpu().numpy() for i in range(3 if post is None else 4)]
    head_n = 2 * t + 2 + 3 * n_groups
    pos, p2, worst, part, tail = np.split(host, [2 * t + 1, 2 * t + 1 + 3 * n_groups, head_n, head_n + n_part])
    if not worst[0] == 0.0:
        raise ValueError(f"contributors of one video frame disagree on its ground truth by up to {worst[0]} m: the index entries do not "
                         "name the frames the shards hold")
    out: Dict[str, object] = {"group_names": group_names, "fuse": fuse, "ramp": ramp, "sequences": len(table.seq_keys),
                              "clip_frames": table.clips * t}
    out.update(metric_values(sum_blocks(part.reshape(-1, n_groups, METRIC_SLOTS)), p2[:2 * n_groups].reshape(n_groups, 2)[:, 1]))
    by_pos = pos[:2 * t].reshape(t, 2) / pos[2 * t]
    out["position_p1"], out["position_p2"] = by_pos[:, 0].copy(), by_pos[:, 1].copy()
    if keep_poses:
        out.update(seq_keys=list(table.seq_keys), seq_start=table.seq_start.copy(), frame_idx=table.idx.copy(), pred=poses[0], gt=poses[1],
                   frame_spread=poses[2], count=np.diff(table.offsets).astype(np.int32))
    if post is not None:
        n_edges = len(post.edges)
        n_stats = 3 * len(table.seq_keys) * n_edges * smooth.STAT_SLOTS
        p2_post, part_post, stats, short = np.split(tail, [3 * n_groups, 3 * n_groups + n_part, 3 * n_groups + n_part + n_stats])
        vals = metric_values(sum_blocks(part_post.reshape(-1, n_groups, METRIC_SLOTS)), p2_post[:2 * n_groups].reshape(n_groups, 2)[:, 1])
        for m in ("p1", "p2", "mpjve", "accel"):
            for suffix in ("", "_all", "_mean"):
                out["post_" + m + suffix] = vals[m + suffix]
        # the runs hold whole sequences in table order: run c's block is (3, S_c, E, 2)
        by_kind, at = [[], [], []], 0
        for chunk in chunks:
            n = len(chunk.table.seq_keys) * n_edges * smooth.STAT_SLOTS
            for k in range(3):
                by_kind[k].append(stats[at + k * n: at + (k + 1) * n].reshape(-1, n_edges, smooth.STAT_SLOTS))
            at += 3 * n
        seq_rows = np.diff(table.seq_start)
        for k, name in enumerate(("raw", "post", "gt")):
            per, over = smooth.bone_std_mm(np.concatenate(by_kind[k]), seq_rows, seq_group, n_groups)
            out["bone_std_" + name], out["bone_std_" + name + "_all"] = per, over
        short = short.reshape(-1, 2).sum(axis=0)
        out["post_short_rows"], out["post_short_segments"] = int(round(short[0])), int(round(short[1]))
        out["post"] = post.describe()
        if keep_poses:
            out["pred_post"] = poses[3]
    return out


def dense_lines(res: Dict[str, object]) -> List[str]:
    """The printed lines of ``--dense`` from an ``evaluate_dense`` result, each starting with ``Dense |``: the summary (all frames and
    the action mean), one line per action, and the clip-wise P1 / P2 at window positions 1, T/2 and T.  Millimetres."""
    def summary(key: str) -> str:
        return (f"p1 (mm) {res['p1' + key] * 1000.0:.2f} | p2 (mm) {res['p2' + key] * 1000.0:.2f} | vel (mm/frame) "
                f"{res['mpjve' + key] * 1000.0:.2f} | accel (mm/frame^2) {res['accel' + key] * 1000.0:.2f} | spread (mm) "
                f"{res['spread' + key] * 1000.0:.2f}")

    lines = [f"Dense | fuse {res['fuse']} (ramp {res['ramp']}) | sequences {res['sequences']} | frames {res['frames_all']} of "
             f"{res['clip_frames']} clip frames | fused from >= 2 clips {res['multi_frames']} | all: {summary('_all')} | action mean: "
             f"{summary('_mean')}"]
    for i, name in enumerate(res["group_names"]):
        lines.append(f"Dense |   {name} | frames {int(res['frames'][i])} | p1 (mm) {res['p1'][i] * 1000.0:.2f} | p2 (mm) "
                     f"{res['p2'][i] * 1000.0:.2f} | vel (mm/frame) {res['mpjve'][i] * 1000.0:.2f} | accel (mm/frame^2) "
                     f"{res['accel'][i] * 1000.0:.2f} | spread (mm) {res['spread'][i] * 1000.0:.2f}")
    p1, p2 = res["position_p1"], res["position_p2"]
    at = sorted({1, max(len(p1) // 2, 1), len(p1)})
    lines.append("Dense | clip-wise by window position | p1 (mm) " + " | ".join(f"@{k}: {p1[k - 1] * 1000.0:.2f}" for k in at) +
                 " | p2 (mm) " + " | ".join(f"@{k}: {p2[k - 1] * 1000.0:.2f}" for k in at))
    return lines


def dense_post_lines(res: Dict[str, object]) -> List[str]:
    """The ``Dense | post`` lines of an ``evaluate_dense`` result that carries ``post``: raw -> processed over all frames and per
    action, errors in millimetres and the bone-length standard deviation over time of the raw, processed and ground-truth poses."""
    def pair(m: str, key, i=None) -> str:
        a, b = res[m + key], res["post_" + m + key]
        a, b = (a, b) if i is None else (a[i], b[i])
        return f"{a * 1000.0:.2f} -> {b * 1000.0:.2f}"

    def row(key: str, i=None) -> str:
        std = [res[f"bone_std_{k}{'_all' if i is None else ''}"] for k in ("raw", "post", "gt")]
        std = [v if i is None else v[i] for v in std]
        return (f"p1 (mm) {pair('p1', key, i)} | p2 (mm) {pair('p2', key, i)} | vel (mm/frame) {pair('mpjve', key, i)} | accel (mm/frame^2) "
                f"{pair('accel', key, i)} | bone std (mm) {std[0]:.3f} -> {std[1]:.3f} (gt {std[2]:.3f})")

    lines = [f"Dense | post {res['post']} | frames copied (segment shorter than the window) {res['post_short_rows']} in "
             f"{res['post_short_segments']} segments | raw -> processed, all: {row('_all')}"]
    for i, name in enumerate(res["group_names"]):
        lines.append(f"Dense | post   {name} | {row('', i)}")
    return lines


def dense_npz(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``.npz`` keys of ``--dense``: ``dense_actions`` (G,) str, ``dense_frames`` (G,) int64, ``dense_M`` (G,) and ``dense_M_all`` ()
    fp32 for M in p1, p2, mpjve, accel, spread (metres, metres per frame, metres per frame^2), ``dense_position_p1`` / ``_p2`` (T,) fp32,
    ``dense_counts`` int64 [sequences, frames, clip frames, frames fused from >= 2 clips], ``dense_fuse`` str."""
    out = {"dense_actions": np.array([str(n) for n in res["group_names"]], dtype=str),
           "dense_frames": np.asarray(res["frames"], dtype=np.int64), "dense_fuse": np.array(str(res["fuse"])),
           "dense_counts": np.array([res["sequences"], res["frames_all"], res["clip_frames"], res["multi_frames"]], dtype=np.int64),
           "dense_position_p1": np.asarray(res["position_p1"], dtype=np.float32),
           "dense_position_p2": np.asarray(res["position_p2"], dtype=np.float32)}
    for m in ("p1", "p2", "mpjve", "accel", "spread"):
        out["dense_" + m] = np.asarray(res[m], dtype=np.float32)
        out["dense_" + m + "_all"] = np.asarray(res[m + "_all"], dtype=np.float32)
    if "post" in res:                        # --dense-smooth / --dense-fix-bones: dense_post_M, dense_post_bone_std_{raw,post,gt} (mm), ...
        out["dense_post"] = np.array(str(res["post"]))
        out["dense_post_short"] = np.array([res["post_short_rows"], res["post_short_segments"]], dtype=np.int64)
        for m in ("p1", "p2", "mpjve", "accel"):
            out["dense_post_" + m] = np.asarray(res["post_" + m], dtype=np.float32)
            out["dense_post_" + m + "_all"] = np.asarray(res["post_" + m + "_all"], dtype=np.float32)
        for k in ("raw", "post", "gt"):
            out["dense_post_bone_std_" + k] = np.asarray(res["bone_std_" + k], dtype=np.float32)
            out["dense_post_bone_std_" + k + "_all"] = np.asarray(res["bone_std_" + k + "_all"], dtype=np.float32)
    return out


def dense_export(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The arrays of ``--dense-out``: ``seq_keys`` (S, 3) str [subject, action, cam], ``seq_start`` (S+1,), ``frame_idx`` (F,) int32
    (sub-sampled frame units), ``pred`` and ``gt`` (F, J, 3) fp32 in metres, ``spread`` (F,) fp32, ``count`` (F,) int32 = the clips
    that showed the frame; sequence s is rows ``seq_start[s]:seq_start[s+1]``."""
    out = {"seq_keys": np.array([[str(v) for v in k] for k in res["seq_keys"]], dtype=str), "seq_start": res["seq_start"],
           "frame_idx": res["frame_idx"], "pred": res["pred"], "gt": res["gt"], "spread": res["frame_spread"], "count": res["count"]}
    if "pred_post" in res:                   # --dense-smooth / --dense-fix-bones: the processed poses beside the raw ones, and what made them
        out["pred_post"], out["post"] = res["pred_post"], np.array(str(res["post"]))
    return out
