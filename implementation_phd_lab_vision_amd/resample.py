"""A pose at any time stamp from the rows around it, for stitched per-frame pose sequences (INTEGRATION.md section AB,
include/r50_resample.h).

The head runs at the cadence it was trained at (every ``--frame-skip``-th frame), and the stitch, the 2D fit, the filters, the bone step
and the BVH export inherit that cadence.  This module is the stage after them: linear or cubic Hermite interpolation inside the runs of
a sequence whose stamps lie at most ``max_gap`` apart, the nearer knot inside a break and the end row outside a sequence, both flagged.

* ``ResampleTable`` checks the four index tables on the host -- the kernel trusts them -- and uploads them once;
* ``left_rows`` is ``out_left`` by its definition; ``uniform_times`` the times of a uniform clock that skips the breaks;
* ``resample_sequences`` is the one ``r50_op_resample_sequences`` launch;
* ``ResampleSettings`` / ``resample_video`` are what ``predict --resample`` runs;
* ``holdout_table`` / ``evaluate_holdout`` / ``holdout_lines`` / ``holdout_npz`` answer what ``results --dense --dense-holdout K`` asks:
  how much accuracy is lost when only every K-th row is computed and the rows in between are interpolated.

fp32 in and out, fp64 in between, one rounding at the store, the same bits on every run.  No CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

MAX_JOINTS = 64                               # the op's limits (include/r50_resample.h)
MAX_ROWS = (2 ** 31 - 1) // 192
KINDS = {"linear": 0, "cubic": 1}
FLAG_IN_BREAK, FLAG_OUTSIDE = 1, 2
FLAG_NAMES = ("in a break", "outside the sequence")


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def _check_sequences(seq_start, idx) -> Tuple[np.ndarray, np.ndarray]:
    seq_start, idx = np.asarray(seq_start), np.asarray(idx)
    if seq_start.ndim != 1 or idx.ndim != 1 or seq_start.size < 2 or not np.issubdtype(seq_start.dtype, np.integer) or \
            not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("seq_start (S+1,) and idx (F,) must be 1-D integer arrays with at least one sequence")
    ss, ix = seq_start.astype(np.int64), idx.astype(np.int64)
    f = int(ix.size)
    if ss[0] != 0 or ss[-1] != f or np.any(np.diff(ss) < 1):
        raise ValueError(f"seq_start must rise strictly from 0 to len(idx) = {f} (every sequence has at least one row)")
    if f > MAX_ROWS:
        raise ValueError(f"too many rows: {f} > {MAX_ROWS}")
    if f and (int(ix.min()) < -2 ** 31 or int(ix.max()) >= 2 ** 31):
        raise ValueError("the stamps must fit int32")
    falls = np.diff(ix) <= 0
    falls[ss[1:-1] - 1] = False                                                   # a new sequence may start anywhere
    if falls.any():
        r = int(np.flatnonzero(falls)[0])
        raise ValueError(f"the stamps must be strictly increasing inside a sequence: idx[{r}] = {int(ix[r])} is followed by {int(ix[r + 1])}")
    return ss, ix


def left_rows(seq_start, idx, out_time, out_seq) -> np.ndarray:
    """``out_left`` (G,) int32 by its definition: per output row the last row i of its sequence with ``idx[i] <= tau``, or the
    sequence's first row where ``tau`` lies before it."""
    ss, ix = np.asarray(seq_start, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    tau, seq = np.asarray(out_time, dtype=np.float64), np.asarray(out_seq, dtype=np.int64)
    out = np.empty(tau.size, dtype=np.int32)
    order = np.argsort(seq, kind="stable")
    bounds = np.searchsorted(seq[order], np.arange(ss.size))
    for s in range(ss.size - 1):
        rows = order[bounds[s]:bounds[s + 1]]
        if rows.size:
            a, b = int(ss[s]), int(ss[s + 1])
            pos = np.searchsorted(ix[a:b].astype(np.float64), tau[rows], side="right") - 1
            out[rows] = a + np.maximum(pos, 0)
    return out


class ResampleTable:
    """The tables of one resampling, checked on the host -- the kernel trusts them -- and uploaded once per device: ``seq_start`` (S+1,),
    ``idx`` (F,) strictly increasing inside a sequence, ``out_time`` (G,) finite fp64, ``out_seq`` (G,) in ``[0, S)`` and ``out_left``
    (G,) what ``left_rows`` gives (computed when not given; refused when given and different)."""

    def __init__(self, seq_start, idx, out_time, out_seq, out_left=None):
        ss, ix = _check_sequences(seq_start, idx)
        tau, seq = np.asarray(out_time), np.asarray(out_seq)
        if tau.ndim != 1 or seq.ndim != 1 or tau.size < 1 or tau.size != seq.size or not np.issubdtype(seq.dtype, np.integer) or \
                tau.dtype.kind not in "fiu":
            raise ValueError(f"out_time (G,) numbers and out_seq (G,) integers with G >= 1 expected, got {tau.shape} {tau.dtype}, "
                             f"{seq.shape} {seq.dtype}")
        if tau.size > MAX_ROWS:
            raise ValueError(f"too many output rows: {tau.size} > {MAX_ROWS}")
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        if not np.isfinite(tau).all():
            raise ValueError(f"every output time must be finite: out_time[{int(np.flatnonzero(~np.isfinite(tau))[0])}] is not")
        n_seq = int(ss.size - 1)
        if int(seq.min()) < 0 or int(seq.max()) >= n_seq:
            raise ValueError(f"every out_seq entry must lie in [0, {n_seq}), got [{int(seq.min())}, {int(seq.max())}]")
        want = left_rows(ss, ix, tau, seq)
        if out_left is not None:
            given = np.asarray(out_left)
            if given.shape != want.shape or not np.issubdtype(given.dtype, np.integer):
                raise ValueError(f"out_left must be ({want.size},) integers, got {given.shape} {given.dtype}")
            wrong = np.flatnonzero(given.astype(np.int64) != want)
            if wrong.size:
                g = int(wrong[0])
                raise ValueError(f"out_left[{g}] = {int(given[g])} is not the last row of sequence {int(seq[g])} with idx <= "
                                 f"{float(tau[g])!r} (that is row {int(want[g])}); {wrong.size} such rows")
        self.seq_start, self.idx = ss.astype(np.int32), ix.astype(np.int32)
        self.out_time, self.out_seq, self.out_left = tau, np.ascontiguousarray(seq, dtype=np.int32), want
        self.rows, self.sequences, self.outputs = int(ix.size), n_seq, int(tau.size)
        self._dev: Dict[str, Tuple[torch.Tensor, ...]] = {}

    def on(self, device) -> Tuple[torch.Tensor, ...]:
        """``(idx, seq_start, out_time, out_seq, out_left)`` on ``device``, uploaded on first use."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.idx, self.seq_start, self.out_time, self.out_seq,
                                                                            self.out_left))
        return self._dev[key]

    def bridged(self, max_gap: int) -> np.ndarray:
        """(G,) bool: the output rows that lie on a knot or inside a bridged interval, so that their flag is 0."""
        i, tau = self.out_left.astype(np.int64), self.out_time
        ix = self.idx.astype(np.int64)
        last = self.seq_start.astype(np.int64)[self.out_seq.astype(np.int64) + 1] - 1
        nxt = np.minimum(i + 1, last)
        on_knot = tau == ix[i]
        return on_knot | ((tau > ix[i]) & (i < last) & (ix[nxt] - ix[i] <= int(max_gap)))


def uniform_times(seq_start, idx, step: float, max_gap: int, phase: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """``(out_time (G,) fp64, out_seq (G,) int32)``: per sequence the times ``idx[first] + phase + k * step`` (k = 0, 1, ..; each formed
    from k, not accumulated) up to ``idx[last]``.  Times that fall strictly inside a break (an interval longer than ``max_gap``) are left
    out, so every row has flag 0.  ``step > 0``, ``phase >= 0``, both finite.  A sequence may get no time at all (G may be 0)."""
    ss, ix = _check_sequences(seq_start, idx)
    step, phase, max_gap = float(step), float(phase), int(max_gap)
    if not (math.isfinite(step) and step > 0.0 and math.isfinite(phase) and phase >= 0.0):
        raise ValueError(f"need a finite step > 0 and a finite phase >= 0, got {step}, {phase}")
    if max_gap < 1:
        raise ValueError(f"max_gap must be >= 1, got {max_gap}")
    times, seqs = [], []
    for s in range(ss.size - 1):
        t = ix[ss[s]:ss[s + 1]].astype(np.float64)
        start = t[0] + phase
        if start > t[-1]:
            continue
        n = int(math.floor((t[-1] - start) / step)) + 1
        tau = start + np.arange(n + 1, dtype=np.float64) * step                  # one more, then cut: the floor above may be one short
        tau = tau[tau <= t[-1]]
        i = np.searchsorted(t, tau, side="right") - 1
        nxt = np.minimum(i + 1, t.size - 1)
        keep = (tau == t[i]) | (t[nxt] - t[i] <= max_gap)
        times.append(tau[keep])
        seqs.append(np.full(int(keep.sum()), s, dtype=np.int32))
    if not times:
        return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int32)
    return np.concatenate(times), np.concatenate(seqs)


# ---- the op -----------------------------------------------------------------------------------------------------------------------------------
def _kind_id(kind) -> int:
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    return KINDS[kind]


def resample_sequences(x: torch.Tensor, table: ResampleTable, kind: str = "cubic", max_gap: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``r50_op_resample_sequences`` launch: x (F, J, 3) fp32 on a GPU, the rows of ``table`` -> ``(y (G, J, 3) fp32, flags (G,)
    int32)`` on that GPU.  ``flags``: bit 0 = the time lies inside a break (the nearer knot was copied), bit 1 = it lies outside the
    sequence (the end row was copied).  Nothing waits for the GPU.  There is no CPU fallback."""
    if not isinstance(table, ResampleTable):
        raise ValueError("table must be a ResampleTable: the kernel trusts what it has checked")
    kind_id, max_gap = _kind_id(kind), int(max_gap)
    if max_gap < 1:
        raise ValueError(f"max_gap must be >= 1, got {max_gap}")
    if x.dim() != 3 or x.shape[2] != 3 or x.dtype != torch.float32:
        raise ValueError(f"resample_sequences: poses (F, J, 3) fp32 expected, got {tuple(x.shape)} {x.dtype}")
    f, j, _ = x.shape
    if f != table.rows or not 1 <= j <= MAX_JOINTS:
        raise ValueError(f"resample_sequences: the table holds {table.rows} rows, the poses {f}; need 1 <= J <= {MAX_JOINTS} (got {j})")
    if x.device.type != "cuda":
        raise ValueError("resample_sequences: the poses must be on a GPU: there is no CPU fallback")
    if not x.is_contiguous():
        raise ValueError("resample_sequences: poses must be contiguous")
    with torch.cuda.device(x.device):
        idx, seq_start, out_time, out_seq, out_left = table.on(x.device)
        y = torch.empty((table.outputs, j, 3), dtype=torch.float32, device=x.device)
        flags = torch.empty(table.outputs, dtype=torch.int32, device=x.device)
        rc = _lib.load_library().r50_op_resample_sequences(x.data_ptr(), idx.data_ptr(), seq_start.data_ptr(), f, table.sequences, j,
                                                           out_time.data_ptr(), out_seq.data_ptr(), out_left.data_ptr(), table.outputs,
                                                           kind_id, max_gap, y.data_ptr(), flags.data_ptr(),
                                                           torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, None, "r50_op_resample_sequences")
    return y, flags


# ---- one video (``predict --resample``) ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ResampleSettings:
    """``step``: the output spacing in video frames (> 0; 1 = a pose for every frame of the video); ``kind``: ``linear`` or ``cubic``."""
    step: float
    kind: str = "cubic"

    def __post_init__(self):
        step = float(self.step)
        if not (math.isfinite(step) and step > 0.0):
            raise ValueError(f"the step must be finite and > 0, got {self.step!r}")
        _kind_id(self.kind)
        object.__setattr__(self, "step", step)

    def describe(self) -> str:
        return f"step={self.step:g} kind={self.kind}"

    def times(self, frame_idx) -> np.ndarray:
        """``0, step, 2 step, .. <= frame_idx[-1]`` in video frames (fp64), each formed from its count."""
        last = float(np.asarray(frame_idx)[-1])
        n = int(math.floor(last / self.step)) + 1
        tau = np.arange(n + 1, dtype=np.float64) * self.step
        return tau[tau <= last]


def resample_video(joints3d: torch.Tensor, frame_idx, frame_skip: int, settings: ResampleSettings) -> Tuple[torch.Tensor, torch.Tensor, np.ndarray]:
    """The poses of one video (n, J, 3) on the device, at the stamps ``frame_idx``, as one sequence bridged throughout (``max_gap =
    frame_skip``) -> ``(resampled (m, J, 3), flags (m,), times (m,) fp64 host)``."""
    frame_idx = np.asarray(frame_idx)
    n = int(frame_idx.size)
    tau = settings.times(frame_idx)
    table = ResampleTable(np.array([0, n], dtype=np.int32), frame_idx, tau, np.zeros(tau.size, dtype=np.int32))
    y, flags = resample_sequences(joints3d.contiguous(), table, settings.kind, max(1, int(frame_skip)))
    return y, flags, tau


def add_video_flags(parser) -> None:
    """``--resample`` and ``--resample-kind``; absent from the namespace unless given."""
    import argparse
    parser.add_argument("--resample", type=float, default=argparse.SUPPRESS, metavar="STEP",
                        help="also poses every STEP video frames (> 0; 1 = every frame of the video, FRAME_SKIP * 25 / 30 = 30 fps), "
                             "interpolated after --refine-2d / --smooth / --fix-bones and before --bvh (INTEGRATION.md section AB): the "
                             "file gains resampled3d, resampled_time, resampled_flags")
    parser.add_argument("--resample-kind", choices=sorted(KINDS), default=argparse.SUPPRESS,
                        help="how --resample interpolates (default cubic: Hermite with three-point tangents); needs --resample")


def settings_from_args(args, error) -> Optional[ResampleSettings]:
    """The ``ResampleSettings`` of ``predict``'s parsed arguments, or None without ``--resample``."""
    if hasattr(args, "resample_kind") and not hasattr(args, "resample"):
        error("--resample-kind needs --resample")
    if not hasattr(args, "resample"):
        return None
    try:
        return ResampleSettings(args.resample, getattr(args, "resample_kind", "cubic"))
    except ValueError as exc:
        error(f"--resample: {exc}")


# ---- what interpolating between every K-th row costs: the dense pass ------------------------------------------------------------------------
def holdout_table(seq_start, idx, k: int) -> Tuple[np.ndarray, ResampleTable]:
    """``(keep (F,) bool, table)``: per sequence the kept rows are those whose stamp is ``k * n`` past the first stamp of their segment
    (``smooth.segment_table``) and every segment's last row.  ``table`` resamples the KEPT rows (F_k of them, in order) at the stamps of
    ALL rows, so a held-out row lies inside an interval of at most ``k`` frames between two kept rows of its own segment."""
    from .smooth import segment_table
    k = int(k)
    if k < 2:
        raise ValueError(f"the holdout keeps every K-th row with K >= 2, got {k}")
    ss, ix = _check_sequences(seq_start, idx)
    seg_start, row_seg = segment_table(ss, ix)
    first = seg_start[:-1].astype(np.int64)[row_seg]
    keep = (ix - ix[first]) % k == 0
    keep[seg_start[1:].astype(np.int64) - 1] = True
    seq = np.repeat(np.arange(ss.size - 1, dtype=np.int32), np.diff(ss))
    kept_start = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(np.int64), ss[:-1]))])
    return keep, ResampleTable(kept_start, ix[keep], ix.astype(np.float64), seq)


@torch.no_grad()
def evaluate_holdout(dense: Dict[str, object], k: int, kind: str = "cubic", device="cuda", keep: bool = False) -> Dict[str, object]:
    """``dense`` is the result of ``sequences.evaluate_dense(keep_poses=True)``; of its ``pred_post`` where a post-process ran, else its
    ``pred``, only the rows of ``holdout_table`` are kept and all rows are rebuilt from them (stamps ``frame_idx``, ``max_gap = k``).
    The held-out rows alone are scored against ``gt`` by the protocols launch, at full rate and interpolated; all rows go through the
    sequence-metrics launch, the distance between the interpolated and the full-rate pose in the spread slot; the sums are read once.
    Returns (metres; fp64)::

        holdout_full_M / holdout_M (G,), *_all, *_mean      M in p1, p2: the held-out rows alone, full rate / interpolated
        holdout_M (G,), holdout_M_all, holdout_M_mean       M in mpjve, accel: all rows, interpolated (beside M or post_M of ``dense``)
        holdout_distance (G,), holdout_distance_all         mean joint distance interpolated <-> full rate over all rows
        holdout_rows (G,) int64, holdout_rows_all           the held-out rows;  holdout_kept_all  the kept ones
        holdout_flagged (2,) int64                          rows with flag bit 0, 1 set: 0 by construction
        holdout (the settings);  with keep: pred_holdout (F, J, 3)
    """
    from . import protocols, sequences
    missing = [m for m in ("seq_keys", "seq_start", "frame_idx", "pred", "gt", "group_names", "count") if m not in dense]
    if missing:
        raise ValueError(f"the dense result lacks {missing}: run evaluate_dense with keep_poses=True")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("evaluate_holdout runs on a GPU: there is no CPU fallback")
    _kind_id(kind)
    single = np.ascontiguousarray(dense["pred_post"] if "pred_post" in dense else dense["pred"], dtype=np.float32)
    f, joints = int(single.shape[0]), int(single.shape[1])
    seq_keys, seq_start, frame_idx = dense["seq_keys"], np.asarray(dense["seq_start"]).astype(np.int64), np.asarray(dense["frame_idx"])
    kept_mask, table = holdout_table(seq_start, frame_idx, k)
    group_names = list(dense["group_names"])
    gpos = {a: g for g, a in enumerate(group_names)}
    seq_group = np.array([gpos[protocols.action_name(key[1])] for key in seq_keys], dtype=np.int32)
    n_groups, n_seq = len(group_names), len(seq_keys)
    seq = np.repeat(np.arange(n_seq, dtype=np.int32), np.diff(seq_start))
    held = np.flatnonzero(~kept_mask)
    h = int(held.size)
    with torch.cuda.device(device):
        full = torch.from_numpy(single).to(device)
        gt = torch.from_numpy(np.ascontiguousarray(dense["gt"], dtype=np.float32)).to(device)
        source = full.index_select(0, torch.from_numpy(np.flatnonzero(kept_mask)).to(device))
        interp, flags = resample_sequences(source, table, kind, int(k))
        distance = (interp - full).norm(dim=2).mean(dim=1)
        group = torch.from_numpy(seq_group[seq]).to(device)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(np.asarray(dense["count"]), dtype=np.int64)]).astype(np.int32)).to(device)
        part = sequences.sequence_metrics(interp, gt, distance, offsets, torch.from_numpy(seq).to(device),
                                          torch.from_numpy(np.ascontiguousarray(frame_idx, dtype=np.int32)).to(device), group, n_groups)
        acc = torch.zeros((2, 3 * n_groups), dtype=torch.float64, device=device)
        if h:
            rows = torch.from_numpy(held).to(device)
            gt_h, group_h = gt.index_select(0, rows).view(h, 1, joints, 3), group.index_select(0, rows)
            for slot, poses in enumerate((full, interp)):
                protocols._launch(poses.index_select(0, rows).view(h, 1, joints, 3), gt_h, 0, group_h, n_groups, acc[slot], protocols.ROOT_JOINT)
        bits = torch.stack([((flags >> b) & 1).sum() for b in range(2)]).to(torch.float64)
        host = torch.cat([acc.reshape(-1), part.reshape(-1), bits]).cpu().numpy()
        kept = {"pred_holdout": interp.cpu().numpy()} if keep else {}
    acc, part, bits = np.split(host, [6 * n_groups, host.size - 2])
    acc = acc.reshape(2, 3 * n_groups)
    vals = sequences.metric_values(sequences.sum_blocks(part.reshape(-1, n_groups, sequences.METRIC_SLOTS)), np.zeros(n_groups))
    out: Dict[str, object] = dict(kept)
    counts = acc[0, 2 * n_groups:]                                                  # the protocols launch counts the rows of a group
    for slot, prefix in enumerate(("holdout_full_", "holdout_")):
        sums = acc[slot, :2 * n_groups].reshape(n_groups, 2)
        for col, m in enumerate(("p1", "p2")):
            per = sequences._ratio(sums[:, col], counts)
            out[prefix + m], out[prefix + m + "_all"] = per, float(sequences._ratio(sums[:, col].sum(), counts.sum()))
            out[prefix + m + "_mean"] = sequences._defined_mean(per)
    for m in ("mpjve", "accel"):
        for suffix in ("", "_all", "_mean"):
            out["holdout_" + m + suffix] = vals[m + suffix]
    out["holdout_distance"], out["holdout_distance_all"] = vals["spread"], vals["spread_all"]
    out["holdout_rows"], out["holdout_rows_all"] = counts.round().astype(np.int64), h
    out["holdout_kept_all"] = int(kept_mask.sum())
    out["holdout_flagged"] = bits.round().astype(np.int64)
    out["holdout"] = f"K={int(k)} kind={kind}"
    return out


def holdout_lines(dense: Dict[str, object], res: Dict[str, object]) -> List[str]:
    """The ``Dense | holdout`` lines: full rate -> interpolated over all frames and per action (mm), the held-out and the flagged rows."""
    single = "post_" if "pred_post" in dense else ""

    def held(m: str, key: str, i=None) -> str:
        a, b = res["holdout_full_" + m + key], res["holdout_" + m + key]
        a, b = (a, b) if i is None else (a[i], b[i])
        return f"{a * 1000.0:.2f} -> {b * 1000.0:.2f}"

    def every(m: str, key: str, i=None) -> str:
        a, b = dense[single + m + key], res["holdout_" + m + key]
        a, b = (a, b) if i is None else (a[i], b[i])
        return f"{a * 1000.0:.2f} -> {b * 1000.0:.2f}"

    def row(key: str, i=None) -> str:
        d = res["holdout_distance" + key]
        d = d if i is None else d[i]
        n = res["holdout_rows_all"] if i is None else res["holdout_rows"][i]
        return (f"held-out rows {int(n)} | p1 (mm) {held('p1', key, i)} | p2 (mm) {held('p2', key, i)} | all rows: vel (mm/frame) "
                f"{every('mpjve', key, i)} | accel (mm/frame^2) {every('accel', key, i)} | distance (mm) {d * 1000.0:.2f}")

    lines = [f"Dense | holdout {res['holdout']} (section AB) | kept rows {int(res['holdout_kept_all'])} | flagged rows " +
             ", ".join(f"{name} {int(n)}" for name, n in zip(FLAG_NAMES, res["holdout_flagged"])) +
             f" | full rate -> interpolated, all: {row('_all')}"]
    for i, name in enumerate(dense["group_names"]):
        lines.append(f"Dense | holdout   {name} | {row('', i)}")
    lines.append(f"Dense | holdout   action mean | p1 (mm) {held('p1', '_mean')} | p2 (mm) {held('p2', '_mean')} | all rows: vel (mm/frame) "
                 f"{every('mpjve', '_mean')} | accel (mm/frame^2) {every('accel', '_mean')}")
    return lines


def holdout_npz(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``dense_holdout_*`` keys of the result ``.npz``: ``dense_holdout_M`` (G,) and ``dense_holdout_M_all`` () fp32 for M in full_p1,
    full_p2, p1, p2, mpjve, accel, distance; ``dense_holdout_rows`` (G,), ``dense_holdout_flagged`` (2,) int64; ``dense_holdout`` (the
    settings)."""
    out = {"dense_holdout": np.array(str(res["holdout"])), "dense_holdout_rows": np.asarray(res["holdout_rows"], dtype=np.int64),
           "dense_holdout_flagged": np.asarray(res["holdout_flagged"], dtype=np.int64)}
    for m in ("full_p1", "full_p2", "p1", "p2", "mpjve", "accel", "distance"):
        out["dense_holdout_" + m] = np.asarray(res["holdout_" + m], dtype=np.float32)
        out["dense_holdout_" + m + "_all"] = np.asarray(res["holdout_" + m + "_all"], dtype=np.float32)
    return out


def holdout_export(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """What ``--dense-out`` gains: ``pred_holdout`` (F, J, 3) fp32 of an ``evaluate_holdout(keep=True)`` result, and what made it."""
    return {"pred_holdout": res["pred_holdout"], "holdout": np.array(str(res["holdout"]))}
