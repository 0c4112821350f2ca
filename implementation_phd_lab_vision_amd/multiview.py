"""Multi-view fusion: the cameras of one take brought into one frame of reference and fused into one pose per frame (INTEGRATION.md
section X, include/r50_multiview.h).

Human3.6M films every take with four synchronised cameras and the feature cache holds all four, but ``sequences.sequence_key`` keeps
them apart: ``results --dense`` ends in one pose per video frame of every camera on its own.  This module is the step after it:

* ``ViewTable.from_sequences`` relates the stitched sequences of one **take** ``(int(subject), str(action))`` with numpy (no GPU): the
  ordered **pairs** (source view -> target view) with their frame-matched rows, and per row its **peers**, the rows of the other views
  that show the same frame; ``DeviceViews`` checks the tables on the host and uploads them once;
* ``rigid_fit`` (``r50_op_view_rigid_fit``) is one least-squares rigid transform per pair over all matched rows.  The shards carry no
  extrinsics, but the ground-truth poses of two cameras are exact rigid images of each other: the fit of the ground truths IS the
  relative camera pose (the calibrated setting), its residual proves that the index matches frames across cameras, and the fit of the
  predictions is self-calibration;
* ``fuse_views`` (``r50_op_view_fuse``) maps every row's peers into its camera and fuses them -- ``mean``, per-coordinate ``median`` or
  ``others`` (the peers alone: what the other cameras say about this one) -- and reports how far the views lie apart (``disagreement``);
* ``evaluate_multiview`` runs the pass on the kept poses of ``sequences.evaluate_dense`` and scores the fused rows with the launches
  that scored the single views.

fp32 in and out, fp64 in between, the same bits on every run.  No CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_VIEWS = 8                 # the fuse kernel reads a row and at most 7 peers (include/r50_multiview.h)
MAX_JOINTS = 64
FIT_SLOTS = 16                # r50_op_view_rigid_fit: R (9), t (3), n, rms, scale, sqrt(sx / n)
FUSE_MODES = {"mean": 0, "median": 1, "others": 2}
FITS = ("gt", "pred")


def take_key(seq_key) -> Tuple[int, str]:
    return int(seq_key[0]), str(seq_key[1])


def _int32(a, what: str) -> np.ndarray:
    a = np.asarray(a, dtype=np.int64)
    if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) >= 2 ** 31):
        raise ValueError(f"{what} exceeds the int32 range")
    return np.ascontiguousarray(a, dtype=np.int32)


@dataclass
class ViewTable:
    """The views of every take over F rows of S sequences (all int32).  ``pair_start`` (P+1,), ``match`` (M, 2): pair p maps the source
    rows ``match[pair_start[p]:pair_start[p+1], 0]`` onto the target rows ``[..., 1]``, ascending ``frame_idx``; ``pair_src``,
    ``pair_dst`` (P,) = its sequences, ``pair_take`` (P,) = its take; pairs are ordered by (target sequence, source sequence).  The peers
    of row r: ``peer_row[peer_start[r]:peer_start[r+1]]`` in source-sequence order, ``peer_fit`` = the pair whose transform maps that
    peer into r's camera.  ``take_keys`` [n_takes] in order of first appearance, ``seq_take`` (S,) = a sequence's take, ``seq_view`` (S,)
    bool = whether the ``cams`` filter kept it, ``pair_origin`` (P,) = the pair's index in the table ``drop_takes`` was called on."""
    rows: int
    take_keys: List[Tuple[int, str]]
    seq_take: np.ndarray
    seq_view: np.ndarray
    pair_start: np.ndarray
    match: np.ndarray
    pair_src: np.ndarray
    pair_dst: np.ndarray
    pair_take: np.ndarray
    peer_start: np.ndarray
    peer_row: np.ndarray
    peer_fit: np.ndarray
    pair_origin: np.ndarray

    @property
    def pairs(self) -> int:
        return int(self.pair_src.shape[0])

    @property
    def takes(self) -> int:
        return len(self.take_keys)

    def views(self) -> np.ndarray:
        """(F,) int32: the views that show a row's frame, itself included."""
        return (1 + np.diff(self.peer_start)).astype(np.int32)

    @classmethod
    def from_sequences(cls, seq_keys: Sequence, seq_start, frame_idx, cams: Optional[Sequence] = None,
                       max_views: int = MAX_VIEWS) -> "ViewTable":
        seq_start, frame_idx = np.asarray(seq_start), np.asarray(frame_idx)
        n_seq, f = len(seq_keys), int(frame_idx.size)
        if seq_start.ndim != 1 or frame_idx.ndim != 1 or seq_start.size != n_seq + 1 or n_seq < 1 or \
                not np.issubdtype(seq_start.dtype, np.integer) or not np.issubdtype(frame_idx.dtype, np.integer):
            raise ValueError("seq_keys [S], seq_start (S+1,) and frame_idx (F,) must be 1-D integer tables of at least one sequence")
        ss = seq_start.astype(np.int64)
        if ss[0] != 0 or ss[-1] != f or np.any(np.diff(ss) < 1):
            raise ValueError(f"seq_start must rise strictly from 0 to len(frame_idx) = {f}")
        if f >= 2 ** 31:
            raise ValueError("too many rows for an int32 table")
        if not 2 <= int(max_views) <= MAX_VIEWS:
            raise ValueError(f"max_views must lie in [2, {MAX_VIEWS}], got {max_views}")
        idx = frame_idx.astype(np.int64)
        rising = np.ones(f, dtype=bool)
        rising[1:] = idx[1:] > idx[:-1]
        rising[ss[:-1]] = True
        if not rising.all():
            raise ValueError("frame_idx must rise strictly inside every sequence")
        keep = None if cams is None else {str(c) for c in cams}
        take_keys: List[Tuple[int, str]] = []
        pos: Dict[Tuple[int, str], int] = {}
        seq_take = np.empty(n_seq, dtype=np.int64)
        seq_view = np.zeros(n_seq, dtype=bool)
        members: List[List[int]] = []
        for s, key in enumerate(seq_keys):
            tk = take_key(key)
            if tk not in pos:
                pos[tk] = len(take_keys)
                take_keys.append(tk)
                members.append([])
            seq_take[s] = pos[tk]
            if keep is None or str(key[2]) in keep:
                seq_view[s] = True
                members[pos[tk]].append(s)
        for tk, mem in zip(take_keys, members):
            if len(mem) > max_views:
                raise ValueError(f"take {tk} has {len(mem)} views, more than {max_views}")
        found = []                                                               # (target, source, source rows, target rows)
        for mem in members:
            for v in mem:
                for u in mem:
                    if u == v:
                        continue
                    _, iu, iv = np.intersect1d(idx[ss[u]:ss[u + 1]], idx[ss[v]:ss[v + 1]], assume_unique=True, return_indices=True)
                    if iu.size:
                        found.append((v, u, ss[u] + iu, ss[v] + iv))
        found.sort(key=lambda e: (e[0], e[1]))
        n_pairs = len(found)
        counts = np.array([e[2].size for e in found], dtype=np.int64)
        pair_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        if n_pairs:
            match = np.stack([np.concatenate([e[2] for e in found]), np.concatenate([e[3] for e in found])], axis=1)
        else:
            match = np.zeros((0, 2), dtype=np.int64)
        pair_src = np.array([e[1] for e in found], dtype=np.int64)
        pair_dst = np.array([e[0] for e in found], dtype=np.int64)
        table = cls(rows=f, take_keys=take_keys, seq_take=_int32(seq_take, "seq_take"), seq_view=seq_view,
                    pair_start=_int32(pair_start, "pair_start"), match=_int32(match, "match").reshape(-1, 2),
                    pair_src=_int32(pair_src, "pair_src"), pair_dst=_int32(pair_dst, "pair_dst"),
                    pair_take=_int32(seq_take[pair_dst] if n_pairs else np.zeros(0), "pair_take"), peer_start=np.zeros(f + 1, dtype=np.int32),
                    peer_row=np.zeros(0, dtype=np.int32), peer_fit=np.zeros(0, dtype=np.int32), pair_origin=np.arange(n_pairs, dtype=np.int32))
        table._build_peers()
        return table

    def _build_peers(self) -> None:
        """The peers of every row from the pairs: pairs are ordered by (target, source), so a stable sort of the matches by target row
        leaves a row's peers in source-sequence order."""
        m = self.match.astype(np.int64)
        pair_of = np.repeat(np.arange(self.pairs, dtype=np.int64), np.diff(self.pair_start.astype(np.int64)))
        order = np.argsort(m[:, 1], kind="stable")
        self.peer_row = _int32(m[order, 0], "peer_row")
        self.peer_fit = _int32(pair_of[order], "peer_fit")
        self.peer_start = _int32(np.concatenate([[0], np.cumsum(np.bincount(m[:, 1], minlength=self.rows))]), "peer_start")

    def drop_takes(self, mask) -> "ViewTable":
        """The table without the pairs and peers of the takes flagged in ``mask`` (n_takes,) bool: their rows keep zero peers."""
        mask = np.asarray(mask, dtype=bool)
        if mask.shape != (self.takes,):
            raise ValueError(f"mask must be ({self.takes},) bool, got {mask.shape}")
        keep = ~mask[self.pair_take] if self.pairs else np.zeros(0, dtype=bool)
        counts = np.diff(self.pair_start.astype(np.int64))
        rows = np.repeat(keep, counts)
        out = ViewTable(rows=self.rows, take_keys=list(self.take_keys), seq_take=self.seq_take, seq_view=self.seq_view,
                        pair_start=_int32(np.concatenate([[0], np.cumsum(counts[keep])]), "pair_start"),
                        match=np.ascontiguousarray(self.match[rows]), pair_src=self.pair_src[keep], pair_dst=self.pair_dst[keep],
                        pair_take=self.pair_take[keep], peer_start=self.peer_start, peer_row=self.peer_row, peer_fit=self.peer_fit,
                        pair_origin=np.flatnonzero(keep).astype(np.int32))
        out._build_peers()
        return out


class DeviceViews:
    """A ``ViewTable`` checked on the host -- the kernels trust the tables -- and uploaded once.  Empty tables are padded to one element
    so that every pointer is valid."""

    def __init__(self, table: ViewTable, device):
        f, p = int(table.rows), table.pairs
        ps, mt = table.pair_start.astype(np.int64), table.match.astype(np.int64)
        pe, pr, pf = table.peer_start.astype(np.int64), table.peer_row.astype(np.int64), table.peer_fit.astype(np.int64)
        if ps.shape != (p + 1,) or ps[0] != 0 or ps[-1] != mt.shape[0] or np.any(np.diff(ps) < 0) or mt.ndim != 2 or mt.shape[1] != 2:
            raise ValueError(f"pair_start must be non-decreasing from 0 to len(match) = {mt.shape[0]} over {p} pairs")
        if mt.size and (int(mt.min()) < 0 or int(mt.max()) >= f):
            raise ValueError(f"every matched row must lie in [0, {f})")
        if pe.shape != (f + 1,) or pe[0] != 0 or pe[-1] != pr.size or pr.size != pf.size or np.any(np.diff(pe) < 0):
            raise ValueError(f"peer_start must be non-decreasing from 0 to len(peer_row) = len(peer_fit) = {pr.size} over {f} rows")
        if pr.size and (int(pr.min()) < 0 or int(pr.max()) >= f or int(pf.min()) < 0 or int(pf.max()) >= p):
            raise ValueError(f"every peer row must lie in [0, {f}) and every peer fit in [0, {p})")
        if f and int(np.diff(pe).max()) > MAX_VIEWS - 1:
            raise ValueError(f"a row has {int(np.diff(pe).max())} peers, more than {MAX_VIEWS - 1}")
        self.table, self.rows, self.pairs = table, f, p
        self.device = torch.device(device)

        def up(a):
            a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
            return torch.from_numpy(a if a.size else np.zeros(1, dtype=np.int32)).to(self.device)
        self.pair_start, self.match, self.peer_start, self.peer_row, self.peer_fit = up(table.pair_start), up(table.match), \
            up(table.peer_start), up(table.peer_row), up(table.peer_fit)

    @classmethod
    def of(cls, views, device) -> "DeviceViews":
        if isinstance(views, cls):
            if views.device != torch.device(device):
                raise ValueError(f"the tables were uploaded to {views.device}, the poses are on {device}")
            return views
        return cls(views, device)


def _check_poses(x: torch.Tensor, views: DeviceViews, what: str) -> Tuple[int, int]:
    if x.dim() != 3 or x.shape[2] != 3 or x.dtype != torch.float32:
        raise ValueError(f"{what}: poses (F, J, 3) fp32 expected, got {tuple(x.shape)} {x.dtype}")
    f, j, _ = x.shape
    if f != views.rows or not 1 <= j <= MAX_JOINTS:
        raise ValueError(f"{what}: the tables hold {views.rows} rows, the poses {f}; need 1 <= J <= {MAX_JOINTS} (got {j})")
    if x.device.type != "cuda" or x.device != views.device:
        raise ValueError(f"{what}: poses and tables must be on one GPU: there is no CPU fallback")
    if not x.is_contiguous():
        raise ValueError(f"{what}: poses must be contiguous")
    return f, j


def _stream(x: torch.Tensor) -> int:
    return torch.cuda.current_stream(x.device).cuda_stream


def rigid_fit(y: torch.Tensor, x: torch.Tensor, views) -> torch.Tensor:
    """One ``r50_op_view_rigid_fit`` launch: per pair of ``views`` the rigid transform that maps the matched rows of y (the source view)
    onto those of x (the target view); y and x (F, J, 3) fp32 over the same rows, possibly one tensor.  Returns ``fit (P, 16)`` fp64 on
    the device: R row-major, t, n, rms, the least-squares scale (never applied) and sqrt(sx / n).  No launch where there is no pair."""
    views = DeviceViews.of(views, y.device)
    f, j = _check_poses(y, views, "rigid_fit")
    if _check_poses(x, views, "rigid_fit") != (f, j):
        raise ValueError(f"rigid_fit: y and x differ in shape: {tuple(y.shape)}, {tuple(x.shape)}")
    fit = torch.empty((views.pairs, FIT_SLOTS), dtype=torch.float64, device=y.device)
    if views.pairs == 0:
        return fit
    rc = _lib.load_library().r50_op_view_rigid_fit(y.data_ptr(), x.data_ptr(), f, f, j, views.pair_start.data_ptr(), views.match.data_ptr(),
                                                   views.pairs, fit.data_ptr(), _stream(y))
    _lib.check(rc, None, "r50_op_view_rigid_fit")
    return fit


def fuse_views(pose: torch.Tensor, views, fit: torch.Tensor, mode="mean") -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``r50_op_view_fuse`` launch: every row of pose (F, J, 3) fp32 fused with its peers under ``fit (P, 16)`` fp64 (``rigid_fit``'s
    layout); ``mode`` 0 / 1 / 2 or ``mean`` / ``median`` / ``others``.  Returns ``(fused (F, J, 3), disagreement (F,))`` fp32."""
    mode = FUSE_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if mode not in (0, 1, 2):
        raise ValueError(f"mode must be 0, 1, 2 or one of {sorted(FUSE_MODES)}, got {mode!r}")
    views = DeviceViews.of(views, pose.device)
    f, j = _check_poses(pose, views, "fuse_views")
    if fit.dtype != torch.float64 or tuple(fit.shape) != (views.pairs, FIT_SLOTS) or fit.device != pose.device or not fit.is_contiguous():
        raise ValueError(f"fit must be a contiguous ({views.pairs}, {FIT_SLOTS}) fp64 tensor on {pose.device}")
    if views.pairs == 0:
        fit = torch.zeros((1, FIT_SLOTS), dtype=torch.float64, device=pose.device)          # never read: no row has a peer
    fused = torch.empty_like(pose)
    dis = torch.empty(f, dtype=torch.float32, device=pose.device)
    rc = _lib.load_library().r50_op_view_fuse(pose.data_ptr(), f, j, views.peer_start.data_ptr(), views.peer_row.data_ptr(),
                                              views.peer_fit.data_ptr(), fit.data_ptr(), views.pairs, int(mode), fused.data_ptr(),
                                              dis.data_ptr(), _stream(pose))
    _lib.check(rc, None, "r50_op_view_fuse")
    return fused, dis


def extrinsics_error(fit_a: np.ndarray, fit_b: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Per pair, how far two fit tables (P, 16) lie apart: the angle in degrees of ``R_a R_b^T`` -- ``atan2(|axis|, (trace - 1) / 2)``,
    which keeps its digits near 0 and near 180 degrees -- and ``|t_a - t_b|`` in millimetres (the tables are in metres)."""
    a, b = np.asarray(fit_a, dtype=np.float64).reshape(-1, FIT_SLOTS), np.asarray(fit_b, dtype=np.float64).reshape(-1, FIT_SLOTS)
    if a.shape != b.shape:
        raise ValueError(f"the fit tables differ in shape: {a.shape}, {b.shape}")
    d = np.einsum("pij,pkj->pik", a[:, :9].reshape(-1, 3, 3), b[:, :9].reshape(-1, 3, 3))
    axis = 0.5 * np.stack([d[:, 2, 1] - d[:, 1, 2], d[:, 0, 2] - d[:, 2, 0], d[:, 1, 0] - d[:, 0, 1]], axis=1)
    angle = np.degrees(np.arctan2(np.linalg.norm(axis, axis=1), 0.5 * (np.trace(d, axis1=1, axis2=2) - 1.0)))
    return angle, np.linalg.norm(a[:, 9:12] - b[:, 9:12], axis=1) * 1000.0


def frame_p1(pred: np.ndarray, gt: np.ndarray, root: int = 0) -> np.ndarray:
    """(F,) fp64: the root-relative MPJPE of every row, numpy."""
    y, x = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    return np.linalg.norm((y - y[:, root:root + 1]) - (x - x[:, root:root + 1]), axis=-1).mean(axis=-1)


def pearson_r(a: np.ndarray, b: np.ndarray) -> float:
    """Pearson's r in fp64; NaN with fewer than two values or where one side does not vary."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size < 2:
        return float("nan")
    a0, b0 = a - a.mean(), b - b.mean()
    den = np.sqrt((a0 * a0).sum() * (b0 * b0).sum())
    return float((a0 * b0).sum() / den) if den > 0 else float("nan")


@torch.no_grad()
def evaluate_multiview(dense: Dict[str, object], device, fit: str = "gt", fuse: str = "mean", cams: Optional[Sequence] = None,
                       gt_tol_mm: float = 1.0) -> Dict[str, object]:
    """The views of every take fused and scored.  ``dense`` is the result of ``sequences.evaluate_dense(keep_poses=True, post=...)``; the
    single-view poses are its ``pred_post`` where a post-process ran, else ``pred``.

    1. ``ViewTable.from_sequences`` relates the sequences (``cams`` keeps only the named cameras).
    2. ``rigid_fit(gt, gt)``: a take with a pair whose residual is not <= ``gt_tol_mm`` is **misaligned** -- its cameras do not show the
       same frames at the matched rows -- and is left out of the fusion.  Exact rigid images stored as fp32 below 8 m leave at most
       2 sqrt(3) 2^-22 m = 8.3e-4 mm; a mismatch of one frame leaves centimetres.  The default of 1 mm is a condition, not a measurement.
    3. The transforms are that fit (``fit="gt"``, calibrated) or ``rigid_fit(pred, pred)`` (``fit="pred"``, self-calibration).
    4. ``fuse_views`` (``fuse``: ``mean``, ``median``, ``others``).
    5. The fused rows are scored by the metrics and protocols launches of ``evaluate_dense``, with the disagreement in the spread slot
       and offsets built from the views; the sums are read once.

    Returns (metres; fp64), for M in ``p1``, ``p2``, ``mpjve``, ``accel``::

        mv_M (G,), mv_M_all, mv_M_mean             beside M, M_all, M_mean of ``dense`` (the groups are ``dense["group_names"]``)
        mv_disagreement (G,), mv_disagreement_all   the mean disagreement
        mv_views_hist (9,) int64                    frames by number of views
        mv_takes, mv_pairs, excluded_takes          fused takes (two views or more), their pairs, misaligned takes
        excluded                                    [(subject, action, worst ground-truth rms in mm)]
        mv_pair_rms_gt, mv_pair_rms_pred, mv_pair_scale (P,)   per fused pair: the residuals of the two fits and the predictions' scale
        mv_pair_angle_deg, mv_pair_shift_mm (P,)    with fit="pred": the extrinsics error of self-calibration (``extrinsics_error``)
        mv_confidence_r                             Pearson's r of disagreement and single-view P1 over the frames with >= 2 views
        pred_mv (F, J, 3) fp32, frame_disagreement (F,) fp32, views (F,) int32
        mv_fit, mv_fuse                             what was applied
    """
    from . import protocols, sequences
    if fit not in FITS:
        raise ValueError(f"fit must be one of {FITS}, got {fit!r}")
    if fuse not in FUSE_MODES:
        raise ValueError(f"fuse must be one of {sorted(FUSE_MODES)}, got {fuse!r}")
    tol = float(gt_tol_mm)
    if not tol > 0.0:
        raise ValueError(f"gt_tol_mm must be > 0, got {gt_tol_mm}")
    missing = [k for k in ("seq_keys", "seq_start", "frame_idx", "pred", "gt", "group_names") if k not in dense]
    if missing:
        raise ValueError(f"the dense result lacks {missing}: run evaluate_dense with keep_poses=True")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("evaluate_multiview runs on a GPU: there is no CPU fallback")
    seq_keys, seq_start, frame_idx = dense["seq_keys"], np.asarray(dense["seq_start"]), np.asarray(dense["frame_idx"])
    single = np.asarray(dense["pred_post"] if "pred_post" in dense else dense["pred"])
    gt_host = np.asarray(dense["gt"])
    table = ViewTable.from_sequences(seq_keys, seq_start, frame_idx, cams)
    group_names = list(dense["group_names"])
    gpos = {a: g for g, a in enumerate(group_names)}
    seq_rows = np.diff(seq_start.astype(np.int64))
    seq_group = np.array([gpos[protocols.action_name(k[1])] for k in seq_keys], dtype=np.int32)
    n_groups, f, joints = len(group_names), int(single.shape[0]), int(single.shape[1])
    with torch.cuda.device(device):
        pred = torch.from_numpy(np.ascontiguousarray(single, dtype=np.float32)).to(device)
        gt = torch.from_numpy(np.ascontiguousarray(gt_host, dtype=np.float32)).to(device)
        fit_gt_all = rigid_fit(gt, gt, DeviceViews(table, device)).cpu().numpy()      # the one decision that needs the host
        bad_pair = ~(fit_gt_all[:, 13] * 1000.0 <= tol)                               # a NaN residual is misaligned too
        bad_take = np.zeros(table.takes, dtype=bool)
        bad_take[table.pair_take[bad_pair]] = True
        excluded = [(tk[0], tk[1], float(np.max(np.nan_to_num(fit_gt_all[table.pair_take == i, 13], nan=np.inf)) * 1000.0))
                    for i, tk in enumerate(table.take_keys) if bad_take[i]]
        kept = table.drop_takes(bad_take)
        views = DeviceViews(kept, device)
        fit_gt = torch.from_numpy(np.ascontiguousarray(fit_gt_all[kept.pair_origin])).to(device)
        fit_pred = rigid_fit(pred, pred, views)
        fused, dis = fuse_views(pred, views, fit_gt if fit == "gt" else fit_pred, fuse)
        n_views = kept.views()
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(n_views, dtype=np.int64)]).astype(np.int32)).to(device)
        seq = np.repeat(np.arange(len(seq_keys), dtype=np.int32), seq_rows)
        group = torch.from_numpy(seq_group[seq]).to(device)
        part = sequences.sequence_metrics(fused, gt, dis, offsets, torch.from_numpy(seq).to(device),
                                          torch.from_numpy(np.ascontiguousarray(frame_idx, dtype=np.int32)).to(device), group, n_groups)
        acc_p2 = torch.zeros(3 * n_groups, dtype=torch.float64, device=device)
        protocols._launch(fused.view(f, 1, joints, 3), gt.view(f, 1, joints, 3), 0, group, n_groups, acc_p2, protocols.ROOT_JOINT)
        host = torch.cat([acc_p2, part.reshape(-1), fit_pred.reshape(-1)]).cpu().numpy()
        pred_mv, frame_dis = fused.cpu().numpy(), dis.cpu().numpy()
    p2, part, fit_pred_host = np.split(host, [3 * n_groups, host.size - kept.pairs * FIT_SLOTS])
    fit_pred_host = fit_pred_host.reshape(-1, FIT_SLOTS)
    vals = sequences.metric_values(sequences.sum_blocks(part.reshape(-1, n_groups, sequences.METRIC_SLOTS)),
                                   p2[:2 * n_groups].reshape(n_groups, 2)[:, 1])
    out: Dict[str, object] = {"mv_fit": fit, "mv_fuse": fuse}
    for m in ("p1", "p2", "mpjve", "accel"):
        for suffix in ("", "_all", "_mean"):
            out["mv_" + m + suffix] = vals[m + suffix]
    out["mv_disagreement"], out["mv_disagreement_all"] = vals["spread"], vals["spread_all"]
    out["mv_views_hist"] = np.bincount(n_views, minlength=MAX_VIEWS + 1).astype(np.int64)
    out["mv_takes"] = int(np.unique(kept.pair_take).size)
    out["mv_pairs"], out["excluded_takes"], out["excluded"] = kept.pairs, len(excluded), excluded
    fit_gt_host = fit_gt_all[kept.pair_origin]
    out["mv_pair_rms_gt"], out["mv_pair_rms_pred"], out["mv_pair_scale"] = fit_gt_host[:, 13].copy(), fit_pred_host[:, 13].copy(), \
        fit_pred_host[:, 14].copy()
    if fit == "pred":
        out["mv_pair_angle_deg"], out["mv_pair_shift_mm"] = extrinsics_error(fit_pred_host, fit_gt_host)
    multi = n_views >= 2
    out["mv_confidence_r"] = pearson_r(frame_dis[multi].astype(np.float64), frame_p1(single[multi], gt_host[multi], protocols.ROOT_JOINT))
    out["pred_mv"], out["frame_disagreement"], out["views"] = pred_mv, frame_dis, n_views
    return out


def add_flags(parser) -> None:
    """The ``--multiview`` flags of ``results``; absent from the namespace unless given."""
    import argparse
    s = argparse.SUPPRESS
    parser.add_argument("--multiview", action="store_true", default=s,
                        help="also bring the cameras of every take into one frame of reference, fuse them into one pose per frame and "
                             "score the result beside the single views (--dense; INTEGRATION.md section X)")
    parser.add_argument("--multiview-fit", choices=FITS, default=s,
                        help="where the relative camera poses come from (--multiview): a rigid fit of the ground truths (gt, default: "
                             "calibrated) or of the predictions themselves (pred: self-calibration)")
    parser.add_argument("--multiview-fuse", choices=tuple(FUSE_MODES), default=s,
                        help="how the views of a frame are fused (--multiview): mean (default), per-coordinate median, or the other "
                             "cameras alone (others)")
    parser.add_argument("--multiview-cams", nargs="+", default=s, metavar="CAM", help="only fuse these cameras (--multiview; default: all)")
    parser.add_argument("--multiview-gt-tol-mm", type=float, default=s, metavar="MM",
                        help="a take whose ground truths are not rigid images of each other within this residual is left out "
                             "(--multiview; default 1.0)")


OPTION_FLAGS = ("multiview_fit", "multiview_fuse", "multiview_cams", "multiview_gt_tol_mm")


def options_from_args(args) -> Optional[Dict[str, object]]:
    """The keyword arguments of ``evaluate_multiview`` from parsed arguments, or None without ``--multiview``."""
    if not hasattr(args, "multiview"):
        return None
    return {"fit": getattr(args, "multiview_fit", "gt"), "fuse": getattr(args, "multiview_fuse", "mean"),
            "cams": getattr(args, "multiview_cams", None), "gt_tol_mm": getattr(args, "multiview_gt_tol_mm", 1.0)}


def multiview_lines(dense: Dict[str, object], res: Dict[str, object]) -> List[str]:
    """The ``Dense | multiview`` lines: what was applied and the counts, single view -> fused over all frames and per action (mm), and
    with ``fit="pred"`` the extrinsics error of self-calibration."""
    single = "post_" if "pred_post" in dense else ""

    def pair(m: str, key: str, i=None) -> str:
        a, b = dense[single + m + key], res["mv_" + m + key]
        a, b = (a, b) if i is None else (a[i], b[i])
        return f"{a * 1000.0:.2f} -> {b * 1000.0:.2f}"

    def row(key: str, i=None) -> str:
        d = res["mv_disagreement" + key]
        d = d if i is None else d[i]
        return (f"p1 (mm) {pair('p1', key, i)} | p2 (mm) {pair('p2', key, i)} | vel (mm/frame) {pair('mpjve', key, i)} | accel (mm/frame^2) "
                f"{pair('accel', key, i)} | disagreement (mm) {d * 1000.0:.2f}")

    hist = res["mv_views_hist"]
    lines = [f"Dense | multiview fit {res['mv_fit']} fuse {res['mv_fuse']} | takes {res['mv_takes']} | pairs {res['mv_pairs']} | frames by "
             "views " + " ".join(f"{k}:{int(n)}" for k, n in enumerate(hist) if n) + f" | excluded takes {res['excluded_takes']}"
             f" | confidence r {res['mv_confidence_r']:.3f} | single view -> fused, all: {row('_all')}"]
    for i, name in enumerate(dense["group_names"]):
        lines.append(f"Dense | multiview   {name} | {row('', i)}")
    for subject, action, rms in res["excluded"]:
        lines.append(f"Dense | multiview   excluded S{subject} {action}: the ground truths of its cameras are not rigid images of each "
                     f"other (rms {rms:.3f} mm)")
    if "mv_pair_angle_deg" in res and res["mv_pairs"]:
        ang, shift = res["mv_pair_angle_deg"], res["mv_pair_shift_mm"]
        lines.append(f"Dense | multiview   self-calibration against the ground-truth extrinsics | angle (deg) mean {ang.mean():.3f} max "
                     f"{ang.max():.3f} | shift (mm) mean {shift.mean():.2f} max {shift.max():.2f}")
    return lines


PAIR_KEYS = ("mv_pair_rms_gt", "mv_pair_rms_pred", "mv_pair_scale", "mv_pair_angle_deg", "mv_pair_shift_mm")


def multiview_npz(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``dense_mv_*`` keys of the result ``.npz``: ``dense_mv_M`` (G,) and ``dense_mv_M_all`` () fp32 for M in p1, p2, mpjve, accel,
    disagreement; ``dense_mv_views_hist`` (9,), ``dense_mv_counts`` int64 [takes, pairs, excluded takes], ``dense_mv_excluded`` str,
    ``dense_mv_applied`` str [fit, fuse], ``dense_mv_confidence_r`` and the per-pair arrays ``dense_mv_pair_*`` fp64."""
    out = {"dense_mv_applied": np.array([str(res["mv_fit"]), str(res["mv_fuse"])], dtype=str),
           "dense_mv_counts": np.array([res["mv_takes"], res["mv_pairs"], res["excluded_takes"]], dtype=np.int64),
           "dense_mv_views_hist": np.asarray(res["mv_views_hist"], dtype=np.int64),
           "dense_mv_excluded": np.array([f"S{s} {a}" for s, a, _ in res["excluded"]], dtype=str),
           "dense_mv_confidence_r": np.asarray(res["mv_confidence_r"], dtype=np.float64)}
    for m in ("p1", "p2", "mpjve", "accel", "disagreement"):
        out["dense_mv_" + m] = np.asarray(res["mv_" + m], dtype=np.float32)
        out["dense_mv_" + m + "_all"] = np.asarray(res["mv_" + m + "_all"], dtype=np.float32)
    for k in PAIR_KEYS:
        if k in res:
            out["dense_" + k] = np.asarray(res[k], dtype=np.float64)
    return out


def multiview_export(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """What ``--dense-out`` gains: ``pred_mv`` (F, J, 3) fp32, ``frame_disagreement`` (F,) fp32, ``views`` (F,) int32, ``mv_pair_*``."""
    out = {"pred_mv": res["pred_mv"], "frame_disagreement": res["frame_disagreement"], "views": res["views"]}
    out.update({k: np.asarray(res[k], dtype=np.float64) for k in PAIR_KEYS if k in res})
    return out
