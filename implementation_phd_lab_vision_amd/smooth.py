"""Temporal smoothing and constant bone lengths for stitched per-frame pose sequences (include/r50_smooth.h).

``results --dense`` and ``predict`` end in one 3D pose per video frame; this module is the step between the stitch and the metrics (or
the files): a filter along time inside every **segment** (a maximal run of rows of one sequence whose ``idx`` are consecutive integers)
and a rigid-skeleton step per **sequence**, both on the device where the stitched poses already sit.

* ``segment_table`` builds the ragged tables with numpy; ``DeviceTables`` checks them on the host and uploads them once;
* ``gauss_table`` / ``savgol_table`` build the position-dependent FIR table ``coef (W, W)`` in fp64; ``fir_sequences`` applies any such
  table (``r50_op_fir_sequences``);
* ``one_euro_sequences`` is the causal One-Euro filter (``r50_op_one_euro_sequences``);
* ``bone_stats`` / ``fix_bone_lengths`` give every bone of a sequence its mean length (``r50_op_bone_stats``, ``r50_op_bone_rebuild``);
* ``PostProcess`` bundles the choice and ``apply`` runs it without a host round trip.

fp32 in and out, fp64 in between, one rounding at the store, the same bits on every run.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .train import H36M_EDGES

MAX_W = 63                  # the op's limits (include/r50_smooth.h)
MAX_JOINTS = 64
KINDS = (None, "gauss", "savgol", "one_euro")
STAT_SLOTS = 2              # r50_op_bone_stats: (mean, sum of squared deviations) per (sequence, edge)


def segment_table(seq_start, idx) -> Tuple[np.ndarray, np.ndarray]:
    """``(seg_start (G+1,) int32, row_seg (F,) int32)`` of the rows ``idx (F,)`` of the sequences ``seq_start (S+1,)``: a segment ends
    where the sequence ends or where ``idx`` does not go on with the next integer."""
    seq_start, idx = np.asarray(seq_start), np.asarray(idx)
    if seq_start.ndim != 1 or idx.ndim != 1 or seq_start.size < 2 or not np.issubdtype(seq_start.dtype, np.integer) or \
            not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("seq_start (S+1,) and idx (F,) must be 1-D integer arrays with at least one sequence")
    ss = seq_start.astype(np.int64)
    f = int(idx.size)
    if ss[0] != 0 or ss[-1] != f or np.any(np.diff(ss) < 1):
        raise ValueError(f"seq_start must rise strictly from 0 to len(idx) = {f} (every sequence has at least one row)")
    if f >= 2 ** 31:
        raise ValueError("too many rows for an int32 table")
    new = np.zeros(f, dtype=bool)
    new[ss[:-1]] = True
    ix = idx.astype(np.int64)
    new[1:] |= ix[1:] != ix[:-1] + 1
    first = np.flatnonzero(new)
    return np.append(first, f).astype(np.int32), (np.cumsum(new) - 1).astype(np.int32)


def gauss_table(sigma: float = 1.5) -> np.ndarray:
    """``coef (W, W)`` fp64, ``W = 2 ceil(3 sigma) + 1``: row e is ``exp(-(k - e)^2 / (2 sigma^2))`` for ``|k - e| <= R``, zero
    elsewhere, normalised to sum 1 (row R is the centred kernel, the others the kernel cut at the segment's edge and renormalised)."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma must be positive and finite, got {sigma}")
    r = int(math.ceil(3.0 * sigma))
    w = 2 * r + 1
    if w > MAX_W:
        raise ValueError(f"sigma = {sigma} needs a window of {w} rows, more than {MAX_W}")
    k = np.arange(w, dtype=np.float64)
    d = k[None, :] - k[:, None]
    coef = np.where(np.abs(d) <= r, np.exp(-(d * d) / (2.0 * sigma * sigma)), 0.0)
    return coef / coef.sum(axis=1, keepdims=True)


def savgol_table(window: int = 9, degree: int = 2) -> np.ndarray:
    """``coef (W, W)`` fp64: row e holds the weights that evaluate, at window position e, the least-squares polynomial of ``degree``
    over the W window positions -- ``A pinv(A)`` of the Vandermonde matrix A, computed as ``Q Q^T`` from A's QR factors on positions
    scaled to [-1, 1].  Row R is the centred Savitzky-Golay filter, the others its "interp" edge treatment."""
    w, p = int(window), int(degree)
    if w != window or p != degree or w < 1 or w > MAX_W or w % 2 == 0:
        raise ValueError(f"window must be an odd integer in [1, {MAX_W}], got {window!r}")
    if p < 0 or p >= w:
        raise ValueError(f"degree must satisfy 0 <= degree < window = {w}, got {degree!r}")
    r = (w - 1) // 2
    t = (np.arange(w, dtype=np.float64) - r) / max(r, 1)
    q, _ = np.linalg.qr(np.vander(t, p + 1, increasing=True))
    return q @ q.T


def check_coef(coef) -> np.ndarray:
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 2 or coef.shape[0] != coef.shape[1] or coef.shape[0] % 2 == 0 or not 1 <= coef.shape[0] <= MAX_W:
        raise ValueError(f"coef must be (W, W) with W odd in [1, {MAX_W}], got {coef.shape}")
    if not np.isfinite(coef).all():
        raise ValueError("coef must be finite")
    return coef


def check_edges(edges, joints: int) -> np.ndarray:
    """The edge list as a (E, 2) int32 array, refused unless ``1 <= E <= J - 1``, every index is in ``[0, J)``, a joint is a child at
    most once, and every edge comes after the one that places its parent."""
    e = np.asarray(edges)
    if e.ndim != 2 or e.shape[1] != 2 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"edges must be (E, 2) integers (parent, child), got {e.shape} {e.dtype}")
    n = int(e.shape[0])
    if not 1 <= n <= joints - 1:
        raise ValueError(f"need 1 <= E <= J - 1 = {joints - 1} edges, got {n}")
    if int(e.min()) < 0 or int(e.max()) >= joints:
        raise ValueError(f"every edge index must lie in [0, {joints})")
    children = set(int(c) for c in e[:, 1])
    placed = set()
    for pa, ch in e.tolist():
        if pa == ch:
            raise ValueError(f"edge ({pa}, {ch}) needs two different joints")
        if ch in placed:
            raise ValueError(f"joint {ch} is the child of more than one edge")
        if pa in children and pa not in placed:
            raise ValueError(f"edge ({pa}, {ch}) comes before the edge that places its parent")
        placed.add(ch)
    return np.ascontiguousarray(e, dtype=np.int32)


class DeviceTables:
    """The ragged tables of one stitched buffer, checked on the host -- the kernels trust them -- and uploaded once: ``seq_start``
    (S+1,), ``row_seq`` (F,), ``seg_start`` (G+1,), ``row_seg`` (F,), all int32."""

    def __init__(self, seq_start, idx, device):
        self.seg_start_host, self.row_seg_host = segment_table(seq_start, idx)
        self.seq_start_host = np.ascontiguousarray(seq_start, dtype=np.int32)
        self.rows = int(np.asarray(idx).size)
        self.sequences = int(self.seq_start_host.size - 1)
        self.segments = int(self.seg_start_host.size - 1)
        row_seq = np.repeat(np.arange(self.sequences, dtype=np.int32), np.diff(self.seq_start_host))
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)          # noqa: E731
        self.seq_start, self.row_seq, self.seg_start, self.row_seg = up(self.seq_start_host), up(row_seq), up(self.seg_start_host), \
            up(self.row_seg_host)

    @classmethod
    def of(cls, table, device) -> "DeviceTables":
        """From a ``DeviceTables`` (returned as it is), a ``SequenceTable`` or a pair ``(seq_start, idx)``."""
        if isinstance(table, cls):
            if table.device != torch.device(device):
                raise ValueError(f"the tables were uploaded to {table.device}, the poses are on {device}")
            return table
        if hasattr(table, "seq_start") and hasattr(table, "idx"):
            return cls(table.seq_start, table.idx, device)
        return cls(table[0], table[1], device)


def _check_poses(x: torch.Tensor, tables: DeviceTables, what: str) -> Tuple[int, int]:
    if x.dim() != 3 or x.shape[2] != 3 or x.dtype != torch.float32:
        raise ValueError(f"{what}: poses (F, J, 3) fp32 expected, got {tuple(x.shape)} {x.dtype}")
    f, j, _ = x.shape
    if f != tables.rows or not 1 <= j <= MAX_JOINTS:
        raise ValueError(f"{what}: the tables hold {tables.rows} rows, the poses {f}; need 1 <= J <= {MAX_JOINTS} (got {j})")
    if x.device.type != "cuda" or x.device != tables.device:
        raise ValueError(f"{what}: poses and tables must be on one GPU: there is no CPU fallback")
    if not x.is_contiguous():
        raise ValueError(f"{what}: poses must be contiguous")
    return f, j


def _stream(x: torch.Tensor) -> int:
    return torch.cuda.current_stream(x.device).cuda_stream


def fir_sequences(x: torch.Tensor, tables: DeviceTables, coef: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """One ``r50_op_fir_sequences`` launch: x (F, J, 3) fp32, ``coef`` (W, W) fp64 on the same GPU (``upload_coef``).  Returns ``(out,
    short_rows)``: the filtered poses, and on the device the int32 pair [rows of segments shorter than W (copied), such segments]."""
    f, j = _check_poses(x, tables, "fir_sequences")
    if coef.dtype != torch.float64 or coef.dim() != 2 or coef.shape[0] != coef.shape[1] or coef.device != x.device or not coef.is_contiguous():
        raise ValueError(f"coef must be a contiguous (W, W) fp64 tensor on {x.device}, got {tuple(coef.shape)} {coef.dtype} on {coef.device}")
    w = int(coef.shape[0])
    if w % 2 == 0 or not 1 <= w <= MAX_W:
        raise ValueError(f"W must be odd and in [1, {MAX_W}], got {w}")
    out = torch.empty_like(x)
    short = torch.empty(2, dtype=torch.int32, device=x.device)
    rc = _lib.load_library().r50_op_fir_sequences(x.data_ptr(), tables.seg_start.data_ptr(), tables.row_seg.data_ptr(), f, tables.segments, j,
                                                  coef.data_ptr(), w, out.data_ptr(), short.data_ptr(), _stream(x))
    _lib.check(rc, None, "r50_op_fir_sequences")
    return out, short


def upload_coef(coef, device) -> torch.Tensor:
    return torch.from_numpy(check_coef(coef)).to(device)


def one_euro_sequences(x: torch.Tensor, tables: DeviceTables, rate: float = 25.0, min_cutoff: float = 1.0, beta: float = 0.0,
                       d_cutoff: float = 1.0) -> torch.Tensor:
    """One ``r50_op_one_euro_sequences`` launch: the causal One-Euro filter per coordinate, restarted at every segment's first row."""
    f, j = _check_poses(x, tables, "one_euro_sequences")
    rate, min_cutoff, beta, d_cutoff = float(rate), float(min_cutoff), float(beta), float(d_cutoff)
    if not (all(math.isfinite(v) for v in (rate, min_cutoff, beta, d_cutoff)) and rate > 0 and min_cutoff > 0 and d_cutoff > 0 and beta >= 0):
        raise ValueError(f"need finite rate, min_cutoff, d_cutoff > 0 and beta >= 0, got {rate}, {min_cutoff}, {d_cutoff}, {beta}")
    out = torch.empty_like(x)
    rc = _lib.load_library().r50_op_one_euro_sequences(x.data_ptr(), tables.seg_start.data_ptr(), f, tables.segments, j, rate, min_cutoff,
                                                       beta, d_cutoff, out.data_ptr(), _stream(x))
    _lib.check(rc, None, "r50_op_one_euro_sequences")
    return out


def _edge_array(edges: np.ndarray):
    flat = edges.reshape(-1)
    return (ctypes.c_int * flat.size)(*flat.tolist())


def bone_stats(x: torch.Tensor, tables: DeviceTables, edges=H36M_EDGES) -> torch.Tensor:
    """One ``r50_op_bone_stats`` launch: ``stats (S, E, 2)`` fp64 on the device, per (sequence, edge) the mean bone length over the
    sequence's rows and the sum of squared deviations from it."""
    f, j = _check_poses(x, tables, "bone_stats")
    e = check_edges(edges, j)
    stats = torch.empty((tables.sequences, e.shape[0], STAT_SLOTS), dtype=torch.float64, device=x.device)
    rc = _lib.load_library().r50_op_bone_stats(x.data_ptr(), tables.seq_start.data_ptr(), f, tables.sequences, j, _edge_array(e), e.shape[0],
                                               stats.data_ptr(), _stream(x))
    _lib.check(rc, None, "r50_op_bone_stats")
    return stats


def fix_bone_lengths(x: torch.Tensor, tables: DeviceTables, edges=H36M_EDGES,
                     stats: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Every frame rebuilt from its root down ``edges`` with each bone at its sequence's mean length (``stats``, by default those of x:
    ``r50_op_bone_stats`` then ``r50_op_bone_rebuild``).  Returns ``(out, stats)``."""
    f, j = _check_poses(x, tables, "fix_bone_lengths")
    e = check_edges(edges, j)
    if stats is None:
        stats = bone_stats(x, tables, e)
    if (stats.dtype != torch.float64 or tuple(stats.shape) != (tables.sequences, e.shape[0], STAT_SLOTS) or stats.device != x.device
            or not stats.is_contiguous()):
        raise ValueError(f"stats must be a contiguous ({tables.sequences}, {e.shape[0]}, 2) fp64 tensor on {x.device}")
    out = torch.empty_like(x)
    rc = _lib.load_library().r50_op_bone_rebuild(x.data_ptr(), tables.row_seq.data_ptr(), f, tables.sequences, j, _edge_array(e), e.shape[0],
                                                 stats.data_ptr(), out.data_ptr(), _stream(x))
    _lib.check(rc, None, "r50_op_bone_rebuild")
    return out, stats


def bone_std_mm(stats: np.ndarray, seq_rows: np.ndarray, seq_group: np.ndarray, n_groups: int) -> Tuple[np.ndarray, float]:
    """The bone-length standard deviation over time in millimetres from ``stats (S, E, 2)`` (metres): per group the root of the pooled
    squared deviations of its sequences' bones from their own sequence means, ``sqrt(sum ssd / (E sum rows))``; and over all sequences.
    NaN for a group without rows."""
    stats = np.asarray(stats, dtype=np.float64)
    ssd = stats[:, :, 1].sum(axis=1)
    terms = np.asarray(seq_rows, dtype=np.float64) * stats.shape[1]
    num = np.bincount(seq_group, weights=ssd, minlength=n_groups)
    den = np.bincount(seq_group, weights=terms, minlength=n_groups)
    per = np.where(den > 0, np.sqrt(num / np.where(den > 0, den, 1.0)), np.nan) * 1000.0
    return per, float(np.sqrt(ssd.sum() / terms.sum()) * 1000.0)


@dataclass
class PostProcess:
    """What happens to stitched poses between the stitch and the metrics: a filter ``kind`` (None, ``gauss`` with ``sigma``, ``savgol``
    with ``window`` and ``degree``, ``one_euro`` with ``rate``, ``min_cutoff``, ``beta``, ``d_cutoff``), then, with ``fix_bones``, the
    constant bone lengths over ``edges``.  The parameters are checked when the object is made."""
    kind: Optional[str] = None
    sigma: float = 1.5
    window: int = 9
    degree: int = 2
    rate: float = 25.0
    min_cutoff: float = 1.0
    beta: float = 0.0
    d_cutoff: float = 1.0
    fix_bones: bool = False
    edges: Sequence[Sequence[int]] = H36M_EDGES
    _coef: Dict[str, torch.Tensor] = field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {self.kind!r}")
        self.table = gauss_table(self.sigma) if self.kind == "gauss" else savgol_table(self.window, self.degree) if self.kind == "savgol" \
            else None
        if self.kind == "one_euro":
            v = (float(self.rate), float(self.min_cutoff), float(self.beta), float(self.d_cutoff))
            if not (all(math.isfinite(a) for a in v) and v[0] > 0 and v[1] > 0 and v[3] > 0 and v[2] >= 0):
                raise ValueError(f"one_euro needs finite rate, min_cutoff, d_cutoff > 0 and beta >= 0, got {v}")
        if self.fix_bones:                   # the order and uniqueness of the list; the joint count is checked against the poses in apply
            e = np.asarray(self.edges)
            check_edges(e, int(e.max()) + 1 if e.size and e.ndim == 2 else 0)

    @property
    def causal(self) -> bool:
        return self.kind in (None, "one_euro") or self.look_ahead == 0

    @property
    def look_ahead(self) -> int:
        """R: how many later frames an output frame waits for."""
        return (self.table.shape[0] - 1) // 2 if self.table is not None else 0

    def describe(self) -> str:
        if self.kind == "gauss":
            s = f"gauss sigma={self.sigma:g} W={self.table.shape[0]}"
        elif self.kind == "savgol":
            s = f"savgol W={self.window} degree={self.degree}"
        elif self.kind == "one_euro":
            s = f"one_euro rate={self.rate:g} min_cutoff={self.min_cutoff:g} beta={self.beta:g} d_cutoff={self.d_cutoff:g}"
        else:
            s = "no filter"
        s += f" ({'causal' if self.causal else 'not causal'}, look-ahead R={self.look_ahead})"
        return s + (f" + constant bone lengths over {len(self.edges)} edges (per-sequence mean)" if self.fix_bones else "")

    def apply(self, poses: torch.Tensor, table) -> Tuple[torch.Tensor, Dict[str, object]]:
        """``poses`` (F, J, 3) fp32 on a GPU, ``table`` a ``SequenceTable``, a pair ``(seq_start, idx)`` or ``DeviceTables``.  Returns
        ``(poses_post, info)``; ``poses`` is not modified (with no filter and no bone step ``poses_post`` IS ``poses``).  ``info``:
        ``tables``, ``short_rows`` (the device int32 pair of ``fir_sequences``, zeros for the other kinds: nothing here waits for the
        GPU) and, with ``fix_bones``, ``stats`` (those the rebuild used: of the filtered poses).  The FIR table is uploaded once per
        device and kept."""
        tables = DeviceTables.of(table, poses.device)
        _check_poses(poses, tables, "PostProcess.apply")
        out = poses
        short = None
        if self.table is not None:
            key = str(poses.device)
            if key not in self._coef:
                self._coef[key] = upload_coef(self.table, poses.device)
            out, short = fir_sequences(out, tables, self._coef[key])
        elif self.kind == "one_euro":
            out = one_euro_sequences(out, tables, self.rate, self.min_cutoff, self.beta, self.d_cutoff)
        info: Dict[str, object] = {"tables": tables,
                                   "short_rows": short if short is not None else torch.zeros(2, dtype=torch.int32, device=poses.device)}
        if self.fix_bones:
            out, info["stats"] = fix_bone_lengths(out, tables, self.edges)
        return out, info


FLAG_DEFAULTS = dict(smooth_sigma=1.5, smooth_window=9, smooth_degree=2, smooth_rate=25.0, one_euro_min_cutoff=1.0, one_euro_beta=0.0,
                     one_euro_d_cutoff=1.0)


def add_parameter_flags(parser) -> None:
    """The filter's parameter flags, shared by ``results`` and ``predict``; absent from the namespace unless given."""
    import argparse
    s = argparse.SUPPRESS
    parser.add_argument("--smooth-sigma", type=float, default=s, help="gauss: sigma in frames (default 1.5); W = 2 ceil(3 sigma) + 1")
    parser.add_argument("--smooth-window", type=int, default=s, help="savgol: window W, odd, <= 63 (default 9)")
    parser.add_argument("--smooth-degree", type=int, default=s, help="savgol: polynomial degree p < W (default 2)")
    parser.add_argument("--smooth-rate", type=float, default=s, help="one_euro: frames per second (default 25.0: 50 Hz over FRAME_SKIP = 2)")
    parser.add_argument("--one-euro-min-cutoff", type=float, default=s, help="one_euro: minimum cutoff in Hz (default 1.0)")
    parser.add_argument("--one-euro-beta", type=float, default=s, help="one_euro: speed coefficient (default 0.0)")
    parser.add_argument("--one-euro-d-cutoff", type=float, default=s, help="one_euro: cutoff of the derivative in Hz (default 1.0)")


def post_from_args(args, kind: Optional[str], fix_bones: bool, error) -> Optional[PostProcess]:
    """The ``PostProcess`` of a parsed command line, or None when neither a filter nor the bone step is asked for; ``error`` (the
    parser's) is called if a parameter flag is given without the filter it belongs to, or a parameter is refused."""
    given = [k for k in FLAG_DEFAULTS if hasattr(args, k)]
    owner = {"smooth_sigma": "gauss", "smooth_window": "savgol", "smooth_degree": "savgol", "smooth_rate": "one_euro",
             "one_euro_min_cutoff": "one_euro", "one_euro_beta": "one_euro", "one_euro_d_cutoff": "one_euro"}
    for k in given:
        if kind != owner[k]:
            error(f"--{k.replace('_', '-')} belongs to the {owner[k]} filter, which is not selected")
    if kind is None and not fix_bones:
        return None
    v = {k: getattr(args, k, d) for k, d in FLAG_DEFAULTS.items()}
    try:
        return PostProcess(kind=kind, sigma=v["smooth_sigma"], window=v["smooth_window"], degree=v["smooth_degree"], rate=v["smooth_rate"],
                           min_cutoff=v["one_euro_min_cutoff"], beta=v["one_euro_beta"], d_cutoff=v["one_euro_d_cutoff"],
                           fix_bones=bool(fix_bones))
    except ValueError as exc:
        error(str(exc))
