"""Confidence intervals and the paired comparison of two models by a stratified cluster bootstrap (INTEGRATION.md section AC).

Every report of ``results`` prints point values.  A cache cuts a video into clips of ``seq_len`` frames at a stride of a few frames, so up
to eight clips share a frame and the clips of a take are strongly dependent: a standard error over clips overstates the certainty.  Here
whole UNITS -- sequences (subject, action with trial, camera), takes (all cameras of one motion) or, for comparison, clips -- are
resampled with replacement inside each STRATUM (an action, ``protocols.action_name``), and the table is recomputed for every replicate.
With a second head both models' columns sit side by side in the unit table, so one launch draws the same units for both and the interval
is on the difference (paired).

* ``UnitTable``               host numpy: which unit a clip belongs to, the units sorted by (stratum, key), ``stratum_start``.
* ``collect_clip_scores``     one pass per head through ``clip_pass``: P1 / P2 per clip (``r50_op_pose_protocols`` with one group per clip),
                              read back ONCE per pass -- the pass's single host synchronisation.
* ``unit_rows``               clip rows -> unit rows on the host in fp64, ascending clip order; the last column holds the unit's clips.
* ``bootstrap_sums``          the checked wrapper of ``r50_op_bootstrap_sums`` (include/r50_bootstrap.h): (R, G, M) replicate sums, the
                              multiplicities in LDS, no (R, U) matrix, the same bits on every run and under every cut of [r0, r0 + R).
                              It does not hold the host.  There is no CPU fallback.
* ``statistics``              torch on the device: values, standard errors (ddof 1), percentile intervals from order statistics without
                              interpolation, ``p_better``; one small read-back.
* ``evaluate_bootstrap``, ``bootstrap_lines``, ``bootstrap_npz``     the report behind ``results --bootstrap R``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, clip_pass, protocols
from .sequences import sequence_key

UNIT_KINDS = ("sequence", "take", "clip")
MAX_UNITS = 1 << 24                            # r50_op_bootstrap_sums' limits
MAX_COLUMNS = 4096
MAX_WINDOW = 32768
MAX_ELEMENTS = 1 << 40


def _unit_key(clip: dict, unit: str, item: int) -> tuple:
    subject, action, cam = sequence_key(clip)
    if unit == "sequence":
        return subject, action, cam
    if unit == "take":
        return subject, action
    return subject, action, cam, int(clip["start"]), item


@dataclass
class UnitTable:
    """U resampling units in G strata over N clips: ``unit_of_clip`` (N,) int32, ``stratum_start`` (G+1,) int32 -- stratum g is the units
    ``stratum_start[g]:stratum_start[g+1]`` --, ``stratum_names`` [G] sorted, ``unit_keys`` [U], the units sorted by (stratum, key)."""
    unit: str
    unit_of_clip: np.ndarray
    stratum_start: np.ndarray
    stratum_names: List[str]
    unit_keys: List[tuple]
    _device_starts: dict = field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self):
        ss = np.asarray(self.stratum_start)
        if ss.ndim != 1 or ss.size < 2 or ss.dtype != np.int32 or ss[0] != 0 or np.any(np.diff(ss.astype(np.int64)) < 1):
            raise ValueError("UnitTable: stratum_start must be (G+1,) int32, start at 0 and give every stratum at least one unit")
        if int(ss[-1]) > MAX_UNITS:
            raise ValueError(f"UnitTable: {int(ss[-1])} units exceed the op's limit of 2^24")
        if len(self.stratum_names) != ss.size - 1:
            raise ValueError(f"UnitTable: {len(self.stratum_names)} stratum names for {ss.size - 1} strata")
        uc = np.asarray(self.unit_of_clip)
        if uc.ndim != 1 or uc.size < 1 or uc.min() < 0 or uc.max() >= int(ss[-1]) or np.unique(uc).size != int(ss[-1]):
            raise ValueError("UnitTable: unit_of_clip must name every unit in [0, U) at least once")

    @property
    def units(self) -> int:
        return int(self.stratum_start[-1])

    @property
    def strata(self) -> int:
        return int(self.stratum_start.shape[0]) - 1

    @property
    def clips(self) -> int:
        return int(self.unit_of_clip.shape[0])

    @property
    def largest_stratum(self) -> int:
        return int(np.diff(self.stratum_start).max())

    @property
    def stratum_of_unit(self) -> np.ndarray:
        return np.repeat(np.arange(self.strata, dtype=np.int64), np.diff(self.stratum_start))

    @classmethod
    def from_clips(cls, clips: Sequence[dict], unit: str = "sequence") -> "UnitTable":
        """``clips``: index entries (``DeviceFeatureStore.item_clips()``).  Refuses an unknown unit kind, an empty table and U > 2^24."""
        if unit not in UNIT_KINDS:
            raise ValueError(f"unit: expected one of {UNIT_KINDS}, got {unit!r}")
        if len(clips) < 1:
            raise ValueError("UnitTable: no clips")
        full = [(protocols.action_name(c["action"]), _unit_key(c, unit, i)) for i, c in enumerate(clips)]
        keys = sorted(set(full))
        if len(keys) > MAX_UNITS:
            raise ValueError(f"UnitTable: {len(keys)} units exceed the op's limit of 2^24")
        pos = {k: u for u, k in enumerate(keys)}
        names = sorted({k[0] for k in keys})
        first = np.searchsorted(np.array([names.index(k[0]) for k in keys], dtype=np.int64), np.arange(len(names) + 1))
        return cls(unit=unit, unit_of_clip=np.array([pos[k] for k in full], dtype=np.int32), stratum_start=first.astype(np.int32),
                   stratum_names=names, unit_keys=[k[1] for k in keys])

    @classmethod
    def from_sizes(cls, sizes: Sequence[int], unit: str = "clip") -> "UnitTable":
        """One clip per unit, strata of the given sizes (benchmarks and tests of the op)."""
        sizes = [int(s) for s in sizes]
        if not sizes or min(sizes) < 1:
            raise ValueError("UnitTable: every stratum needs at least one unit")
        start = np.concatenate([[0], np.cumsum(sizes)])
        if int(start[-1]) > MAX_UNITS:
            raise ValueError(f"UnitTable: {int(start[-1])} units exceed the op's limit of 2^24")
        u = int(start[-1])
        return cls(unit=unit, unit_of_clip=np.arange(u, dtype=np.int32), stratum_start=start.astype(np.int32),
                   stratum_names=[f"stratum{g}" for g in range(len(sizes))], unit_keys=[(i,) for i in range(u)])

    def device_starts(self, device) -> torch.Tensor:
        """``stratum_start`` on ``device``, uploaded once per device (the table was checked when it was made)."""
        key = str(torch.device(device))
        if key not in self._device_starts:
            self._device_starts[key] = torch.from_numpy(np.ascontiguousarray(self.stratum_start)).to(device)
        return self._device_starts[key]


def horizons(pred_len: int) -> List[int]:
    """The horizons the ``Rollout protocol metrics`` line prints."""
    return sorted({h for h in (1, 5, 10, int(pred_len)) if h <= int(pred_len)})


def score_names(pred_len: int) -> List[str]:
    return ["p1", "p2"] + [f"{m}@{h}" for h in horizons(pred_len) for m in ("p1", "p2")]


@torch.no_grad()
def collect_clip_scores(head, store, input_len: int = 0, pred_len: int = 0, batch_size: int = 256) -> np.ndarray:
    """(N, K) fp64, metres, one row per item of ``store`` in store order: the reconstruction's P1 and P2 (the mean over the T frames)
    and, with ``pred_len > 0``, P1 / P2 at ``horizons(pred_len)``; the columns are ``score_names(pred_len)``.  One
    ``r50_op_pose_protocols`` launch per batch and scored span with ``group = arange(b)`` and ``n_groups = b``; the batches' rows stay on
    the device and come to the host in ONE read-back per pass."""
    _, i_len, p_len, seq_len = clip_pass.check(store, input_len, pred_len, batch_size, forecast_required=False)
    dev = head._device
    hs = horizons(p_len)
    rows = []
    with torch.cuda.device(dev):
        each = torch.arange(batch_size, dtype=torch.int32, device=dev)
        pick = torch.tensor([h - 1 for h in hs], dtype=torch.long, device=dev)
        for feats, gt, _ in clip_pass.batches(head, store, batch_size):
            b = int(gt.shape[0])
            acc_r = torch.zeros(2 * b * seq_len + b, dtype=torch.float64, device=dev)
            protocols._launch(head.joints(feats), gt, 0, each[:b], b, acc_r, protocols.ROOT_JOINT)
            parts = [acc_r[:2 * b * seq_len].view(b, seq_len, 2).mean(dim=1)]
            if p_len:
                acc_f = torch.zeros(2 * b * p_len + b, dtype=torch.float64, device=dev)
                protocols._launch(head.rollout(feats, i_len, p_len)[1], gt, i_len, each[:b], b, acc_f, protocols.ROOT_JOINT)
                parts.append(acc_f[:2 * b * p_len].view(b, p_len, 2).index_select(1, pick).reshape(b, 2 * len(hs)))
            rows.append(torch.cat(parts, dim=1))
        return torch.cat(rows, dim=0).cpu().numpy()


def unit_rows(scores: np.ndarray, table: UnitTable) -> np.ndarray:
    """(U, K+1) fp64: the clip rows of every unit added up in ascending clip order, and the unit's clips in the last column."""
    scores = np.asarray(scores, dtype=np.float64)
    if scores.ndim != 2 or scores.shape[0] != table.clips:
        raise ValueError(f"scores (N, K) with N = {table.clips} clips expected, got {scores.shape}")
    v = np.zeros((table.units, scores.shape[1] + 1), dtype=np.float64)
    np.add.at(v[:, :-1], table.unit_of_clip, scores)               # unbuffered: one add per clip, in clip order
    v[:, -1] = np.bincount(table.unit_of_clip, minlength=table.units)
    return v


def point_sums(v: np.ndarray, table: UnitTable) -> np.ndarray:
    """(G, M) fp64: the op's sums at c = 1 -- the units of a stratum added up in ascending order from +0.0."""
    out = np.zeros((table.strata, v.shape[1]), dtype=np.float64)
    np.add.at(out, table.stratum_of_unit, np.asarray(v, dtype=np.float64))
    return out


def bootstrap_sums(v: torch.Tensor, table: UnitTable, R: int, seed: int, r0: int = 0, window: int = MAX_WINDOW, counts: bool = False):
    """out (R, G, M) fp64 on v's device [, counts (R, U) int32]: replicate ``r0 + r`` of the stratified bootstrap of the unit rows
    ``v`` (U, M) fp64 (include/r50_bootstrap.h).  The bits do not depend on ``window``; a window above the table's largest stratum is
    lowered to it, which only spares LDS.  One launch on the current stream, no host synchronisation.  No CPU fallback."""
    if not isinstance(table, UnitTable):
        raise ValueError("table: a UnitTable expected (its stratum_start was checked on the host)")
    if not isinstance(v, torch.Tensor) or v.dim() != 2 or v.dtype != torch.float64:
        raise ValueError(f"v (U, M) fp64 expected, got {tuple(v.shape) if isinstance(v, torch.Tensor) else type(v)} "
                         f"{getattr(v, 'dtype', None)}")
    u, m = int(v.shape[0]), int(v.shape[1])
    if u != table.units or not 1 <= m <= MAX_COLUMNS:
        raise ValueError(f"v must have the table's {table.units} rows and 1 <= M <= {MAX_COLUMNS} columns, got {(u, m)}")
    reps, first, seed = int(R), int(r0), int(seed)
    if reps < 1 or first < 0 or first + reps >= 1 << 63:
        raise ValueError(f"need R >= 1, r0 >= 0 and r0 + R below 2^63 (got R={reps}, r0={first})")
    if reps * table.strata * m >= MAX_ELEMENTS or reps * u >= MAX_ELEMENTS:
        raise ValueError("R * G * M and R * U must stay below 2^40")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
    if not 1 <= int(window) <= MAX_WINDOW:
        raise ValueError(f"window must lie in [1, {MAX_WINDOW}], got {window}")
    if v.device.type != "cuda":
        raise ValueError("v must be on a GPU: there is no CPU fallback")
    if not v.is_contiguous():
        raise ValueError("v must be contiguous")
    with torch.cuda.device(v.device):
        starts = table.device_starts(v.device)
        out = torch.empty((reps, table.strata, m), dtype=torch.float64, device=v.device)
        cnt = torch.empty((reps, u), dtype=torch.int32, device=v.device) if counts else None
        rc = _lib.load_library().r50_op_bootstrap_sums(v.data_ptr(), starts.data_ptr(), u, table.strata, m, first, reps, seed,
                                                       min(int(window), table.largest_stratum), out.data_ptr(),
                                                       None if cnt is None else cnt.data_ptr(),
                                                       torch.cuda.current_stream(v.device).cuda_stream)
    _lib.check(rc, None, "r50_op_bootstrap_sums")
    return (out, cnt) if counts else out


def _rows(s: torch.Tensor) -> torch.Tensor:
    """(..., G, M) sums whose last column is the count -> (..., G + 2, M - 1) values: all, the action mean, every stratum.  The sums
    over strata run in ascending stratum order, one add at a time, so a numpy restatement gives the same bits; for the same reason
    no divisor is a Python number (torch multiplies a device tensor by a Python scalar's reciprocal instead of dividing by it)."""
    val = s[..., :, :-1] / s[..., :, -1:]
    tot, mean = s[..., 0, :].clone(), val[..., 0, :].clone()
    for g in range(1, s.shape[-2]):
        tot = tot + s[..., g, :]
        mean = mean + val[..., g, :]
    all_ = tot[..., :-1] / tot[..., -1:]
    mean = mean / torch.full((), float(s.shape[-2]), dtype=s.dtype, device=s.device)
    return torch.cat([all_.unsqueeze(-2), mean.unsqueeze(-2), val], dim=-2)


def order_indices(reps: int, level: float) -> Tuple[int, int]:
    """The sorted replicates a percentile interval takes: ``ceil(q R) - 1`` clamped to [0, R-1] for q = (1 - level) / 2 and 1 - q.
    ``level`` counts as the decimal number it prints as and the products are exact rationals: in floating point (1 - 0.95) / 2 lies
    above 0.025, and R = 1000 would give the lower index 25 beside the upper 974 instead of 24."""
    q = (1 - Fraction(repr(float(level)))) / 2
    clamp = lambda i: min(max(i, 0), reps - 1)                     # noqa: E731
    return clamp(math.ceil(q * reps) - 1), clamp(math.ceil((1 - q) * reps) - 1)


def statistics_device(sums: torch.Tensor, point: torch.Tensor, level: float, pairs: int = 0) -> Dict[str, torch.Tensor]:
    """``statistics`` without the read-back: every entry a device tensor, nothing holds the host."""
    if sums.dim() != 3 or point.dim() != 2 or tuple(point.shape) != tuple(sums.shape[1:]) or sums.shape[2] < 2:
        raise ValueError(f"sums (R, G, M) and point_sums (G, M) with M >= 2 expected, got {tuple(sums.shape)}, {tuple(point.shape)}")
    if sums.dtype != torch.float64 or point.dtype != torch.float64 or sums.device != point.device:
        raise ValueError("sums and point_sums must be fp64 on one device")
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must lie in (0, 1), got {level}")
    k = int(sums.shape[2]) - 1
    if pairs and 2 * int(pairs) != k:
        raise ValueError(f"pairs = {pairs} needs 2 * pairs = {k} value columns")
    rep, pt = _rows(sums), _rows(point)
    reps = int(rep.shape[0])
    lo, hi = order_indices(reps, float(level))
    srt = torch.sort(rep, dim=0).values
    nan = torch.full_like(pt, float("nan"))
    out = {"point": pt, "se": rep.std(dim=0, unbiased=True) if reps > 1 else nan, "lo": srt[lo], "hi": srt[hi]}
    if pairs:
        d = rep[..., pairs:2 * pairs] - rep[..., :pairs]
        ds = torch.sort(d, dim=0).values
        p = ((d < 0).sum(dim=0).to(torch.float64) + 0.5 * (d == 0).sum(dim=0).to(torch.float64)) / torch.full((), float(reps), dtype=torch.float64, device=d.device)
        out.update(diff=pt[..., pairs:2 * pairs] - pt[..., :pairs], diff_se=d.std(dim=0, unbiased=True) if reps > 1 else nan[..., :pairs],
                   diff_lo=ds[lo], diff_hi=ds[hi], p_better=p, p_two_sided=2.0 * torch.minimum(p, 1.0 - p))
    return out


def statistics(sums: torch.Tensor, point_sums: torch.Tensor, level: float = 0.95, pairs: int = 0) -> Dict[str, np.ndarray]:
    """The statistics of a replicate table ``sums`` (R, G, M) whose last column is the count, beside the point sums (G, M) (the same
    formulas at c = 1).  Rows: all (the sum over strata of the sums over the sum of the counts), the action mean (the plain mean over
    strata), every stratum (sum / count).  Per row and value column: ``point``, ``se`` (ddof 1), ``lo`` / ``hi`` (order statistics, no
    interpolation: ``order_indices``).  With ``pairs`` = K the first K value columns are model A's and the next K model B's:
    ``diff`` = B - A with ``diff_se`` / ``diff_lo`` / ``diff_hi``, ``p_better`` = the share of replicates with B - A < 0 plus half
    the ties, ``p_two_sided`` = 2 min(p, 1 - p).  Computed on the device; ONE read-back of (G + 2) x a few columns."""
    dev = statistics_device(sums, point_sums, level, pairs)
    flat = torch.cat([t.reshape(-1) for t in dev.values()]).cpu().numpy()
    out, at = {}, 0
    for name, t in dev.items():
        out[name] = flat[at:at + t.numel()].reshape(tuple(t.shape))
        at += t.numel()
    return out


@torch.no_grad()
def evaluate_bootstrap(head, store, clips: Optional[Sequence[dict]] = None, reps: int = 1000, unit: str = "sequence", seed: int = 0,
                       level: float = 0.95, input_len: int = 0, pred_len: int = 0, batch_size: int = 256, compare=None,
                       design_effect: bool = True) -> Dict[str, object]:
    """The bootstrap report of ``head`` over every item of ``store``: ``clips`` = the items' index entries (default
    ``store.item_clips()``).  With ``compare`` (a second head) both models' columns go through ONE launch, so every replicate resamples
    the same units for both.  With ``unit`` = sequence or take and ``design_effect``, the clip-unit bootstrap of the same scores runs
    too, and ``design_effect`` = the width of this unit's interval on ``all: p1`` over the clip unit's.

    Returns (metres, fp64): ``metrics`` [K], ``rows`` = ["all", "action mean"] + the strata, ``units`` / ``clips`` per stratum,
    ``point`` / ``se`` / ``lo`` / ``hi`` (G+2, K) of ``head``; with ``compare`` also ``b_point`` / ``b_se`` / ``b_lo`` / ``b_hi`` and
    ``diff`` / ``diff_se`` / ``diff_lo`` / ``diff_hi`` / ``p_better`` / ``p_two_sided``; ``unit_table`` (U, M) as it was uploaded, the
    ``table``, the settings.  Host synchronisations: one read-back per head's pass, one of the statistics per bootstrap."""
    if int(reps) < 1:
        raise ValueError(f"reps must be >= 1, got {reps}")
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must lie in (0, 1), got {level}")
    clips = store.item_clips() if clips is None else clips
    if len(clips) != len(store):
        raise ValueError(f"{len(clips)} index entries for {len(store)} items")
    table = UnitTable.from_clips(clips, unit)
    names = score_names(pred_len if pred_len > 0 else 0)
    k = len(names)
    scores = [collect_clip_scores(h, store, input_len, pred_len, batch_size) for h in ([head] if compare is None else [head, compare])]
    dev = head._device

    def run(tab: UnitTable, pairs: int):
        rows = unit_rows(np.concatenate(scores, axis=1), tab)
        with torch.cuda.device(dev):
            vd = torch.from_numpy(rows).to(dev)
            sums = bootstrap_sums(vd, tab, int(reps), int(seed))
            return rows, statistics(sums, torch.from_numpy(point_sums(rows, tab)).to(dev), float(level), pairs)

    v, st = run(table, k if compare is not None else 0)
    out: Dict[str, object] = {"metrics": names, "rows": ["all", "action mean"] + list(table.stratum_names), "unit": unit,
                              "reps": int(reps), "seed": int(seed), "level": float(level), "table": table, "unit_table": v,
                              "units": np.diff(table.stratum_start).astype(np.int64),
                              "clips": point_sums(v, table)[:, -1].round().astype(np.int64)}
    for name in ("point", "se", "lo", "hi"):
        out[name] = st[name][:, :k]
        if compare is not None:
            out["b_" + name] = st[name][:, k:]
    if compare is not None:
        out.update({name: st[name] for name in ("diff", "diff_se", "diff_lo", "diff_hi", "p_better", "p_two_sided")})
    out["design_effect"] = None
    if design_effect and unit != "clip":
        _, by_clip = run(UnitTable.from_clips(clips, "clip"), k if compare is not None else 0)
        width = float(by_clip["hi"][0, 0] - by_clip["lo"][0, 0])
        out["clip_interval"] = np.array([by_clip["lo"][0, 0], by_clip["hi"][0, 0]])
        out["design_effect"] = float(out["hi"][0, 0] - out["lo"][0, 0]) / width if width > 0 else float("nan")
    return out


def _mm(x: float) -> str:
    return f"{x * 1000.0:.2f}"


def bootstrap_lines(res: Dict[str, object]) -> List[str]:
    """The printed lines: a header, one line for all clips, one for the action mean and one indented line per action; per metric the
    point value, its interval and standard error in mm, with a second model A, B, B - A with its interval, ``p_better`` and the
    two-sided p; with sequence or take units the design-effect line."""
    names, paired = res["metrics"], "diff" in res
    lines = [f"Bootstrap | unit {res['unit']} | units {int(res['units'].sum())} | strata {len(res['units'])} | clips {int(res['clips'].sum())} "
             f"| replicates {res['reps']} | seed {res['seed']} | level {res['level']:g}" + (" | paired: B - A" if paired else "")]
    for i, row in enumerate(res["rows"]):
        cells = []
        for j, name in enumerate(names):
            if paired:
                cells.append(f"{name} (mm) A {_mm(res['point'][i, j])} B {_mm(res['b_point'][i, j])} B-A {_mm(res['diff'][i, j])} "
                             f"[{_mm(res['diff_lo'][i, j])}, {_mm(res['diff_hi'][i, j])}] p_better {res['p_better'][i, j]:.3f} "
                             f"p {res['p_two_sided'][i, j]:.3f}")
            else:
                cells.append(f"{name} (mm) {_mm(res['point'][i, j])} [{_mm(res['lo'][i, j])}, {_mm(res['hi'][i, j])}] se {_mm(res['se'][i, j])}")
        head = f"Bootstrap | {row}" if i < 2 else f"  Bootstrap | {row} | units {int(res['units'][i - 2])} | clips {int(res['clips'][i - 2])}"
        lines.append(head + " | " + " | ".join(cells))
    if res.get("design_effect") is not None:
        lo, hi = res["clip_interval"]
        lines.append(f"Bootstrap | design effect | all: p1 interval width, {res['unit']} units over clip units: {res['design_effect']:.2f} "
                     f"(clip units: [{_mm(lo)}, {_mm(hi)}])")
    return lines


def bootstrap_npz(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``.npz`` keys: ``bootstrap_metrics`` (K,) and ``bootstrap_rows`` (G+2,) str, ``bootstrap_units`` / ``bootstrap_clips`` (G,),
    ``bootstrap_settings`` = [replicates, seed, level], ``bootstrap_unit``, ``bootstrap_point`` / ``_se`` / ``_lo`` / ``_hi`` (G+2, K)
    fp64 in metres; with a second model ``bootstrap_b_*`` and ``bootstrap_diff`` / ``_diff_se`` / ``_diff_lo`` / ``_diff_hi`` /
    ``_p_better`` / ``_p_two_sided``; with sequence or take units ``bootstrap_design_effect``."""
    out = {"bootstrap_metrics": np.array(res["metrics"], dtype=str), "bootstrap_rows": np.array([str(r) for r in res["rows"]], dtype=str),
           "bootstrap_units": np.asarray(res["units"], dtype=np.int64), "bootstrap_clips": np.asarray(res["clips"], dtype=np.int64),
           "bootstrap_settings": np.array([res["reps"], res["seed"], res["level"]], dtype=np.float64),
           "bootstrap_unit": np.array(res["unit"], dtype=str)}
    for name in ("point", "se", "lo", "hi", "b_point", "b_se", "b_lo", "b_hi", "diff", "diff_se", "diff_lo", "diff_hi", "p_better",
                 "p_two_sided"):
        if name in res:
            out["bootstrap_" + name] = np.asarray(res[name], dtype=np.float64)
    if res.get("design_effect") is not None:
        out["bootstrap_design_effect"] = np.array(res["design_effect"], dtype=np.float64)
    return out
