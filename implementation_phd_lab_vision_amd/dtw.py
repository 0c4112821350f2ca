"""Forecast error after dynamic time warping, per action and per horizon.

``results --protocols --pred-len P`` compares predicted frame ``I+k`` with ground-truth frame ``I+k``: a rollout that produces the right
motion too slowly scores as badly as one that produces the wrong motion.  Dynamic time warping (DTW) tells the two apart.  Per clip,
``Y_0..Y_{P-1}`` the predicted poses and ``X_0..X_{Q-1}`` the ground truth's frames ``i0 .. i0+Q-1`` (read as fp32, computed in fp64):

* two cost matrices, ``C1[i][j]`` = P1 and ``C2[i][j]`` = P2 of ``(Y_i, X_j)`` as ``protocols.py`` defines them, one similarity fit per
  cell giving both;
* ``band < 0`` allows every cell, ``band >= 0`` the cells with ``|i - j| <= band``; ``band`` must be ``>= |P - Q|``;
* per metric a closed-ended DP: ``D[0][0] = C[0][0]``, ``D[i][j] = C[i][j]`` + the best predecessor among ``(i-1,j-1)``, ``(i-1,j)``,
  ``(i,j-1)`` that exist and are allowed, taken in that order, a later one replacing the current one only if strictly smaller: ties go
  diagonal, then up, then left, and a NaN never replaces anything;
* the path is the backtrack from ``(P-1, Q-1)`` to ``(0, 0)``, ``L`` cells with ``max(P, Q) <= L <= P+Q-1``.

Per clip and metric: ``total = D[P-1][Q-1]``, ``L``, and per predicted frame k over the path cells with ``i = k``: ``cost_sum[k]`` (the
sum of ``C[i][j]``), ``cells[k]`` (their count) and ``lag_sum[k]`` (the sum of ``i - j``).  The **DTW error** of a clip is ``total / L``,
at horizon k ``cost_sum[k] / cells[k]``; the **lag** at horizon k is ``lag_sum[k] / cells[k]`` frames, positive when the prediction runs
behind the ground truth's clock (it is slow).  A group's value is the sum of its clips' values over its clip count, ``all`` the same
over every clip, the action mean the plain mean of the per-action values (``protocols.py``'s conventions, whose ``action_name`` and
``action_groups`` name the groups).

One ``r50_op_dtw_protocols`` call per batch (one workgroup per clip: cost matrices, the DP's diagonals and the choices in LDS; then one
workgroup per group) adds into an fp64 device accumulator that is read once per pass.  No CPU fallback.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, clip_pass, protocols
from .protocols import ROOT_JOINT

MAX_LEN = 64                                  # r50_op_dtw_protocols' limit on P and Q


def acc_size(n_groups: int, p: int) -> int:
    """The accumulator's fp64 values: (G, 2, 1 + 2P) sums, then G clip counts."""
    return n_groups * 2 * (1 + 2 * p) + n_groups


def _launch(pred: torch.Tensor, gt: torch.Tensor, i0: int, q: int, group: torch.Tensor, n_groups: int, acc: torch.Tensor, band: int,
            root: int, clip_out: Optional[torch.Tensor], path_out: Optional[torch.Tensor]) -> torch.Tensor:
    """Shape, dtype and device checks (in the style of ``protocols._launch``), then one call; the group VALUES are the caller's to have
    checked.  Returns the per-clip records (``clip_out``, or a fresh tensor)."""
    b, p, t, j = protocols.check_poses(pred, gt, root)
    if b < 1 or not 1 <= p <= MAX_LEN or not 1 <= q <= MAX_LEN or i0 < 0 or i0 + q > t:
        raise ValueError(f"need B >= 1, 1 <= P, Q <= {MAX_LEN} and 0 <= i0, i0 + Q <= T (got B={b}, P={p}, Q={q}, i0={i0}, T={t})")
    if 0 <= band < abs(p - q):
        raise ValueError(f"a band >= 0 must be >= |P - Q| = {abs(p - q)}, got {band}")
    protocols.check_group_acc(b, group, n_groups, acc, acc_size(n_groups, p))
    if clip_out is not None and (clip_out.dtype != torch.float64 or tuple(clip_out.shape) != (b, 2, 2 + 3 * p)
                                 or not clip_out.is_contiguous() or clip_out.device != pred.device):
        raise ValueError(f"clip_out must be ({b}, 2, {2 + 3 * p}) contiguous fp64 on pred's device")
    if path_out is not None and (path_out.dtype != torch.int32 or tuple(path_out.shape) != (b, 2, p + q - 1, 2)
                                 or not path_out.is_contiguous() or path_out.device != pred.device):
        raise ValueError(f"path_out must be ({b}, 2, {p + q - 1}, 2) contiguous int32 on pred's device")
    protocols.check_one_gpu(pred, gt, group, acc)
    if clip_out is None:
        clip_out = torch.empty((b, 2, 2 + 3 * p), dtype=torch.float64, device=pred.device)
    rc = _lib.load_library().r50_op_dtw_protocols(pred.data_ptr(), gt.data_ptr(), group.data_ptr(), b, p, t, int(i0), int(q), j, int(root),
                                                  int(band), int(n_groups), clip_out.data_ptr(),
                                                  path_out.data_ptr() if path_out is not None else None, acc.data_ptr(),
                                                  torch.cuda.current_stream(pred.device).cuda_stream)
    _lib.check(rc, None, "r50_op_dtw_protocols")
    return clip_out


def add_dtw_sums(pred: torch.Tensor, gt: torch.Tensor, i0: int, q: int, group: torch.Tensor, n_groups: int, acc: torch.Tensor,
                 band: int = -1, root: int = ROOT_JOINT, clip_out: Optional[torch.Tensor] = None,
                 path_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acc (G*2*(1+2P) + G) fp64 on the device += the DTW sums of one batch: pred (B, P, J, 3) fp32 is warped onto frames i0 .. i0+Q-1 of
    gt (B, T, J, 3) fp32; group (B,) int32 on the device, each value in [0, n_groups) (checked on the host before the launch: one read).
    With V = 1 + 2P, ``acc[(g*2 + m)*V]`` += total / L, ``acc[(g*2 + m)*V + 1 + k]`` += cost_sum[k] / cells[k],
    ``acc[(g*2 + m)*V + 1 + P + k]`` += lag_sum[k] / cells[k], ``acc[2*G*V + g]`` += the clips of g.  ``clip_out`` (B, 2, 2 + 3P) fp64
    receives ``[total, L, cost_sum[P], cells[P], lag_sum[P]]`` per clip and metric and is returned (a fresh tensor when None);
    ``path_out`` (B, 2, P+Q-1, 2) int32, if given, the paths' (i, j) pairs from (0, 0) onward, -1 past L."""
    protocols.check_group_values(group, n_groups)
    return _launch(pred, gt, int(i0), int(q), group, int(n_groups), acc, int(band), int(root), clip_out, path_out)


def _values(sums: np.ndarray, n_groups: int, p: int):
    """(dtw (G, 2), dtw_all (2,), future (G, P, 2), future_all (P, 2), lag (G, P, 2), lag_all (P, 2), clips (G,)) from one accumulator;
    a group without clips gets NaN."""
    v = 1 + 2 * p
    s = sums[:n_groups * 2 * v].reshape(n_groups, 2, v)
    clips = sums[n_groups * 2 * v:]
    per_group = np.full_like(s, np.nan)
    has = clips > 0
    per_group[has] = s[has] / clips[has, None, None]
    all_ = s.sum(axis=0) / clips.sum()
    split = lambda a: (a[..., 0], np.swapaxes(a[..., 1:1 + p], -1, -2), np.swapaxes(a[..., 1 + p:], -1, -2))   # noqa: E731
    d, f, lag = split(per_group)
    da, fa, la = split(all_)
    return d, da, f, fa, lag, la, clips


@torch.no_grad()
def evaluate_dtw(head, store, groups: Sequence[int], group_names: Sequence[str], input_len: int, pred_len: int, band: int = -1,
                 batch_size: int = 256) -> Dict[str, object]:
    """The DTW error and lag of ``head``'s forecasts over every item of ``store`` (a ``DeviceFeatureStore``) once, in store order,
    ``batch_size`` clips per batch (the last kept even if short): the P poses of ``head.rollout(feats, input_len, pred_len)[1]`` warped
    onto frames I .. I+P-1 of the ground truth (``i0 = I``, ``Q = P``).  ``groups[i]`` in ``[0, len(group_names))`` is item i's group
    (``protocols.action_groups``).  Returns (fp64; metres, and frames for the lags; [.., 2] = [p1, p2])::

        group_names [G], clips (G,) int64, band
        dtw (G, 2) = total / L per group;  dtw_all (2,);  dtw_mean (2,) = the plain mean over groups
        dtw_future (G, P, 2), dtw_future_all (P, 2)       -- cost_sum[k] / cells[k]
        lag (G, P, 2), lag_all (P, 2)                     -- lag_sum[k] / cells[k], positive = the prediction is slow
        plain_future_all (P, 2), plain_all (2,)           -- the unwarped P1 / P2 per horizon and their mean over the horizons, of the
                                                             same rollouts in the same pass (``evaluate_protocols``' arithmetic)

    A group without clips gets NaN and stays out of the mean.  The accumulators are read back once per pass."""
    n_groups = len(group_names)
    ids, i_len, p_len, _ = clip_pass.check(store, input_len, pred_len, batch_size, groups, n_groups, max_pred_len=MAX_LEN)
    dev = head._device
    with torch.cuda.device(dev):
        acc = torch.zeros(acc_size(n_groups, p_len), dtype=torch.float64, device=dev)
        acc_plain = torch.zeros(2 * n_groups * p_len + n_groups, dtype=torch.float64, device=dev)
        for feats, gt, group in clip_pass.batches(head, store, batch_size, ids):
            pred = head.rollout(feats, i_len, p_len)[1]
            _launch(pred, gt, i_len, p_len, group, n_groups, acc, int(band), ROOT_JOINT, None, None)
            protocols._launch(pred, gt, i_len, group, n_groups, acc_plain, ROOT_JOINT)
        sums = torch.cat([acc, acc_plain]).cpu().numpy()
    d, da, f, fa, lag, la, clips = _values(sums[:acc.numel()], n_groups, p_len)
    plain_all = protocols._values(sums[acc.numel():], n_groups, p_len)[1]
    has = clips > 0
    return {"group_names": list(group_names), "clips": clips.round().astype(np.int64), "band": int(band), "dtw": d, "dtw_all": da,
            "dtw_mean": d[has].mean(axis=0), "dtw_future": f, "dtw_future_all": fa, "lag": lag, "lag_all": la,
            "plain_future_all": plain_all, "plain_all": plain_all.mean(axis=0)}


def dtw_lines(res: Dict[str, object], input_len: int, pred_len: int) -> List[str]:
    """The printed lines of ``--dtw`` from an ``evaluate_dtw`` result: the ``DTW metrics`` line (all clips: the warped P1 / P2 and, after
    ``plain``, the unwarped horizon means of the same rollouts), one indented line per action, and the ``DTW horizons`` line with the
    warped error in mm and the lag in frames (signed: positive = the prediction is slow) at horizons 1, 5, 10 and P."""
    clips = res["clips"]
    da, pa = res["dtw_all"], res["plain_all"]
    band = "none" if res["band"] < 0 else str(int(res["band"]))
    lines = [f"DTW metrics | input {input_len} | pred {pred_len} | band {band} | clips {int(clips.sum())} | all: p1 (mm) {da[0] * 1000.0:.2f} "
             f"| p2 (mm) {da[1] * 1000.0:.2f} | plain p1 (mm) {pa[0] * 1000.0:.2f} | p2 (mm) {pa[1] * 1000.0:.2f}"]
    for name, c, (p1, p2) in zip(res["group_names"], clips, res["dtw"]):
        lines.append(f"  {name} | clips {int(c)} | dtw p1 (mm) {p1 * 1000.0:.2f} | dtw p2 (mm) {p2 * 1000.0:.2f}")
    hs = sorted({h for h in (1, 5, 10, pred_len) if h <= pred_len})
    fa, la = res["dtw_future_all"], res["lag_all"]
    parts = [f"p{m + 1} (mm) " + " | ".join(f"@{h}: {fa[h - 1, m] * 1000.0:.2f}" for h in hs) for m in (0, 1)]
    parts += [f"lag p{m + 1} (frames) " + " | ".join(f"@{h}: {la[h - 1, m]:+.2f}" for h in hs) for m in (0, 1)]
    lines.append("DTW horizons | " + " | ".join(parts))
    return lines


def dtw_arrays(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``.npz`` keys of ``--dtw``: ``dtw_actions`` (G,) str, ``dtw_clips`` (G,) int64, ``dtw_band`` () int64, and fp32 ``dtw`` (G, 2),
    ``dtw_all`` (2,), ``dtw_future`` (G, P, 2), ``dtw_future_all`` (P, 2) in metres and ``dtw_lag`` (G, P, 2), ``dtw_lag_all`` (P, 2) in
    frames; [.., 2] = [p1, p2]."""
    out = {"dtw_actions": np.array([str(n) for n in res["group_names"]], dtype=str),
           "dtw_clips": np.asarray(res["clips"], dtype=np.int64), "dtw_band": np.array(int(res["band"]), dtype=np.int64)}
    for key, src in (("dtw", "dtw"), ("dtw_all", "dtw_all"), ("dtw_future", "dtw_future"), ("dtw_future_all", "dtw_future_all"),
                     ("dtw_lag", "lag"), ("dtw_lag_all", "lag_all")):
        out[key] = np.asarray(res[src], dtype=np.float32)
    return out
