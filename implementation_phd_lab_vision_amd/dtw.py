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

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import protocols
from .protocols import MAX_JOINTS, ROOT_JOINT

MAX_LEN = 64                                  # r50_op_dtw_protocols' limit on P and Q


def acc_size(n_groups: int, p: int) -> int:
    """The accumulator's fp64 values: (G, 2, 1 + 2P) sums, then G clip counts."""
    return n_groups * 2 * (1 + 2 * p) + n_groups


def _launch(pred: torch.Tensor, gt: torch.Tensor, i0: int, q: int, group: torch.Tensor, n_groups: int, acc: torch.Tensor, band: int,
            root: int, clip_out: Optional[torch.Tensor], path_out: Optional[torch.Tensor]) -> torch.Tensor:
    """Shape, dtype and device checks (in the style of ``protocols._launch``), then one call; the group VALUES are the caller's to have
    checked.  Returns the per-clip records (``clip_out``, or a fresh tensor)."""
    if pred.dim() != 4 or gt.dim() != 4:
        raise ValueError(f"pred (B,P,J,3) and gt (B,T,J,3) expected, got {tuple(pred.shape)}, {tuple(gt.shape)}")
    b, p, j, _ = pred.shape
    t = gt.shape[1]
    if tuple(gt.shape) != (b, t, j, 3) or pred.shape[3] != 3 or pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError(f"pred (B,P,J,3) and gt (B,T,J,3) fp32 expected, got {tuple(pred.shape)} {pred.dtype}, {tuple(gt.shape)} {gt.dtype}")
    if not 1 <= j <= MAX_JOINTS or not 0 <= root < j:
        raise ValueError(f"need 1 <= J <= {MAX_JOINTS} and 0 <= root < J (got J={j}, root={root})")
    if b < 1 or not 1 <= p <= MAX_LEN or not 1 <= q <= MAX_LEN or i0 < 0 or i0 + q > t:
        raise ValueError(f"need B >= 1, 1 <= P, Q <= {MAX_LEN} and 0 <= i0, i0 + Q <= T (got B={b}, P={p}, Q={q}, i0={i0}, T={t})")
    if 0 <= band < abs(p - q):
        raise ValueError(f"a band >= 0 must be >= |P - Q| = {abs(p - q)}, got {band}")
    if n_groups < 1:
        raise ValueError("n_groups must be >= 1")
    if group.dtype != torch.int32 or tuple(group.shape) != (b,):
        raise ValueError(f"group must be ({b},) int32, got {tuple(group.shape)} {group.dtype}")
    if acc.dtype != torch.float64 or acc.numel() != acc_size(n_groups, p) or not acc.is_contiguous():
        raise ValueError(f"acc must be {acc_size(n_groups, p)} contiguous fp64 values")
    if clip_out is not None and (clip_out.dtype != torch.float64 or tuple(clip_out.shape) != (b, 2, 2 + 3 * p)
                                 or not clip_out.is_contiguous() or clip_out.device != pred.device):
        raise ValueError(f"clip_out must be ({b}, 2, {2 + 3 * p}) contiguous fp64 on pred's device")
    if path_out is not None and (path_out.dtype != torch.int32 or tuple(path_out.shape) != (b, 2, p + q - 1, 2)
                                 or not path_out.is_contiguous() or path_out.device != pred.device):
        raise ValueError(f"path_out must be ({b}, 2, {p + q - 1}, 2) contiguous int32 on pred's device")
    if pred.device.type != "cuda" or not (pred.device == gt.device == group.device == acc.device):
        raise ValueError("pred, gt, group and acc must be on one GPU: there is no CPU fallback")
    if not (pred.is_contiguous() and gt.is_contiguous() and group.is_contiguous()):
        raise ValueError("pred, gt and group must be contiguous")
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
    if isinstance(group, torch.Tensor) and group.numel() > 0 and group.dtype == torch.int32:
        lo, hi = (int(v) for v in torch.stack([group.min(), group.max()]).cpu())
        if lo < 0 or hi >= n_groups:
            raise ValueError(f"group ids must lie in [0, {n_groups}), got [{lo}, {hi}]")
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
    i_len, p_len = int(input_len), int(pred_len)
    seq_len = int(store.feats.shape[1])
    if len(groups) != len(store):
        raise ValueError(f"groups has {len(groups)} ids for {len(store)} items")
    if n_groups < 1:
        raise ValueError("no groups")
    ids = np.asarray(groups, dtype=np.int64)
    if ids.size and (ids.min() < 0 or ids.max() >= n_groups):
        raise ValueError(f"group ids must lie in [0, {n_groups})")
    if not 1 <= p_len <= MAX_LEN or i_len < 1 or i_len + p_len > seq_len:
        raise ValueError(f"need 1 <= pred_len <= {MAX_LEN}, 1 <= input_len and input_len + pred_len <= seq_len {seq_len} "
                         f"(got {i_len}, {p_len})")
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    dev = head._device
    with torch.cuda.device(dev):
        gdev = torch.tensor(ids, dtype=torch.int32, device=dev)
        acc = torch.zeros(acc_size(n_groups, p_len), dtype=torch.float64, device=dev)
        acc_plain = torch.zeros(2 * n_groups * p_len + n_groups, dtype=torch.float64, device=dev)
        for s in range(0, len(store), batch_size):
            e = min(s + batch_size, len(store))
            batch = store.get_batch(list(range(s, e)))
            gt = batch[1].to(device=dev, dtype=torch.float32).contiguous()
            pred = head.rollout(batch[0], i_len, p_len)[1]
            _launch(pred, gt, i_len, p_len, gdev[s:e], n_groups, acc, int(band), ROOT_JOINT, None, None)
            protocols._launch(pred, gt, i_len, gdev[s:e], n_groups, acc_plain, ROOT_JOINT)
        sums = torch.cat([acc, acc_plain]).cpu().numpy()
    d, da, f, fa, lag, la, clips = _values(sums[:acc.numel()], n_groups, p_len)
    plain_all = protocols._values(sums[acc.numel():], n_groups, p_len)[1]
    has = clips > 0
    return {"group_names": list(group_names), "clips": clips.round().astype(np.int64), "band": int(band), "dtw": d, "dtw_all": da,
            "dtw_mean": d[has].mean(axis=0), "dtw_future": f, "dtw_future_all": fa, "lag": lag, "lag_all": la,
            "plain_future_all": plain_all, "plain_all": plain_all.mean(axis=0)}
