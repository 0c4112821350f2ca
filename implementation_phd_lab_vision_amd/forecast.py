"""Forecasting evaluation of the lifting head: observe ``input_len`` frames, roll f_AR forward
``pred_len`` frames (``PHDFor3DJoints.rollout``), and score the decoded future poses per horizon.

The reference sets out the task (src/config.py: ``INPUT_LEN = 15``, ``PRED_LEN = 25``, ``SEQ_LEN = 40``) but never builds it.
This project's metrics, for ``I + P <= T`` with ``pred[b, k]`` predicting frame ``I + k``:

* ``mpjpe[k]`` = mean over all clips and joints of ``|pred[b,k,j] - joints3d[b,I+k,j]|_2``;
* ``l3d[k]``   = the matching mean squared error (over clips, joints and the three coordinates);
* ``mpjpe_mean`` = the mean of ``mpjpe[k]`` over k.

Every clip weighs the same over the whole pass (not a mean of per-batch means), so the numbers do not depend on the batch size
apart from fp32 rounding.  One ``r50_op_horizon_metrics`` launch per batch adds into an fp64 device accumulator that is read once.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch

from . import _lib, clip_pass
from .protocols import check_poses

INPUT_LEN = 15             # src/config.py
PRED_LEN = 25


def metrics_from_sums(acc: Sequence[float], pred_len: int, joints: int) -> Dict[str, object]:
    """The metrics from the accumulator ``r50_op_horizon_metrics`` fills: acc[k] = sum of per-joint distances at horizon k,
    acc[P+k] = sum of squared errors, acc[2P] = clips."""
    p = int(pred_len)
    if len(acc) != 2 * p + 1:
        raise ValueError(f"expected {2 * p + 1} sums, got {len(acc)}")
    clips = int(round(acc[2 * p]))
    if clips < 1:
        raise ValueError("no clips were scored")
    mpjpe: List[float] = [acc[k] / (clips * joints) for k in range(p)]
    l3d: List[float] = [acc[p + k] / (clips * joints * 3) for k in range(p)]
    return {"mpjpe": mpjpe, "l3d": l3d, "mpjpe_mean": sum(mpjpe) / p, "clips": clips}


def add_horizon_metrics(pred: torch.Tensor, gt: torch.Tensor, input_len: int, acc: torch.Tensor) -> None:
    """acc (2P+1) fp64 on the device += the sums of one batch: pred (B, P, J, 3) fp32 predicts frames input_len .. input_len+P-1 of
    gt (B, T, J, 3) fp32."""
    b, p, t, j = check_poses(pred, gt)
    if acc.dtype != torch.float64 or acc.numel() != 2 * p + 1 or not acc.is_contiguous():
        raise ValueError(f"acc must be {2 * p + 1} contiguous fp64 values")
    if not (pred.is_contiguous() and gt.is_contiguous()) or not (pred.device == gt.device == acc.device):
        raise ValueError("pred, gt and acc must be contiguous and on one device")
    rc = _lib.load_library().r50_op_horizon_metrics(pred.data_ptr(), gt.data_ptr(), b, p, t, int(input_len), j, acc.data_ptr(),
                                                    torch.cuda.current_stream(pred.device).cuda_stream)
    _lib.check(rc, None, "r50_op_horizon_metrics")


@torch.no_grad()
def evaluate_rollout(head, store, input_len: int = INPUT_LEN, pred_len: int = PRED_LEN, batch_size: int = 256) -> Dict[str, object]:
    """Every item of ``store`` (a ``DeviceFeatureStore``) once, in store order, ``batch_size`` clips per rollout, the last batch
    kept even if short.  Returns ``{"mpjpe": [P], "l3d": [P], "mpjpe_mean": float, "clips": int}`` (metres, as the store's joints).
    The default of 256 clips is deliberate: at 32 clips the per-step GEMMs have 480-1248 rows, under a third of the chip's CUs.
    ``head`` is any ``PHDFor3DJoints`` (a training head included); its mode and weights are not touched."""
    _, i_len, p_len, _ = clip_pass.check(store, input_len, pred_len, batch_size)
    dev = head._device
    with torch.cuda.device(dev):
        acc = torch.zeros(2 * p_len + 1, dtype=torch.float64, device=dev)
        for feats, gt, _ in clip_pass.batches(head, store, batch_size):
            add_horizon_metrics(head.rollout(feats, i_len, p_len)[1], gt, i_len, acc)
        sums = acc.tolist()
    return metrics_from_sums(sums, p_len, head.joints_num)
