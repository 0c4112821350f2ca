"""The two H3.6M evaluation protocols of the lifting head, per action and per horizon.

Published Human3.6M results are quoted under two protocols, usually per action.  Per pose, X the ground truth and Y the prediction
(J x 3, read as fp32, computed in fp64):

* **P1**, root-relative MPJPE: ``(1/J) sum_j |(Y_j - Y_r) - (X_j - X_r)|`` with the pelvis ``r = 0`` as the root.  All J joints are
  in the mean, so the root adds 0.
* **P2**, PA-MPJPE: the same distance after the least-squares proper similarity fit of Y onto X (Umeyama 1991: centroids, the SVD
  of ``M = sum_j X0_j Y0_j^T``, no reflections, scale ``a = tr(D S) / sum_j |Y0_j|^2``; ``a = 0`` when either pose has no spread).

A group (one action) holds clips; each clip adds one pose per scored frame.  A group's value at a frame or horizon is the sum of its
per-pose errors over its clip count; ``all`` is the same over every clip; the action mean is the plain mean of the per-action values
(the H3.6M table convention).  Action names are ``meta["action"]`` / the index entry's ``action`` without a trailing ``_<digits>`` or
`` <digits>`` trial suffix.

One ``r50_op_pose_protocols`` launch per batch and scored span adds into an fp64 device accumulator that is read once per pass; the
kernel solves each pose's fit in Horn's quaternion form with a bounded fp64 Jacobi (``csrc/kernels.h``).  No CPU fallback.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, clip_pass

ROOT_JOINT = 0                                # the pelvis (src/dataset.py: joint 0 is the root)
MAX_JOINTS = 64                               # r50_op_pose_protocols' limit

_TRIAL_SUFFIX = re.compile(r"[_ ]\d+$")


def action_name(name) -> str:
    """``Directions_1`` and ``Directions 1`` -> ``Directions``; a name without a trial suffix (``act0``) is kept."""
    return _TRIAL_SUFFIX.sub("", str(name))


def action_groups(names: Sequence) -> Tuple[List[str], List[int]]:
    """(group_names sorted, ids): ids[i] is the index in group_names of ``action_name(names[i])``."""
    actions = [action_name(n) for n in names]
    group_names = sorted(set(actions))
    pos = {a: g for g, a in enumerate(group_names)}
    return group_names, [pos[a] for a in actions]


def check_poses(pred: torch.Tensor, gt: torch.Tensor, root: Optional[int] = None) -> Tuple[int, int, int, int]:
    """The first checks of every op that scores pred (B, P, J, 3) against gt (B, T, J, 3): rank, shapes and fp32 and, with ``root``, the
    grouped pose ops' ``J <= MAX_JOINTS`` and ``0 <= root < J``.  Returns (B, P, T, J)."""
    if pred.dim() != 4 or gt.dim() != 4:
        raise ValueError(f"pred (B,P,J,3) and gt (B,T,J,3) expected, got {tuple(pred.shape)}, {tuple(gt.shape)}")
    b, p, j, _ = pred.shape
    t = gt.shape[1]
    if tuple(gt.shape) != (b, t, j, 3) or pred.shape[3] != 3 or pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError(f"pred (B,P,J,3) and gt (B,T,J,3) fp32 expected, got {tuple(pred.shape)} {pred.dtype}, {tuple(gt.shape)} {gt.dtype}")
    if root is not None and (not 1 <= j <= MAX_JOINTS or not 0 <= root < j):
        raise ValueError(f"need 1 <= J <= {MAX_JOINTS} and 0 <= root < J (got J={j}, root={root})")
    return b, p, t, j


def check_group_acc(b: int, group: torch.Tensor, n_groups: int, acc: torch.Tensor, n_acc: int) -> None:
    """The grouped pose ops' checks after their own limits: ``n_groups``, group (B,) int32 and acc ``n_acc`` contiguous fp64."""
    if n_groups < 1:
        raise ValueError("n_groups must be >= 1")
    if group.dtype != torch.int32 or tuple(group.shape) != (b,):
        raise ValueError(f"group must be ({b},) int32, got {tuple(group.shape)} {group.dtype}")
    if acc.dtype != torch.float64 or acc.numel() != n_acc or not acc.is_contiguous():
        raise ValueError(f"acc must be {n_acc} contiguous fp64 values")


def check_one_gpu(pred: torch.Tensor, gt: torch.Tensor, group: torch.Tensor, acc: torch.Tensor) -> None:
    """The grouped pose ops' last checks, after their own output buffers: one GPU, then contiguity."""
    if pred.device.type != "cuda" or not (pred.device == gt.device == group.device == acc.device):
        raise ValueError("pred, gt, group and acc must be on one GPU: there is no CPU fallback")
    if not (pred.is_contiguous() and gt.is_contiguous() and group.is_contiguous()):
        raise ValueError("pred, gt and group must be contiguous")


def check_group_values(group, n_groups: int) -> None:
    """The host-side check of the ``add_*_sums`` wrappers: every value of an int32 ``group`` lies in [0, n_groups) (one read)."""
    if isinstance(group, torch.Tensor) and group.numel() > 0 and group.dtype == torch.int32:
        lo, hi = (int(v) for v in torch.stack([group.min(), group.max()]).cpu())
        if lo < 0 or hi >= n_groups:
            raise ValueError(f"group ids must lie in [0, {n_groups}), got [{lo}, {hi}]")


def _launch(pred: torch.Tensor, gt: torch.Tensor, i0: int, group: torch.Tensor, n_groups: int, acc: torch.Tensor, root: int) -> None:
    """Shape, dtype and device checks, then one launch; the group VALUES are the caller's to have checked."""
    b, p, t, j = check_poses(pred, gt, root)
    if b < 1 or p < 1 or i0 < 0 or i0 + p > t:
        raise ValueError(f"need B, P >= 1 and 0 <= i0, i0 + P <= T (got B={b}, P={p}, i0={i0}, T={t})")
    check_group_acc(b, group, n_groups, acc, 2 * n_groups * p + n_groups)
    check_one_gpu(pred, gt, group, acc)
    rc = _lib.load_library().r50_op_pose_protocols(pred.data_ptr(), gt.data_ptr(), group.data_ptr(), b, p, t, int(i0), j, int(root),
                                                   int(n_groups), acc.data_ptr(), torch.cuda.current_stream(pred.device).cuda_stream)
    _lib.check(rc, None, "r50_op_pose_protocols")


def add_protocol_sums(pred: torch.Tensor, gt: torch.Tensor, i0: int, group: torch.Tensor, n_groups: int, acc: torch.Tensor,
                      root: int = ROOT_JOINT) -> None:
    """acc (2*G*P + G) fp64 on the device += the sums of one batch: pred (B, P, J, 3) fp32 scores frames i0 .. i0+P-1 of gt
    (B, T, J, 3) fp32; group (B,) int32 on the device, each value in [0, n_groups) (checked on the host before the launch: one
    read).  ``acc[(g*P + k)*2 + 0]`` += the P1 sum, ``acc[(g*P + k)*2 + 1]`` += the P2 sum, ``acc[2*G*P + g]`` += the clips of g."""
    check_group_values(group, n_groups)
    _launch(pred, gt, int(i0), group, int(n_groups), acc, int(root))


def _values(sums: np.ndarray, n_groups: int, p: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(per-group (G, P, 2), all (P, 2), clips (G,)) from one accumulator; a group without clips gets NaN."""
    s = sums[:2 * n_groups * p].reshape(n_groups, p, 2)
    clips = sums[2 * n_groups * p:]
    per_group = np.full_like(s, np.nan)
    has = clips > 0
    per_group[has] = s[has] / clips[has, None, None]
    return per_group, s.sum(axis=0) / clips.sum(), clips


@torch.no_grad()
def evaluate_protocols(head, store, groups: Sequence[int], group_names: Sequence[str], input_len: int = 0, pred_len: int = 0,
                       batch_size: int = 256) -> Dict[str, object]:
    """P1 / P2 of ``head`` over every item of ``store`` (a ``DeviceFeatureStore``) once, in store order, ``batch_size`` clips per
    batch (the last kept even if short).  ``groups[i]`` in ``[0, len(group_names))`` is item i's group (``action_groups``).

    Reconstruction scores all T frames of ``head.joints(feats)``; with ``pred_len > 0`` the P poses of
    ``head.rollout(feats, input_len, pred_len)[1]`` are scored against frames I .. I+P-1 per horizon.  Returns (metres, fp64)::

        group_names [G], clips (G,) int64
        recon (G, 2) = [p1, p2] per group, the mean over the T frames;  recon_all (2,);  recon_mean (2,) = the plain mean over groups
        future (G, P, 2), future_all (P, 2), future_mean (P, 2)      -- only with pred_len > 0

    A group without clips gets NaN and stays out of the means.  ``head`` is any ``PHDFor3DJoints``; its mode and weights are not
    touched.  The sums are read back once per pass."""
    n_groups = len(group_names)
    ids, i_len, p_len, seq_len = clip_pass.check(store, input_len, pred_len, batch_size, groups, n_groups, forecast_required=False)
    dev = head._device
    with torch.cuda.device(dev):
        acc_r = torch.zeros(2 * n_groups * seq_len + n_groups, dtype=torch.float64, device=dev)
        acc_f = torch.zeros(2 * n_groups * p_len + n_groups if p_len else 0, dtype=torch.float64, device=dev)
        for feats, gt, group in clip_pass.batches(head, store, batch_size, ids):
            _launch(head.joints(feats), gt, 0, group, n_groups, acc_r, ROOT_JOINT)
            if p_len:
                _launch(head.rollout(feats, i_len, p_len)[1], gt, i_len, group, n_groups, acc_f, ROOT_JOINT)
        sums = torch.cat([acc_r, acc_f]).cpu().numpy()
    rec, rec_all, clips = _values(sums[:acc_r.numel()], n_groups, seq_len)
    has = clips > 0
    out: Dict[str, object] = {"group_names": list(group_names), "clips": clips.round().astype(np.int64),
                              "recon": rec.mean(axis=1), "recon_all": rec_all.mean(axis=0)}
    out["recon_mean"] = out["recon"][has].mean(axis=0)
    if p_len:
        fut, fut_all, _ = _values(sums[acc_r.numel():], n_groups, p_len)
        out.update(future=fut, future_all=fut_all, future_mean=fut[has].mean(axis=0))
    return out


def protocol_lines(res: Dict[str, object], input_len: int, pred_len: int) -> List[str]:
    """The printed lines of ``--protocols`` from an ``evaluate_protocols`` result: the ``Protocol metrics`` line (all clips and the
    action mean), one indented line per action, and with ``pred_len > 0`` the ``Rollout protocol metrics`` line (all clips, horizons
    1, 5, 10 and P as the ``Rollout metrics`` line).  Millimetres."""
    clips = res["clips"]
    ra, rm = res["recon_all"], res["recon_mean"]
    lines = [f"Protocol metrics | clips {int(clips.sum())} | actions {len(res['group_names'])} | all: p1 (mm) {ra[0] * 1000.0:.2f} "
             f"| p2 (mm) {ra[1] * 1000.0:.2f} | action mean: p1 (mm) {rm[0] * 1000.0:.2f} | p2 (mm) {rm[1] * 1000.0:.2f}"]
    for name, c, (p1, p2) in zip(res["group_names"], clips, res["recon"]):
        lines.append(f"  {name} | clips {int(c)} | p1 (mm) {p1 * 1000.0:.2f} | p2 (mm) {p2 * 1000.0:.2f}")
    if pred_len > 0:
        fa = res["future_all"]
        hs = sorted({h for h in (1, 5, 10, pred_len) if h <= pred_len})
        at = [" | ".join(f"@{h}: {fa[h - 1, m] * 1000.0:.2f}" for h in hs) for m in (0, 1)]
        lines.append(f"Rollout protocol metrics | input {input_len} | pred {pred_len} | clips {int(clips.sum())} | p1 (mm) {at[0]} "
                     f"| p2 (mm) {at[1]}")
    return lines


def protocol_arrays(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``.npz`` keys of ``--protocols``: ``protocol_actions`` (G,) str, ``protocol_clips`` (G,) int64, ``protocol_recon`` (G, 2)
    and ``protocol_recon_all`` (2,) fp32 [p1, p2] in metres; with a rollout ``protocol_future`` (G, P, 2), ``protocol_future_all``
    (P, 2)."""
    out = {"protocol_actions": np.array([str(n) for n in res["group_names"]], dtype=str),
           "protocol_clips": np.asarray(res["clips"], dtype=np.int64),
           "protocol_recon": np.asarray(res["recon"], dtype=np.float32),
           "protocol_recon_all": np.asarray(res["recon_all"], dtype=np.float32)}
    if "future" in res:
        out["protocol_future"] = np.asarray(res["future"], dtype=np.float32)
        out["protocol_future_all"] = np.asarray(res["future_all"], dtype=np.float32)
    return out
