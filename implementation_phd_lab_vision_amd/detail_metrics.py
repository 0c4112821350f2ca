"""Per-joint errors, PCK / AUC and velocity / acceleration errors of the lifting head, per action and per horizon (INTEGRATION.md
section O).  The companion of ``protocols.py``: the same pass structure, one ``r50_op_pose_detail_metrics`` launch per batch and scored
span into an fp64 device accumulator that is read once per pass.  No CPU fallback.

Per clip, scored frame k and joint j, X the ground truth, Y the prediction, r the root (the pelvis), ``~`` root-relative
(``~Y_j = Y_j - Y_r``), read as fp32 and computed in fp64:

* ``d1 = |~Y_j - ~X_j|``, the per-joint term of P1, and ``d2 = |a R (Y_j - muY) + muX - X_j|`` after the proper similarity fit of
  ``protocols.py``, the per-joint term of P2.  Their means over joints are P1 / P2, so ``p1p2`` needs no second pass.
* **PCK** (MPI-INF-3DHP): the share of joints with ``d < thr_max`` (150 mm).  **AUC**: the mean of that share over the ``n_thr`` (31)
  thresholds ``tau_i = thr_max * i / (n_thr - 1)``; ``tau_0 = 0`` is never hit (the comparison is strict).  Both for d1 and for d2.
* **Velocity error** (MPJVE) ``|(~Y[k] - ~Y[k-1]) - (~X[k] - ~X[k-1])|``, k >= 1, in **metres per frame**, and **acceleration error**
  (the HMMR / PHD line of work) ``|(~Y[k-1] - 2 ~Y[k] + ~Y[k+1]) - (the same of ~X)|``, 1 <= k <= P-2, in **metres per frame^2**, each
  a mean over joints.  No frame rate is assumed.  Differences are taken inside the scored span only: a rollout's first predicted
  frame has no predicted predecessor and so no velocity error.

Groups, ``all`` and the action mean are those of ``protocols.py``.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _lib, clip_pass, protocols
from .protocols import ROOT_JOINT

MAX_THRESHOLDS = 1024                         # r50_op_pose_detail_metrics' limit on n_thr
N_THR = 31                                    # MPI-INF-3DHP: AUC over 0 .. 150 mm in 31 steps
THR_MAX = 0.150                               # metres

# Human3.6M's 17 joints in the dataset's order (frames.H36M_FLIP_PAIRS pairs 1-3 with 4-6 and 11-13 with 14-16).  Labels only.
H36M_JOINT_NAMES = ["pelvis", "r_hip", "r_knee", "r_ankle", "l_hip", "l_knee", "l_ankle", "spine", "thorax", "neck", "head",
                    "l_shoulder", "l_elbow", "l_wrist", "r_shoulder", "r_elbow", "r_wrist"]

METRICS = ("per_joint", "p1p2", "pck", "auc", "vel", "acc")


def joint_names(joints: int) -> List[str]:
    """The H3.6M labels for 17 joints, the indices otherwise."""
    return list(H36M_JOINT_NAMES) if joints == len(H36M_JOINT_NAMES) else [str(j) for j in range(joints)]


def acc_size(n_groups: int, p: int, joints: int) -> int:
    """Doubles in one accumulator: per-joint sums 2*G*P*J, then 6 per (group, frame), then the G clip counts."""
    return 2 * n_groups * p * joints + 6 * n_groups * p + n_groups


def _launch(pred: torch.Tensor, gt: torch.Tensor, i0: int, group: torch.Tensor, n_groups: int, acc: torch.Tensor, root: int, n_thr: int,
            thr_max: float) -> None:
    """Shape, dtype and device checks (those of ``protocols._launch``), then one launch; the group VALUES are the caller's to check."""
    b, p, t, j = protocols.check_poses(pred, gt, root)
    if b < 1 or p < 1 or i0 < 0 or i0 + p > t:
        raise ValueError(f"need B, P >= 1 and 0 <= i0, i0 + P <= T (got B={b}, P={p}, i0={i0}, T={t})")
    if not 2 <= n_thr <= MAX_THRESHOLDS or not (np.isfinite(thr_max) and thr_max > 0):
        raise ValueError(f"need 2 <= n_thr <= {MAX_THRESHOLDS} and a finite thr_max > 0 (got {n_thr}, {thr_max})")
    protocols.check_group_acc(b, group, n_groups, acc, acc_size(n_groups, p, j))
    protocols.check_one_gpu(pred, gt, group, acc)
    rc = _lib.load_library().r50_op_pose_detail_metrics(pred.data_ptr(), gt.data_ptr(), group.data_ptr(), b, p, t, int(i0), j, int(root),
                                                        int(n_groups), int(n_thr), float(thr_max), acc.data_ptr(),
                                                        torch.cuda.current_stream(pred.device).cuda_stream)
    _lib.check(rc, None, "r50_op_pose_detail_metrics")


def add_detail_sums(pred: torch.Tensor, gt: torch.Tensor, i0: int, group: torch.Tensor, n_groups: int, acc: torch.Tensor,
                    root: int = ROOT_JOINT, n_thr: int = N_THR, thr_max: float = THR_MAX) -> None:
    """acc (``acc_size(G, P, J)``) fp64 on the device += the sums of one batch: pred (B, P, J, 3) fp32 scores frames i0 .. i0+P-1 of gt
    (B, T, J, 3) fp32; group (B,) int32 on the device, each value in [0, n_groups) (checked on the host before the launch: one read).
    Layout, with A = 2*G*P*J: ``acc[((g*P + k)*J + j)*2 + {0,1}]`` += the d1, d2 sums; ``acc[A + (g*P + k)*6 + {0,1,2,3}]`` += the hits
    of d1 over all thresholds, of d1 at thr_max, the same two of d2; ``acc[A + (g*P + k)*6 + {4,5}]`` += the velocity and acceleration
    error sums over joints where defined; ``acc[A + 6*G*P + g]`` += the clips of g."""
    protocols.check_group_values(group, n_groups)
    _launch(pred, gt, int(i0), group, int(n_groups), acc, int(root), int(n_thr), float(thr_max))


def values(sums: np.ndarray, n_groups: int, p: int, joints: int, n_thr: int) -> Dict[str, np.ndarray]:
    """One accumulator as arrays (metres, fp64): ``per_joint`` (G, P, J, 2) = [d1, d2] means over the group's clips, ``p1p2`` (G, P, 2)
    = its mean over joints, ``pck`` (G, P, 2) = hits at thr_max / (clips J), ``auc`` (G, P, 2) = hits over all thresholds /
    (n_thr clips J), ``vel`` (G, P) with NaN at k = 0, ``acc`` (G, P) with NaN at k = 0 and k = P-1; each with its ``_all`` form (no
    G axis): the sums over groups over the total clips; ``clips`` (G,).  A group without clips is NaN everywhere."""
    sums = np.asarray(sums, dtype=np.float64)
    a_end = 2 * n_groups * p * joints
    sec_a = sums[:a_end].reshape(n_groups, p, joints, 2)
    sec_b = sums[a_end:a_end + 6 * n_groups * p].reshape(n_groups, p, 6)
    clips = sums[a_end + 6 * n_groups * p:a_end + 6 * n_groups * p + n_groups]
    out: Dict[str, np.ndarray] = {"clips": clips}
    for suffix, a, b, n in (("", sec_a, sec_b, np.where(clips > 0, clips, np.nan)[:, None]),
                            ("_all", sec_a.sum(axis=0), sec_b.sum(axis=0), np.full(1, clips.sum() if clips.sum() > 0 else np.nan))):
        per_joint = a / n[..., None, None]
        vel, acc = b[..., 4] / (n * joints), b[..., 5] / (n * joints)
        vel[..., :1] = np.nan
        acc[..., :1] = np.nan
        acc[..., p - 1:] = np.nan
        out.update({"per_joint" + suffix: per_joint, "p1p2" + suffix: per_joint.mean(axis=-2),
                    "pck" + suffix: b[..., [1, 3]] / (n[..., None] * joints), "auc" + suffix: b[..., [0, 2]] / (n[..., None] * (joints * n_thr)),
                    "vel" + suffix: vel, "acc" + suffix: acc})
    return out


def _nanmean(a: np.ndarray, axis: int) -> np.ndarray:
    """The mean over the defined (non-NaN) entries; NaN where there is none."""
    n = (~np.isnan(a)).sum(axis=axis)
    return np.where(n > 0, np.nansum(a, axis=axis) / np.maximum(n, 1), np.nan)


@torch.no_grad()
def evaluate_detail(head, store, groups: Sequence[int], group_names: Sequence[str], input_len: int = 0, pred_len: int = 0,
                    batch_size: int = 256, n_thr: int = N_THR, thr_max: float = THR_MAX) -> Dict[str, object]:
    """The detail metrics of ``head`` over every item of ``store`` once: the pass of ``protocols.evaluate_protocols`` (store order,
    ``batch_size`` clips per batch, the last kept even if short; ``groups[i]`` in ``[0, len(group_names))``).

    Reconstruction scores all T frames of ``head.joints(feats)``; with ``pred_len > 0`` the P poses of
    ``head.rollout(feats, input_len, pred_len)[1]`` are scored against frames I .. I+P-1.  Returns (metres, metres per frame, metres
    per frame^2, shares in [0, 1]; fp64), with M one of ``per_joint`` (J, 2), ``p1p2`` (2,), ``pck`` (2,), ``auc`` (2,), ``vel`` (),
    ``acc`` () and [.., 2] = [root-relative, after the similarity fit]::

        group_names [G], joint_names [J], clips (G,) int64, n_thr, thr_max
        recon_M (G, ...) the mean over the T frames (over the frames where it is defined for vel / acc), recon_M_all (...),
        recon_M_mean (...) = the plain mean over the non-empty groups
        future_M (G, P, ...), future_M_all (P, ...), future_M_mean (P, ...)          -- only with pred_len > 0

    A group without clips gets NaN and stays out of the means.  ``head``'s mode and weights are not touched.  One launch per batch
    and span, the sums read back once per pass."""
    n_groups = len(group_names)
    ids, i_len, p_len, seq_len = clip_pass.check(store, input_len, pred_len, batch_size, groups, n_groups, forecast_required=False)
    joints = int(head.joints_num)
    dev = head._device
    with torch.cuda.device(dev):
        acc_r = torch.zeros(acc_size(n_groups, seq_len, joints), dtype=torch.float64, device=dev)
        acc_f = torch.zeros(acc_size(n_groups, p_len, joints) if p_len else 0, dtype=torch.float64, device=dev)
        for feats, gt, group in clip_pass.batches(head, store, batch_size, ids):
            _launch(head.joints(feats), gt, 0, group, n_groups, acc_r, ROOT_JOINT, n_thr, thr_max)
            if p_len:
                _launch(head.rollout(feats, i_len, p_len)[1], gt, i_len, group, n_groups, acc_f, ROOT_JOINT, n_thr, thr_max)
        sums = torch.cat([acc_r, acc_f]).cpu().numpy()
    rec = values(sums[:acc_r.numel()], n_groups, seq_len, joints, n_thr)
    has = rec["clips"] > 0
    out: Dict[str, object] = {"group_names": list(group_names), "joint_names": joint_names(joints), "n_thr": int(n_thr),
                              "thr_max": float(thr_max), "clips": rec["clips"].round().astype(np.int64)}
    for m in METRICS:
        over = _nanmean if m in ("vel", "acc") else np.mean
        out[f"recon_{m}"] = over(rec[m], axis=1)
        out[f"recon_{m}_all"] = over(rec[m + "_all"], axis=0)
        out[f"recon_{m}_mean"] = out[f"recon_{m}"][has].mean(axis=0)
    if p_len:
        fut = values(sums[acc_r.numel():], n_groups, p_len, joints, n_thr)
        for m in METRICS:
            out[f"future_{m}"] = fut[m]
            out[f"future_{m}_all"] = fut[m + "_all"]
            out[f"future_{m}_mean"] = fut[m][has].mean(axis=0)
    return out


def _pair(v, scale: float) -> str:
    """``raw / pa`` of a [root-relative, after the similarity fit] pair."""
    return f"{v[0] * scale:.2f} / pa {v[1] * scale:.2f}"


def detail_lines(res: Dict[str, object], input_len: int, pred_len: int) -> List[str]:
    """The printed lines of ``--detail-metrics`` from an ``evaluate_detail`` result: the ``Detail metrics`` line (all clips and the
    action mean: PCK and AUC in percent, raw and after the similarity fit; velocity and acceleration errors in mm per frame and mm per
    frame^2), one ``Per-joint`` line (P1 / P2 in mm per joint name, all clips), one indented line per action, and with ``pred_len > 0``
    the ``Rollout detail metrics`` line at horizons 1, 5, 10 and P (``-`` where a motion error is not defined)."""
    clips = res["clips"]
    at_mm = f"pck@{res['thr_max'] * 1000.0:g}"

    def summary(which: str, key: str = "") -> str:
        g = lambda m: res[f"{which}_{m}{key}"]                        # noqa: E731
        return (f"{at_mm} (%) {_pair(g('pck'), 100.0)} | auc (%) {_pair(g('auc'), 100.0)} | vel (mm/frame) {g('vel') * 1000.0:.2f} "
                f"| accel (mm/frame^2) {g('acc') * 1000.0:.2f}")

    lines = [f"Detail metrics | clips {int(clips.sum())} | actions {len(res['group_names'])} | all: {summary('recon', '_all')} "
             f"| action mean: {summary('recon', '_mean')}"]
    pj = res["recon_per_joint_all"]
    lines.append("Per-joint p1 / p2 (mm) | " + " | ".join(f"{name} {pj[j, 0] * 1000.0:.2f} / {pj[j, 1] * 1000.0:.2f}"
                                                           for j, name in enumerate(res["joint_names"])))
    for i, (name, c) in enumerate(zip(res["group_names"], clips)):
        row = {m: res[f"recon_{m}"][i] for m in ("pck", "auc", "vel", "acc")}
        lines.append(f"  {name} | clips {int(c)} | {at_mm} (%) {_pair(row['pck'], 100.0)} | auc (%) {_pair(row['auc'], 100.0)} "
                     f"| vel (mm/frame) {row['vel'] * 1000.0:.2f} | accel (mm/frame^2) {row['acc'] * 1000.0:.2f}")
    if pred_len > 0:
        hs = sorted({h for h in (1, 5, 10, pred_len) if h <= pred_len})
        num = lambda v, scale: "-" if np.isnan(v) else f"{v * scale:.2f}"                  # noqa: E731
        parts = []
        for label, key in ((f"{at_mm} (%)", "pck"), ("auc (%)", "auc")):
            fa = res[f"future_{key}_all"]
            parts.append(f"{label} " + " | ".join(f"@{h}: {_pair(fa[h - 1], 100.0)}" for h in hs))
        for label, key in (("vel (mm/frame)", "vel"), ("accel (mm/frame^2)", "acc")):
            fa = res[f"future_{key}_all"]
            parts.append(f"{label} " + " | ".join(f"@{h}: {num(fa[h - 1], 1000.0)}" for h in hs))
        lines.append(f"Rollout detail metrics | input {input_len} | pred {pred_len} | clips {int(clips.sum())} | " + " | ".join(parts))
    return lines


def detail_npz(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``.npz`` keys of ``--detail-metrics``: ``detail_actions`` (G,) and ``detail_joint_names`` (J,) str, ``detail_clips`` (G,)
    int64, and fp32 ``detail_recon_M`` (G, ...) / ``detail_recon_M_all`` (...) for M in per_joint (J, 2), p1p2 (2,), pck (2,), auc (2,),
    vel (), acc () -- metres, metres per frame, metres per frame^2, shares in [0, 1]; [.., 2] = [root-relative, after the fit]; with a
    rollout ``detail_future_M`` (G, P, ...) and ``detail_future_M_all`` (P, ...)."""
    out = {"detail_actions": np.array([str(n) for n in res["group_names"]], dtype=str),
           "detail_joint_names": np.array([str(n) for n in res["joint_names"]], dtype=str),
           "detail_clips": np.asarray(res["clips"], dtype=np.int64)}
    for which in ("recon", "future"):
        for m in ("per_joint", "p1p2", "pck", "auc", "vel", "acc"):
            for key in (f"{which}_{m}", f"{which}_{m}_all"):
                if key in res:
                    out["detail_" + key] = np.asarray(res[key], dtype=np.float32)
    return out
