"""Evaluation of the hallucinator f_hal: what the lifting head gives from ONE frame, beside what it gives
with temporal context, on the same clips.

* **Reconstruction from one frame.**  ``head.hallucinate(feats)[1]`` -- every frame's pose from that frame alone -- beside
  ``head.joints(feats)`` (f_movie over the clip): MPJPE, root-relative MPJPE (P1) and PA-MPJPE (P2) over every frame.
* **Forecast from one frame** (``pred_len > 0``).  The predictor ``hal`` is ``head.hallucinated_rollout(feats, input_len - 1, P)``:
  only the last observed frame is seen, and its P poses are scored against frames I .. I+P-1 -- the frames ``rollout(feats, I, P)``
  (``model``) and the baselines of section U forecast, so the rows compare line by line.

One pass in store order; the sums by ``forecast.add_horizon_metrics`` and ``protocols``' kernel into fp64 device accumulators that are
read once.  No CPU fallback.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import clip_pass, protocols
from .forecast import add_horizon_metrics, metrics_from_sums
from .protocols import ROOT_JOINT

NAMES = ("model", "hal")
NO_HALLUCINATOR = ("this checkpoint has no hallucinator (no f_hal.* keys): train one with "
                   "python -m implementation_phd_lab_vision_amd.train_hal --init CKPT")


def require_hallucinator(state_keys) -> None:
    """``--hallucinate``'s rule, a function of a state dict's keys alone: ``SystemExit`` naming ``train_hal`` when f_hal is missing."""
    from .model import has_hallucinator
    if not has_hallucinator(state_keys):
        raise SystemExit(f"results: --hallucinate: {NO_HALLUCINATOR}")


@torch.no_grad()
def evaluate_hallucinator(head, store, groups: Sequence[int], group_names: Sequence[str], input_len: int, pred_len: int,
                          batch_size: int = 256) -> Dict[str, object]:
    """``hal`` beside ``model`` over every item of ``store`` (a ``DeviceFeatureStore``) once, in store order, ``batch_size`` clips per
    batch (the last kept even if short).  ``groups[i]`` in ``[0, len(group_names))`` is item i's group (``protocols.action_groups``).
    Returns (metres, fp64), in ``baselines.evaluate_baselines``' layout::

        names = ("model", "hal");  group_names [G];  clips (G,) int64;  input_len;  pred_len
        recon: {<name>: {"mpjpe" (T,), "p1" (T,), "p2" (T,), "per_action" (G, T, 2)}}      per frame of the clip
        <name>: {"mpjpe" (P,), "p1" (P,), "p2" (P,), "per_action" (G, P, 2)}               per horizon; only with pred_len > 0

    ``recon["model"]`` is ``joints(feats)``, ``recon["hal"]`` is ``hallucinate(feats)[1]``; the forecast's ``model`` rows are
    ``evaluate_baselines``' ``model`` rows exactly (the same launches into the same sums).  The head's mode and weights are not
    touched."""
    n_groups = len(group_names)
    ids, i_len, p_len, seq_len = clip_pass.check(store, input_len, pred_len, batch_size, groups, n_groups, forecast_required=False)
    if not getattr(head, "hallucinator", False):
        raise ValueError(NO_HALLUCINATOR)
    dev = head._device

    def sizes(p: int):
        return 2 * p + 1, 2 * n_groups * p + n_groups

    rh, rp = sizes(seq_len)
    fh, fp = sizes(p_len) if p_len else (0, 0)
    with torch.cuda.device(dev):
        acc = {"rh": torch.zeros((2, rh), dtype=torch.float64, device=dev), "rp": torch.zeros((2, rp), dtype=torch.float64, device=dev),
               "fh": torch.zeros((2, fh), dtype=torch.float64, device=dev), "fp": torch.zeros((2, fp), dtype=torch.float64, device=dev)}
        for feats, gt, group in clip_pass.batches(head, store, batch_size, ids):
            recon = {"model": head.joints(feats), "hal": head.hallucinate(feats)[1]}
            for r, name in enumerate(NAMES):
                add_horizon_metrics(recon[name], gt, 0, acc["rh"][r])
                protocols._launch(recon[name], gt, 0, group, n_groups, acc["rp"][r], ROOT_JOINT)
            if p_len:
                preds = {"model": head.rollout(feats, i_len, p_len)[1], "hal": head.hallucinated_rollout(feats, i_len - 1, p_len)[1]}
                for r, name in enumerate(NAMES):
                    add_horizon_metrics(preds[name], gt, i_len, acc["fh"][r])
                    protocols._launch(preds[name], gt, i_len, group, n_groups, acc["fp"][r], ROOT_JOINT)
        host = {k: v.cpu().numpy() for k, v in acc.items()}

    def rows(hsum: np.ndarray, psum: np.ndarray, p: int) -> Dict[str, np.ndarray]:
        hm = metrics_from_sums(hsum.tolist(), p, head.joints_num)
        per, all_, clips = protocols._values(psum, n_groups, p)
        out["clips"] = clips.round().astype(np.int64)
        return {"mpjpe": np.asarray(hm["mpjpe"], dtype=np.float64), "p1": all_[:, 0].copy(), "p2": all_[:, 1].copy(), "per_action": per}

    out: Dict[str, object] = {"names": NAMES, "group_names": list(group_names), "input_len": i_len, "pred_len": p_len}
    out["recon"] = {name: rows(host["rh"][r], host["rp"][r], seq_len) for r, name in enumerate(NAMES)}
    if p_len:
        for r, name in enumerate(NAMES):
            out[name] = rows(host["fh"][r], host["fp"][r], p_len)
    return out


def _ratio(a: float, b: float) -> str:
    return f"{a / b:.4f}" if b > 0 else "nan"


def hallucinate_lines(res: Dict[str, object]) -> List[str]:
    """The printed lines of ``--hallucinate`` from an ``evaluate_hallucinator`` result, after ``baselines.baseline_lines``: the
    ``Hallucinator`` header; per predictor (``model`` = with temporal context, ``hal`` = from one frame) the reconstruction's MPJPE / P1 /
    P2 in mm, the mean over the clip's frames, ``hal`` with the ratio hal / model on P1; one line per action; and with a forecast the
    same per horizon (1, 5, 10, P and the mean) and per action.  Millimetres."""
    i_len, p_len = int(res["input_len"]), int(res["pred_len"])
    lines = [f"Hallucinator | clips {int(np.sum(res['clips']))} | actions {len(res['group_names'])} | predictors {len(res['names'])}"
             + (f" | input {i_len} (hal sees frame {i_len - 1} only) | pred {p_len}" if p_len else "")]
    rec = res["recon"]
    for name in res["names"]:
        row = rec[name]
        line = f"  recon {name} | " + " | ".join(f"{key} (mm) {np.mean(row[key]) * 1000.0:.2f}" for key in ("mpjpe", "p1", "p2"))
        if name != "model":
            line += f" | hal / model on p1: {_ratio(float(np.mean(row['p1'])), float(np.mean(rec['model']['p1'])))}"
        lines.append(line)
    for g, gname in enumerate(res["group_names"]):
        m, h = (np.nanmean(rec[n]["per_action"][g], axis=0) for n in ("model", "hal"))
        lines.append(f"    recon {gname} | clips {int(res['clips'][g])} | model p1 (mm) {m[0] * 1000.0:.2f} | p2 (mm) {m[1] * 1000.0:.2f} "
                     f"| hal p1 (mm) {h[0] * 1000.0:.2f} | p2 (mm) {h[1] * 1000.0:.2f} | hal / model on p1: {_ratio(h[0], m[0])}")
    if p_len:
        hs = sorted({h for h in (1, 5, 10, p_len) if h <= p_len})
        for name in res["names"]:
            row = res[name]
            parts = [f"{key} (mm) " + " | ".join(f"@{h}: {row[key][h - 1] * 1000.0:.2f}" for h in hs) + f" | mean: {np.mean(row[key]) * 1000.0:.2f}"
                     for key in ("mpjpe", "p1", "p2")]
            line = f"  forecast {name} | " + " | ".join(parts)
            if name != "model":
                line += f" | hal / model on p1: {_ratio(float(np.mean(row['p1'])), float(np.mean(res['model']['p1'])))}"
            lines.append(line)
        for g, gname in enumerate(res["group_names"]):
            m, h = (np.nanmean(res[n]["per_action"][g], axis=0) for n in ("model", "hal"))
            lines.append(f"    forecast {gname} | clips {int(res['clips'][g])} | model p1 (mm) {m[0] * 1000.0:.2f} | hal p1 (mm) "
                         f"{h[0] * 1000.0:.2f} | hal / model on p1: {_ratio(h[0], m[0])}")
    return lines


def hallucinate_arrays(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``.npz`` keys of ``--hallucinate``: ``hal_names`` (2,) str [model, hal]; ``hal_actions`` (G,) str; fp32 ``hal_recon_mpjpe``,
    ``hal_recon_p1``, ``hal_recon_p2`` (2, T) and ``hal_recon_per_action`` (2, G, T, 2) in metres; with a forecast ``hal_mpjpe``,
    ``hal_p1``, ``hal_p2`` (2, P), ``hal_per_action`` (2, G, P, 2) and ``hal_lens`` int64 [the frame hal sees, P]."""
    names = list(res["names"])
    out = {"hal_names": np.array(names, dtype=str), "hal_actions": np.array([str(n) for n in res["group_names"]], dtype=str),
           "hal_recon_per_action": np.stack([np.asarray(res["recon"][n]["per_action"], dtype=np.float32) for n in names])}
    for key in ("mpjpe", "p1", "p2"):
        out["hal_recon_" + key] = np.stack([np.asarray(res["recon"][n][key], dtype=np.float32) for n in names])
    if int(res["pred_len"]) > 0:
        out["hal_per_action"] = np.stack([np.asarray(res[n]["per_action"], dtype=np.float32) for n in names])
        for key in ("mpjpe", "p1", "p2"):
            out["hal_" + key] = np.stack([np.asarray(res[n][key], dtype=np.float32) for n in names])
        out["hal_lens"] = np.array([int(res["input_len"]) - 1, int(res["pred_len"])], dtype=np.int64)
    return out
