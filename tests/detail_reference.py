"""numpy fp64 oracle of the detail metrics and the seeded inputs its CPU and GPU tests share.  Not a test.

Per clip, scored frame k and joint j, X the ground truth, Y the prediction, r the root, ``~`` root-relative (``~Y_j = Y_j - Y_r``), all
read as fp32 and computed in fp64:

* ``d1 = |~Y_j - ~X_j|`` (P1's per-joint term), ``d2 = |a R (Y_j - muY) + muX - X_j|`` with ``(a, R, muY, muX)`` from
  ``protocols_reference.similarity_fit`` (P2's per-joint term; an SVD where the kernel runs Horn's quaternion form);
* thresholds ``tau_i = thr_max * i / (n_thr - 1)``, a hit when ``d < tau`` (strict); PCK counts the hits at ``thr_max`` itself;
* ``ev = |(~Y[k] - ~Y[k-1]) - (~X[k] - ~X[k-1])|`` for k >= 1, ``ea = |(~Y[k-1] - 2 ~Y[k] + ~Y[k+1]) - (the same of ~X)|`` for
  1 <= k <= P-2, differences inside ``pred`` only; metres per frame and per frame^2.

``detail_sums`` returns the accumulator ``r50_op_pose_detail_metrics`` adds, in the same layout."""
import functools
from typing import Dict, Tuple

import numpy as np

from tests import protocols_reference as pr

THR_MAX = 0.150

# (b, p, t_gt, i0, J, G, root, n_thr): the smallest shapes at which the kernel can go wrong
CASES = [(5, 3, 7, 2, 17, 4, 0, 31),          # one acceleration frame, empty groups
         (300, 2, 4, 1, 3, 3, 2, 31),         # b > 256 (two passes), velocity only, root != 0
         (7, 4, 4, 0, 1, 2, 0, 2),            # J = 1: every distance exactly 0; the minimal n_thr
         (33, 5, 9, 4, 64, 6, 63, 31),        # J at the limit, root last, i0 + p = t_gt
         (2, 1, 1, 0, 17, 1, 0, 31),          # p = 1: no motion terms at all
         (40, 40, 40, 0, 17, 15, 0, 31),      # the evaluation's own shape
         (9, 3, 3, 0, 17, 2, 0, 7)]


def acc_size(n_groups: int, p: int, joints: int) -> int:
    return 2 * n_groups * p * joints + 6 * n_groups * p + n_groups


def thresholds(n_thr: int, thr_max: float) -> np.ndarray:
    return np.float64(thr_max) * np.arange(n_thr, dtype=np.float64) / np.float64(n_thr - 1)


def distances(pred, gt, i0: int, root: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(d1, d2, ev, ea), each (B, P, J) fp64; ev / ea are NaN at the frames where they are not defined."""
    y, x = pr._f64(pred), pr._f64(gt)
    b, p, j = y.shape[:3]
    x = x[:, i0:i0 + p]
    ry, rx = y - y[:, :, root:root + 1], x - x[:, :, root:root + 1]
    d1 = np.linalg.norm(ry - rx, axis=-1)
    d2 = np.empty((b, p, j))
    for i in range(b):
        for k in range(p):
            a, r, mu_y, mu_x = pr.similarity_fit(y[i, k], x[i, k])
            d2[i, k] = np.linalg.norm(a * (y[i, k] - mu_y) @ r.T + mu_x - x[i, k], axis=-1)
    ev, ea = np.full((b, p, j), np.nan), np.full((b, p, j), np.nan)
    if p >= 2:
        ev[:, 1:] = np.linalg.norm((ry[:, 1:] - ry[:, :-1]) - (rx[:, 1:] - rx[:, :-1]), axis=-1)
    if p >= 3:
        ea[:, 1:-1] = np.linalg.norm((ry[:, :-2] - 2.0 * ry[:, 1:-1] + ry[:, 2:]) - (rx[:, :-2] - 2.0 * rx[:, 1:-1] + rx[:, 2:]), axis=-1)
    return d1, d2, ev, ea


def smallest_threshold_gap(d1: np.ndarray, d2: np.ndarray, n_thr: int, thr_max: float) -> float:
    """min |d - tau_i| over every d1, d2 and every POSITIVE threshold (and thr_max itself): the tie-free condition's figure."""
    tau = np.append(thresholds(n_thr, thr_max)[1:], thr_max)
    d = np.concatenate([d1.ravel(), d2.ravel()])
    return float(np.abs(d[:, None] - tau[None, :]).min())


def detail_sums(pred, gt, i0: int, group, n_groups: int, root: int = 0, n_thr: int = 31, thr_max: float = THR_MAX,
                dists=None) -> np.ndarray:
    """pred (B, P, J, 3) scores frames i0 .. i0+P-1 of gt (B, T, J, 3); group (B,) in [0, n_groups).  The fp64 accumulator of
    ``r50_op_pose_detail_metrics``: A ``[((g*P + k)*J + j)*2 + {0,1}]`` = sums of d1, d2; B ``[A + (g*P + k)*6 + {0..5}]`` = hits of d1
    over all thresholds, at thr_max, the same for d2, sums of ev, ea; C ``[A + 6*G*P + g]`` = clips.  ``dists``: the result of
    ``distances`` on the same inputs, when the caller has it already."""
    d1, d2, ev, ea = distances(pred, gt, i0, root) if dists is None else dists
    group = np.asarray(group.cpu() if hasattr(group, "cpu") else group).astype(np.int64)
    b, p, j = d1.shape
    tau = thresholds(n_thr, thr_max)
    a_end = 2 * n_groups * p * j
    acc = np.zeros(acc_size(n_groups, p, j), dtype=np.float64)
    sec_a = acc[:a_end].reshape(n_groups, p, j, 2)
    sec_b = acc[a_end:a_end + 6 * n_groups * p].reshape(n_groups, p, 6)
    for i in range(b):
        g = int(group[i])
        acc[a_end + 6 * n_groups * p + g] += 1.0
        sec_a[g, :, :, 0] += d1[i]
        sec_a[g, :, :, 1] += d2[i]
        for m, d in ((0, d1[i]), (2, d2[i])):
            sec_b[g, :, m] += (d[:, :, None] < tau[None, None, :]).sum(axis=(1, 2))
            sec_b[g, :, m + 1] += (d < np.float64(thr_max)).sum(axis=1)
        sec_b[g, 1:, 4] += ev[i, 1:].sum(axis=1)
        sec_b[g, 1:p - 1, 5] += ea[i, 1:p - 1].sum(axis=1)
    return acc


def values_from_sums(acc: np.ndarray, n_groups: int, p: int, joints: int, n_thr: int) -> Dict[str, np.ndarray]:
    """The arrays of ``detail_metrics.values``, restated: per group a sum over its clip count (NaN without clips), ``_all`` the
    section sums over groups over the total clips; vel / acc NaN where undefined."""
    acc = np.asarray(acc, dtype=np.float64)
    a_end = 2 * n_groups * p * joints
    sec_a = acc[:a_end].reshape(n_groups, p, joints, 2)
    sec_b = acc[a_end:a_end + 6 * n_groups * p].reshape(n_groups, p, 6)
    clips = acc[a_end + 6 * n_groups * p:]
    total = clips.sum()

    def arrays(a, b, n):
        with np.errstate(invalid="ignore", divide="ignore"):
            out = {"per_joint": a / n[..., None, None, None], "pck": b[..., [1, 3]] / (n[..., None, None] * joints),
                   "auc": b[..., [0, 2]] / (n[..., None, None] * joints * n_thr), "vel": b[..., 4] / (n[..., None] * joints),
                   "acc": b[..., 5] / (n[..., None] * joints)}
        out["p1p2"] = out["per_joint"].mean(axis=-2)
        out["vel"][..., :1] = np.nan
        out["acc"][..., :1] = np.nan
        out["acc"][..., p - 1:] = np.nan
        return out

    out = arrays(sec_a, sec_b, clips)
    out.update({k + "_all": v for k, v in arrays(sec_a.sum(axis=0), sec_b.sum(axis=0), np.float64(total)).items()})
    out["clips"] = clips
    return out


# ---- seeded inputs (the generators of tests/test_protocols_gpu.py, restated) ------------------------------------------------------
def clips(rng, b, t, j):
    """(B, T, J, 3) fp32 ground truth: a person 4.5 m from the camera, joints spread ~0.3 m, moving ~0.02 m per frame."""
    centre = rng.standard_normal((b, 1, 1, 3)) * np.array([1.0, 0.5, 0.5]) + np.array([0.0, 0.0, 4.5])
    body = rng.standard_normal((b, 1, j, 3)) * 0.3
    return (centre + body + rng.standard_normal((b, t, j, 3)) * 0.02).astype(np.float32)


def predictions(rng, gt, i0, p):
    """Predictions of frames i0 .. i0+p-1: a per-clip similarity of the ground truth plus 0.04 m joint noise."""
    b, j = gt.shape[0], gt.shape[2]
    out = np.empty((b, p, j, 3), dtype=np.float64)
    for i in range(b):
        r, a = pr.random_rotation(rng), rng.uniform(0.8, 1.25)
        x = gt[i, i0:i0 + p].astype(np.float64)
        c = x.mean(axis=(0, 1))
        out[i] = a * (x - c) @ r.T + c + rng.standard_normal(3) * 0.1 + rng.standard_normal((p, j, 3)) * 0.04
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_inputs(case) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(pred, gt, group) of one entry of CASES, seed b*1000 + J*10 + p; with more than two groups some stay empty.  Shared: do not
    write to the arrays."""
    b, p, t_gt, i0, j, n_groups, root, n_thr = case
    rng = np.random.default_rng(b * 1000 + j * 10 + p)
    gt = clips(rng, b, t_gt, j)
    pred = predictions(rng, gt, i0, p)
    used = rng.permutation(n_groups)[:max(1, n_groups - 2)] if n_groups > 2 else np.arange(n_groups)
    group = rng.choice(used, size=b)
    for a in (pred, gt, group):
        a.setflags(write=False)
    return pred, gt, group


@functools.lru_cache(maxsize=None)
def case_distances(case):
    """``distances`` of one entry of CASES, computed once."""
    pred, gt, _ = case_inputs(case)
    return distances(pred, gt, case[3], case[6])


@functools.lru_cache(maxsize=None)
def case_sums(case) -> np.ndarray:
    """``detail_sums`` of one entry of CASES, computed once.  Shared: do not write to it."""
    pred, gt, group = case_inputs(case)
    b, p, t_gt, i0, j, n_groups, root, n_thr = case
    acc = detail_sums(pred, gt, i0, group, n_groups, root, n_thr, THR_MAX, dists=case_distances(case))
    acc.setflags(write=False)
    return acc
