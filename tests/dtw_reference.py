"""numpy fp64 oracle of the forecast error after dynamic time warping, written from the definitions.

Per clip, ``Y_0..Y_{P-1}`` the predicted poses and ``X_0..X_{Q-1}`` = ``gt[i0 : i0+Q]``: ``C1[i][j]`` / ``C2[i][j]`` are
``protocols_reference.p1_pose`` / ``p2_pose`` of ``(Y_i, X_j)`` (an SVD where the kernel runs Horn's quaternion form).  ``band < 0`` allows
every cell, ``band >= 0`` the cells with ``|i - j| <= band`` (``band >= |P - Q|`` or ``ValueError``).  The DP is closed-ended:
``D[0][0] = C[0][0]``, ``D[i][j] = C[i][j]`` + the best predecessor among (i-1,j-1), (i-1,j), (i,j-1) that exist and are allowed, taken
in that order, a later one replacing the current one only if strictly smaller (ties: diagonal, up, left; a NaN never replaces
anything).  The path is the backtrack from (P-1, Q-1) to (0, 0).

``dtw_clip`` also returns the clip's **decision margin**: the smallest gap between the best and the second-best existing predecessor
over the cells of its path (``inf`` where a cell has one candidate): below it, a change of the costs cannot move the path."""
from typing import Dict, List, Tuple

import numpy as np

from tests import protocols_reference as pr

MOVES = ((-1, -1), (-1, 0), (0, -1))                    # diagonal, up, left: the order of the tie rule


def allowed(i: int, j: int, band: int) -> bool:
    return band < 0 or abs(i - j) <= band


def cost_matrices(pred, gt, root: int = 0) -> np.ndarray:
    """(2, P, Q) fp64: [P1, P2] of every (predicted frame, ground-truth frame) pair of one clip; pred (P, J, 3), gt (Q, J, 3)."""
    p, q = len(pred), len(gt)
    c = np.empty((2, p, q), dtype=np.float64)
    for i in range(p):
        for j in range(q):
            c[0, i, j] = pr.p1_pose(pred[i], gt[j], root)
            c[1, i, j] = pr.p2_pose(pred[i], gt[j])
    return c


def dtw_path(c: np.ndarray, band: int = -1) -> Dict[str, object]:
    """The DP and backtrack over one cost matrix c (P, Q): total, L, path [(i, j)] from (0, 0) onward, cost_sum / cells / lag_sum (P,)
    and the decision margin."""
    p, q = c.shape
    if 0 <= band < abs(p - q):
        raise ValueError(f"a band >= 0 must be >= |P - Q| = {abs(p - q)}, got {band}")
    d = np.full((p, q), np.nan)
    choice = np.full((p, q), 3, dtype=np.int64)
    gap = np.full((p, q), np.inf)
    for i in range(p):
        for j in range(q):
            if not allowed(i, j, band):
                continue
            cands = [(n, d[i + di, j + dj]) for n, (di, dj) in enumerate(MOVES)
                     if i + di >= 0 and j + dj >= 0 and allowed(i + di, j + dj, band)]
            if not cands:
                d[i, j] = c[i, j]                                      # the origin
                continue
            best_n, best = cands[0]
            for n, v in cands[1:]:
                if v < best:
                    best_n, best = n, v
            d[i, j] = c[i, j] + best
            choice[i, j] = best_n
            others = [v for n, v in cands if n != best_n]
            if others:
                with np.errstate(invalid="ignore"):
                    gap[i, j] = min(others) - best if np.all(np.isfinite([best] + others)) else 0.0
    path, i, j = [], p - 1, q - 1
    for _ in range(p + q - 1):
        path.append((i, j))
        if i == 0 and j == 0:
            break
        di, dj = MOVES[choice[i, j]]
        i, j = i + di, j + dj
    path.reverse()
    cost_sum, cells, lag_sum = np.zeros(p), np.zeros(p, dtype=np.int64), np.zeros(p, dtype=np.int64)
    for i, j in path:
        cost_sum[i] += c[i, j]
        cells[i] += 1
        lag_sum[i] += i - j
    return {"total": float(d[p - 1, q - 1]), "L": len(path), "path": path, "cost_sum": cost_sum, "cells": cells, "lag_sum": lag_sum,
            "margin": float(min(gap[i, j] for i, j in path))}


def dtw_clip(pred, gt, root: int = 0, band: int = -1) -> Tuple[List[Dict[str, object]], np.ndarray]:
    """([P1's result, P2's result] of ``dtw_path``, the cost matrices (2, P, Q)) of one clip: pred (P, J, 3), gt (Q, J, 3)."""
    c = cost_matrices(pred, gt, root)
    return [dtw_path(c[m], band) for m in (0, 1)], c


def record(res: Dict[str, object]) -> np.ndarray:
    """One metric's per-clip record in the layout of ``clip_out``: [total, L, cost_sum[P], cells[P], lag_sum[P]]."""
    return np.concatenate([[res["total"], float(res["L"])], res["cost_sum"], res["cells"].astype(np.float64),
                           res["lag_sum"].astype(np.float64)])


def path_array(res: Dict[str, object], p: int, q: int) -> np.ndarray:
    """(P+Q-1, 2) int32: the path's (i, j) pairs from (0, 0) onward, -1 past L (the layout of ``path_out``)."""
    out = np.full((p + q - 1, 2), -1, dtype=np.int32)
    out[:res["L"]] = np.asarray(res["path"], dtype=np.int32)
    return out


def dtw_batch(pred, gt, i0: int, q: int, root: int = 0, band: int = -1):
    """Every clip of a batch: pred (B, P, J, 3), gt (B, T, J, 3).  Returns (results [B][2], clip_out (B, 2, 2+3P) fp64, path_out
    (B, 2, P+Q-1, 2) int32, margins (B, 2))."""
    pred, gt = pr._f64(pred), pr._f64(gt)
    b, p = pred.shape[:2]
    if i0 < 0 or q < 1 or i0 + q > gt.shape[1]:
        raise ValueError(f"need 0 <= i0 and i0 + Q <= T (got i0={i0}, Q={q}, T={gt.shape[1]})")
    results = [dtw_clip(pred[i], gt[i, i0:i0 + q], root, band)[0] for i in range(b)]
    clip_out = np.stack([np.stack([record(r[m]) for m in (0, 1)]) for r in results])
    path_out = np.stack([np.stack([path_array(r[m], p, q) for m in (0, 1)]) for r in results])
    margins = np.array([[r[m]["margin"] for m in (0, 1)] for r in results])
    return results, clip_out, path_out, margins


def dtw_sums(clip_out: np.ndarray, group, n_groups: int) -> np.ndarray:
    """The fp64 accumulator ``r50_op_dtw_protocols`` adds, from per-clip records (B, 2, 2+3P): with V = 1 + 2P, ``[(g*2 + m)*V]`` = the
    sum of total / L, ``[(g*2 + m)*V + 1 + k]`` = of cost_sum[k] / cells[k], ``[(g*2 + m)*V + 1 + P + k]`` = of lag_sum[k] / cells[k],
    ``[2*n_groups*V + g]`` = clips."""
    group = np.asarray(group.cpu() if hasattr(group, "cpu") else group).astype(np.int64)
    b = clip_out.shape[0]
    p = (clip_out.shape[2] - 2) // 3
    v = 1 + 2 * p
    acc = np.zeros(n_groups * 2 * v + n_groups, dtype=np.float64)
    for i in range(b):
        g = int(group[i])
        acc[2 * n_groups * v + g] += 1.0
        for m in (0, 1):
            rec = clip_out[i, m]
            cells = rec[2 + p:2 + 2 * p]
            base = (g * 2 + m) * v
            acc[base] += rec[0] / rec[1]
            acc[base + 1:base + 1 + p] += rec[2:2 + p] / cells
            acc[base + 1 + p:base + 1 + 2 * p] += rec[2 + 2 * p:] / cells
    return acc


def values_from_sums(acc: np.ndarray, n_groups: int, p: int) -> Dict[str, np.ndarray]:
    """The reported values from an accumulator: ``dtw`` (G, 2), ``dtw_all`` (2,), ``dtw_mean`` (2,), ``dtw_future`` (G, P, 2),
    ``dtw_future_all`` (P, 2), ``lag`` (G, P, 2), ``lag_all`` (P, 2), ``clips`` (G,).  A group's value is its sum over its clip count (NaN
    without clips), ``all`` the same over every clip, the mean the plain mean over the groups that have clips."""
    v = 1 + 2 * p
    sums = np.asarray(acc[:n_groups * 2 * v], dtype=np.float64).reshape(n_groups, 2, v)
    clips = np.asarray(acc[n_groups * 2 * v:], dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_group = sums / clips[:, None, None]
    all_ = sums.sum(axis=0) / clips.sum()
    return {"clips": clips, "dtw": per_group[:, :, 0], "dtw_all": all_[:, 0], "dtw_mean": per_group[clips > 0][:, :, 0].mean(axis=0),
            "dtw_future": per_group[:, :, 1:1 + p].transpose(0, 2, 1), "dtw_future_all": all_[:, 1:1 + p].T,
            "lag": per_group[:, :, 1 + p:].transpose(0, 2, 1), "lag_all": all_[:, 1 + p:].T}


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def walk_clips(rng, b: int, t: int, j: int) -> np.ndarray:
    """(B, T, J, 3) fp32 ground truth whose frame order matters: the clips of tests/test_protocols_gpu.py (a person a few metres from
    the camera, joints spread ~0.3 m, 0.02-m jitter per frame) plus a random walk of 0.03-m steps per joint."""
    centre = rng.standard_normal((b, 1, 1, 3)) * np.array([1.0, 0.5, 0.5]) + np.array([0.0, 0.0, 4.5])
    body = rng.standard_normal((b, 1, j, 3)) * 0.3
    clips = centre + body + rng.standard_normal((b, t, j, 3)) * 0.02
    return (clips + np.cumsum(rng.standard_normal((b, t, j, 3)) * 0.03, axis=1)).astype(np.float32)


def resample(x: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """x (T, ...) linearly interpolated at the fractional frame positions pos (clamped to [0, T-1])."""
    pos = np.clip(pos, 0.0, len(x) - 1.0)
    lo = np.minimum(np.floor(pos).astype(np.int64), max(len(x) - 2, 0))
    hi = np.minimum(lo + 1, len(x) - 1)
    w = (pos - lo).reshape((-1,) + (1,) * (x.ndim - 1))
    return x[lo] * (1.0 - w) + x[hi] * w


def slowed_predictions(rng, gt: np.ndarray, i0: int, p: int, q: int, similarity: bool) -> np.ndarray:
    """(B, P, J, 3) fp32 predictions: gt[i0 : i0+q] resampled at a per-clip speed in [0.6, 1.0] (frame k shows position k * speed) plus
    0.01-m joint noise; with ``similarity`` a per-clip similarity on top (for P2: P1's path would be the diagonal's)."""
    b, j = gt.shape[0], gt.shape[2]
    out = np.empty((b, p, j, 3), dtype=np.float64)
    for i in range(b):
        x = gt[i, i0:i0 + q].astype(np.float64)
        y = resample(x, np.arange(p) * rng.uniform(0.6, 1.0)) + rng.standard_normal((p, j, 3)) * 0.01
        if similarity:
            r, a = pr.random_rotation(rng), rng.uniform(0.8, 1.25)
            c = y.mean(axis=(0, 1))
            y = a * (y - c) @ r.T + c + rng.standard_normal(3) * 0.1
        out[i] = y
    return out.astype(np.float32)


def plateau_inputs(j: int = 5) -> Tuple[np.ndarray, np.ndarray, List[Tuple[int, int]]]:
    """(pred (1, 6, J, 3), gt (1, 6, J, 3), the P1 path the tie rule gives): a base sequence a b c d of well-separated poses (exact in
    fp32), pred = a a b c d d and gt = a b b c c d.  Every pair of equal poses costs exactly 0 in P1, every other pair is positive, so P1's
    total is exactly 0 while the plain (diagonal) P1 is not, and the path is decided by exact zeros against positives."""
    base = np.zeros((4, j, 3), dtype=np.float32)
    for k in range(4):
        base[k, :, 0] = np.arange(j, dtype=np.float32) * np.float32(0.25) * np.float32(k + 1)
        base[k, :, 1] = np.float32(0.5) * np.float32(k) * (np.arange(j, dtype=np.float32) % 2)
        base[k, :, 2] = np.float32(4.0)
    pred = base[[0, 0, 1, 2, 3, 3]][None]
    gt = base[[0, 1, 1, 2, 2, 3]][None]
    path = [(0, 0), (1, 0), (2, 1), (2, 2), (3, 3), (3, 4), (4, 5), (5, 5)]
    return pred, gt, path
