"""numpy fp64 oracle of the two H3.6M evaluation protocols, written from the equations and solved with
``np.linalg.svd``: deliberately another solver than the kernel's (Horn's quaternion form, a Jacobi eigen-solve).

For one pose, X the ground truth and Y the prediction, both (J, 3), read as fp32 and computed in fp64:

* P1 (root-relative MPJPE): ``(1/J) sum_j |(Y_j - Y_r) - (X_j - X_r)|``;
* P2 (PA-MPJPE, Umeyama 1991): ``M = sum_j X0_j Y0_j^T = U D V^T``, ``S = diag(1, 1, sign(det U det V))``, ``R = U S V^T``,
  ``a = tr(D S) / sum_j |Y0_j|^2`` (0 when either pose has no spread), ``Yhat_j = a R (Y_j - muY) + muX``,
  P2 = ``(1/J) sum_j |Yhat_j - X_j|``.

``protocol_sums`` returns the accumulator ``r50_op_pose_protocols`` adds, in the same layout."""
from typing import Tuple

import numpy as np


def _f64(a) -> np.ndarray:
    """fp32 values in fp64: what the kernel reads (torch tensors or numpy arrays)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def p1_pose(pred, gt, root: int = 0) -> float:
    y, x = _f64(pred), _f64(gt)
    return float(np.linalg.norm((y - y[root]) - (x - x[root]), axis=-1).mean())


def similarity_fit(pred, gt) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
    """(a, R, muY, muX) of the proper similarity that maps the prediction onto the ground truth in the least-squares sense."""
    y, x = _f64(pred), _f64(gt)
    mu_y, mu_x = y.mean(axis=0), x.mean(axis=0)
    y0, x0 = y - mu_y, x - mu_x
    sy, sx = float((y0 ** 2).sum()), float((x0 ** 2).sum())
    m = x0.T @ y0                                                  # sum_j X0_j Y0_j^T
    u, d, vt = np.linalg.svd(m)
    s = np.array([1.0, 1.0, np.sign(np.linalg.det(u) * np.linalg.det(vt))])      # U, V orthogonal: det +-1, never 0
    r = u @ np.diag(s) @ vt
    a = 0.0 if sy == 0.0 or sx == 0.0 else float((d * s).sum()) / sy
    return a, r, mu_y, mu_x


def p2_pose(pred, gt) -> float:
    a, r, mu_y, mu_x = similarity_fit(pred, gt)
    y, x = _f64(pred), _f64(gt)
    y_hat = a * (y - mu_y) @ r.T + mu_x
    return float(np.linalg.norm(y_hat - x, axis=-1).mean())


def protocol_sums(pred, gt, i0: int, group, n_groups: int, root: int = 0) -> np.ndarray:
    """pred (B, P, J, 3) scores frames i0 .. i0+P-1 of gt (B, T, J, 3); group (B,) in [0, n_groups).  Returns the fp64 accumulator
    of ``r50_op_pose_protocols``: ``[(g*P + k)*2 + 0]`` = P1 sum, ``[(g*P + k)*2 + 1]`` = P2 sum, ``[2*n_groups*P + g]`` = clips."""
    pred, gt = _f64(pred), _f64(gt)
    group = np.asarray(group.cpu() if hasattr(group, "cpu") else group).astype(np.int64)
    b, p = pred.shape[:2]
    acc = np.zeros(2 * n_groups * p + n_groups, dtype=np.float64)
    for i in range(b):
        g = int(group[i])
        acc[2 * n_groups * p + g] += 1.0
        for k in range(p):
            acc[(g * p + k) * 2 + 0] += p1_pose(pred[i, k], gt[i, i0 + k], root)
            acc[(g * p + k) * 2 + 1] += p2_pose(pred[i, k], gt[i, i0 + k])
    return acc


def values_from_sums(acc: np.ndarray, n_groups: int, p: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(per-group values (G, P, 2), ``all`` values (P, 2), clips (G,)) from an accumulator: a group's value at frame k is its sum
    over clips divided by its clip count; ``all`` weighs every clip the same."""
    sums = np.asarray(acc[:2 * n_groups * p], dtype=np.float64).reshape(n_groups, p, 2)
    clips = np.asarray(acc[2 * n_groups * p:], dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_group = sums / clips[:, None, None]
    return per_group, sums.sum(axis=0) / clips.sum(), clips


def random_rotation(rng: np.random.Generator) -> np.ndarray:
    """A uniformly random proper rotation (QR of a Gaussian matrix, signs fixed, det +1)."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q
