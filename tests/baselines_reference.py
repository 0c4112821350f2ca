"""numpy fp64 oracle of the forecast baselines: the nearest-neighbour search over 16-bit rows, its derived
error bound, and the three trivial forecasts restated operation by operation.

Search.  Operands are the 16-bit-rounded rows read back as fp64.  True score ``s(q, x) = |x|^2 - 2 q.x``; the device computes
``s^ = x_norm2[x] - 2 fl(q.x)`` with fp32 accumulation.  With ``u = 2^-24`` and ``gamma = (d + 2) u / (1 - (d + 2) u)``: products of two
16-bit values are exact in fp32, so only the sums err, and whatever their order ``|s^ - s| <= E(q, x) = gamma (2 |q| |x| + |x|^2)``.
``E_q = max_x E(q, x)``.  Order statistics move by at most the perturbation: the true score of the device's r-th row lies within
``2 E_q`` of the oracle's r-th smallest.  The device's list equals the oracle's for every query that ``separated`` marks: each of its
k best rows is further below every later row than the two rows' E together.

Forecasts.  fp32 operations, each rounded once, so numpy's float32 arithmetic restates them bit for bit; the one fma is evaluated
exactly (``fractions``) and rounded once to float32."""
from fractions import Fraction
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

U = 2.0 ** -24
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def gamma(d: int) -> float:
    return (d + 2) * U / (1.0 - (d + 2) * U)


def rows16(shape, seed: int, precision: str = "fp16", scale: float = 1.0) -> torch.Tensor:
    """Seeded standard-normal rows rounded to the 16-bit type (a CPU tensor of that type)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DTYPES[precision])


def f64(t) -> np.ndarray:
    if hasattr(t, "detach"):
        t = t.detach().cpu().to(torch.float64).numpy()
    return np.asarray(t, dtype=np.float64)


def true_scores(q, x) -> np.ndarray:
    """(NQ, N) fp64: |x|^2 - 2 q.x of the 16-bit rows."""
    q, x = f64(q), f64(x)
    return (x * x).sum(axis=1)[None, :] - 2.0 * (q @ x.T)


def bound_e(q, x) -> np.ndarray:
    """(NQ, N): E(q, x) = gamma (2 |q| |x| + |x|^2)."""
    q, x = f64(q), f64(x)
    qn, xn = np.sqrt((q * q).sum(axis=1)), np.sqrt((x * x).sum(axis=1))
    return gamma(q.shape[1]) * (2.0 * qn[:, None] * xn[None, :] + (xn * xn)[None, :])


def order(scores: np.ndarray) -> np.ndarray:
    """Row-wise ascending order by (score, index): a stable argsort."""
    return np.argsort(scores, axis=1, kind="stable")


def search(q, x, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(idx (NQ, k), score (NQ, k), dist2 (NQ, k)) of the exact search, ascending by (score, index)."""
    s = true_scores(q, x)
    idx = order(s)[:, :k]
    sc = np.take_along_axis(s, idx, axis=1)
    qq = f64(q)
    return idx, sc, np.maximum(0.0, (qq * qq).sum(axis=1)[:, None] + sc)


def brute_force(q, x, k: int) -> np.ndarray:
    """The same lists by plain loops and tuple comparison: the self-check of ``search``."""
    q, x = f64(q), f64(x)
    out = np.zeros((q.shape[0], k), dtype=np.int64)
    for a in range(q.shape[0]):
        pairs = sorted((float((x[i] * x[i]).sum() - 2.0 * (q[a] * x[i]).sum()), i) for i in range(x.shape[0]))
        out[a] = [i for _, i in pairs[:k]]
    return out


def separated(q, x, k: int) -> np.ndarray:
    """(NQ,) bool: the queries whose list no admissible perturbation can change: for each of the k best rows r and every row j after it in
    the true order, s_j - s_r > E_r + E_j."""
    s, e = true_scores(q, x), bound_e(q, x)
    o = order(s)
    ss, ee = np.take_along_axis(s, o, axis=1), np.take_along_axis(e, o, axis=1)
    ok = np.ones(s.shape[0], dtype=bool)
    for r in range(min(k, s.shape[1])):
        later = slice(r + 1, None)
        ok &= np.all(ss[:, later] - ss[:, r:r + 1] > ee[:, later] + ee[:, r:r + 1], axis=1)
    return ok


def fp32_scores(q, x) -> np.ndarray:
    """The device's arithmetic emulated in numpy float32 (some summation order): norms and dot products in fp32."""
    q32, x32 = f64(q).astype(np.float32), f64(x).astype(np.float32)
    xn = np.array([np.sum(r * r, dtype=np.float32) for r in x32], dtype=np.float32)
    dot = np.array([[np.sum(a * r, dtype=np.float32) for r in x32] for a in q32], dtype=np.float32)
    return xn[None, :] - np.float32(2.0) * dot


def value_bound(q, x) -> np.ndarray:
    """(NQ,): 2 E_q, the distance a returned row's TRUE score may lie from the oracle's score at the same rank."""
    return 2.0 * bound_e(q, x).max(axis=1)


def dist2_bound(q, x) -> np.ndarray:
    """(NQ,): 2 E_q + u (|q|^2 + max |x|^2), the bound on ``dist2_out`` against the oracle's."""
    qq, xx = f64(q), f64(x)
    return value_bound(q, x) + U * ((qq * qq).sum(axis=1) + (xx * xx).sum(axis=1).max())


# ---- the forecasts ------------------------------------------------------------------------------------------------------------------
def _round32(v: Fraction) -> np.float32:
    """The float32 nearest to the exact value, ties to even: the fp64 rounding on the way is only a first guess."""
    best = np.float32(float(v))
    for cand in (np.nextafter(best, np.float32(-np.inf)), np.nextafter(best, np.float32(np.inf))):
        dc, db = abs(v - Fraction(float(cand))), abs(v - Fraction(float(best)))
        if dc < db or (dc == db and not (cand.view(np.uint32) & 1) and (best.view(np.uint32) & 1)):
            best = cand
    return best


def _fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fl32(a * b + c), exactly evaluated (``fractions``) and rounded once."""
    flat = [_round32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
            for x, y, z in zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())]
    return np.array(flat, dtype=np.float32).reshape(a.shape)


def forecasts(a1, a0, nn_row, dbj, input_len: int, pred_len: int, which: Sequence[str], root: int = 0) -> Dict[str, np.ndarray]:
    """``r50_op_baseline_forecasts`` restated: a1, a0 (B, J, 3); nn_row (B, k) rows of dbj (N, T, J, 3); all read as fp32."""
    def f32(t) -> Optional[np.ndarray]:
        if t is None:
            return None
        return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)

    a1, a0, dbj = f32(a1), f32(a0), f32(dbj)
    b, j, _ = a1.shape
    i_len, p_len = int(input_len), int(pred_len)
    out: Dict[str, np.ndarray] = {}
    if "const_pose" in which:
        out["const_pose"] = np.broadcast_to(a1[:, None], (b, p_len, j, 3)).copy()
    if "const_vel" in which:
        step = a1 - a0                                                                  # one fp32 subtraction
        h1 = np.arange(1, p_len + 1, dtype=np.float32)[None, :, None, None]
        shape = (b, p_len, j, 3)
        out["const_vel"] = _fma32(np.broadcast_to(h1, shape), np.broadcast_to(step[:, None], shape), np.broadcast_to(a1[:, None], shape))
    if "nn" in which:
        rows = np.asarray(nn_row.detach().cpu().numpy() if hasattr(nn_row, "detach") else nn_row, dtype=np.int64)
        k = rows.shape[1]
        total = None
        for i in range(k):                                                              # left to right, fp32
            clip = dbj[rows[:, i]]                                                      # (B, T, J, 3)
            term = clip[:, i_len:i_len + p_len] - clip[:, i_len - 1, root][:, None, None, :]
            total = term if total is None else total + term
        out["nn"] = a1[:, root][:, None, None, :] + total / np.float32(k)
    return {name: np.asarray(v, dtype=np.float32) for name, v in out.items()}


def grid_poses(shape, seed: int) -> torch.Tensor:
    """Seeded fp32 poses: half on a coarse grid (multiples of 2^-10 within +-4, where sums cancel exactly and tie), half Gaussian."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.randint(-4096, 4097, shape, generator=g).to(torch.float32) / 1024.0
    return torch.where(torch.rand(shape, generator=g) < 0.5, grid, torch.randn(shape, generator=g))


def horizon_sums(pred, gt, input_len: int) -> np.ndarray:
    """The accumulator ``r50_op_horizon_metrics`` adds, with ITS arithmetic: per joint the difference, its square sum and the square
    root in fp32 (each operation rounded once, in the kernel's order), the sums over clips and joints in fp64:
    [per-horizon distance sums (P) | squared-error sums (P) | clips]."""
    f32 = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)      # noqa: E731
    pred, gt = f32(pred), f32(gt)
    p = pred.shape[1]
    d = pred - gt[:, input_len:input_len + p]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    dist = np.sqrt(d2)
    assert d2.dtype == np.float32 and dist.dtype == np.float32
    return np.concatenate([dist.astype(np.float64).sum(axis=(0, 2)), d2.astype(np.float64).sum(axis=(0, 2)), [float(pred.shape[0])]])
