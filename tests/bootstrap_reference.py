"""A numpy restatement of include/r50_bootstrap.h and of ``bootstrap.statistics`` (INTEGRATION.md section AC): Philox4x32-10 vectorised
on uint64 lanes, the multiply-shift mapping of a word to a unit, the multiplicities, the sequential ascending sums (every product and
every add rounded on its own, units with a multiplicity of 0 skipped) and the statistics of a replicate table.  Test infrastructure
only: the product never imports it."""
from decimal import ROUND_CEILING, Decimal

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter (..., 4) and key (2,) or (..., 2) of 32-bit values -> (..., 4) uint32.  The arithmetic is on uint64 lanes: a 32 x 32
    product fits, its halves are the round's hi and lo words."""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64) & MASK, c.shape[:-1] + (2,))
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def draw_units(stratum_start, rho, seed):
    """(U,) int64: the unit that the draw at each global position i names in replicate ``rho``."""
    ss = np.asarray(stratum_start, dtype=np.int64)
    u = int(ss[-1])
    i = np.arange(u, dtype=np.uint64)
    seed, rho = int(seed) & (2 ** 64 - 1), int(rho) & (2 ** 64 - 1)
    ctr = np.stack([i >> np.uint64(2), np.zeros_like(i), np.full_like(i, rho & 0xFFFFFFFF), np.full_like(i, rho >> 32)], axis=-1)
    words = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    word = words[np.arange(u), (i & np.uint64(3)).astype(np.int64)].astype(np.uint64)
    g = np.searchsorted(ss, np.arange(u), side="right") - 1
    a, n = ss[g], (ss[g + 1] - ss[g]).astype(np.uint64)
    return a + ((word * n) >> S32).astype(np.int64)


def counts(stratum_start, r0, reps, seed):
    """(R, U) int32: c[rho][u], the number of draws of replicate rho = r0 + r that name u."""
    u = int(np.asarray(stratum_start)[-1])
    out = np.zeros((reps, u), dtype=np.int32)
    for r in range(reps):
        out[r] = np.bincount(draw_units(stratum_start, r0 + r, seed), minlength=u)
    return out


def sums(v, stratum_start, c):
    """(R, G, M) fp64: out[r, g, m] = the sum over u = a_g .. b_g - 1, ascending and from +0.0, of (double)c[r, u] * v[u, m] with the
    units of multiplicity 0 skipped."""
    v = np.asarray(v, dtype=np.float64)
    ss = np.asarray(stratum_start, dtype=np.int64)
    reps, groups = c.shape[0], ss.size - 1
    out = np.zeros((reps, groups, v.shape[1]), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(groups):
            acc = np.zeros((reps, v.shape[1]), dtype=np.float64)
            for u in range(int(ss[g]), int(ss[g + 1])):
                cu = c[:, u].astype(np.float64)[:, None]
                acc = np.where(cu > 0, acc + cu * v[u][None, :], acc)
            out[:, g] = acc
    return out


def bootstrap_sums(v, stratum_start, reps, seed, r0=0):
    c = counts(stratum_start, r0, reps, seed)
    return sums(v, stratum_start, c), c


def point_sums(v, stratum_start):
    """(G, M): the sums at c = 1."""
    ss = np.asarray(stratum_start, dtype=np.int64)
    return sums(v, ss, np.ones((1, int(ss[-1])), dtype=np.int32))[0]


def _rows(s):
    """(..., G, M) sums whose last column is the count -> (..., G + 2, M - 1) values: all, the action mean, every stratum.  The sums over
    strata run in ascending stratum order, one add at a time."""
    val = s[..., :, :-1] / s[..., :, -1:]
    tot, mean = s[..., 0, :].copy(), val[..., 0, :].copy()
    for g in range(1, s.shape[-2]):
        tot = tot + s[..., g, :]
        mean = mean + val[..., g, :]
    all_ = tot[..., :-1] / tot[..., -1:]
    mean = mean / float(s.shape[-2])
    return np.concatenate([all_[..., None, :], mean[..., None, :], val], axis=-2)


def order_indices(reps, level):
    """ceil(q R) - 1 clamped to [0, R - 1] for q = (1 - level) / 2 and 1 - q, in exact decimal arithmetic on ``level`` as it prints."""
    q = (Decimal(1) - Decimal(repr(float(level)))) / Decimal(2)
    lo = int((q * reps).to_integral_value(rounding=ROUND_CEILING)) - 1
    hi = int(((Decimal(1) - q) * reps).to_integral_value(rounding=ROUND_CEILING)) - 1
    return min(max(lo, 0), reps - 1), min(max(hi, 0), reps - 1)


def statistics(s, point, level, pairs=0):
    """The restatement of ``bootstrap.statistics``: s (R, G, M), point (G, M).  With ``pairs`` = K > 0 the first K value columns are
    model A's and the next K model B's, and the B - A rows are added."""
    rep, pt = _rows(np.asarray(s, dtype=np.float64)), _rows(np.asarray(point, dtype=np.float64))
    reps = rep.shape[0]
    lo, hi = order_indices(reps, level)
    srt = np.sort(rep, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"point": pt, "se": rep.std(axis=0, ddof=1) if reps > 1 else np.full_like(pt, np.nan), "lo": srt[lo], "hi": srt[hi]}
    if pairs:
        d = rep[..., pairs:2 * pairs] - rep[..., :pairs]
        ds = np.sort(d, axis=0)
        p = ((d < 0).sum(axis=0) + 0.5 * (d == 0).sum(axis=0)) / reps
        with np.errstate(invalid="ignore", divide="ignore"):
            out.update(diff=pt[..., pairs:2 * pairs] - pt[..., :pairs], diff_se=d.std(axis=0, ddof=1) if reps > 1 else np.full_like(p, np.nan),
                       diff_lo=ds[lo], diff_hi=ds[hi], p_better=p, p_two_sided=2.0 * np.minimum(p, 1.0 - p))
    return out
