"""INTEGRATION.md section W restated in plain numpy fp64, from the definitions: segments, the two FIR tables, the position-dependent
FIR, the One-Euro recurrence, bone statistics and the rebuild.  Slow loops on purpose: one line per line of the definition."""
import math

import numpy as np


def segments(seq_start, idx):
    """[(first row, one past the last row)] of every maximal run of consecutive ``idx`` inside one sequence."""
    out = []
    for s in range(len(seq_start) - 1):
        a, b = int(seq_start[s]), int(seq_start[s + 1])
        first = a
        for r in range(a + 1, b):
            if int(idx[r]) != int(idx[r - 1]) + 1:
                out.append((first, r))
                first = r
        out.append((first, b))
    return out


def segment_table(seq_start, idx):
    segs = segments(seq_start, idx)
    seg_start = np.array([a for a, _ in segs] + [segs[-1][1]], dtype=np.int32)
    row_seg = np.concatenate([np.full(b - a, g, dtype=np.int32) for g, (a, b) in enumerate(segs)])
    return seg_start, row_seg


def gauss_table(sigma):
    r = int(math.ceil(3.0 * sigma))
    w = 2 * r + 1
    coef = np.zeros((w, w), dtype=np.float64)
    for e in range(w):
        for k in range(w):
            if abs(k - e) <= r:
                coef[e, k] = math.exp(-((k - e) ** 2) / (2.0 * sigma * sigma))
        coef[e] /= coef[e].sum()
    return coef


def savgol_table(window, degree):
    """Row e: the weights of the least-squares polynomial's value at position e, through the pseudo-inverse of the Vandermonde matrix
    (positions centred and scaled, which changes the basis and not the fit)."""
    r = (window - 1) // 2
    t = (np.arange(window, dtype=np.float64) - r) / max(r, 1)
    a = np.vander(t, degree + 1, increasing=True)
    return a @ np.linalg.pinv(a)


def fir(x, seq_start, idx, coef):
    """x (F, J, 3) fp32 -> (out fp32, rows copied because their segment is shorter than W)."""
    x = np.asarray(x, dtype=np.float32)
    w = coef.shape[0]
    r = (w - 1) // 2
    out = np.empty_like(x)
    short = 0
    for a, b in segments(seq_start, idx):
        n = b - a
        if n < w:
            out[a:b] = x[a:b]
            short += n
            continue
        seg = x[a:b].astype(np.float64)
        for pos in range(n):
            lo = min(max(pos - r, 0), n - w)
            e = pos - lo
            acc = np.zeros(x.shape[1:], dtype=np.float64)
            for k in range(w):
                acc = acc + coef[e, k] * seg[lo + k]
            out[a + pos] = acc.astype(np.float32)
    return out, short


def alpha(fc, te):
    return 1.0 / (1.0 + 1.0 / ((6.283185307179586 * fc) * te))


def one_euro(x, seq_start, idx, rate, min_cutoff, beta, d_cutoff):
    x = np.asarray(x, dtype=np.float32)
    out = np.empty_like(x)
    te = 1.0 / rate
    ad = alpha(d_cutoff, te)
    for a, b in segments(seq_start, idx):
        out[a] = x[a]
        xhat = x[a].astype(np.float64)
        dxhat = np.zeros_like(xhat)
        for r in range(a + 1, b):
            xt = x[r].astype(np.float64)
            dx = (xt - xhat) * rate
            dxhat = dxhat + ad * (dx - dxhat)
            fc = min_cutoff + beta * np.abs(dxhat)
            xhat = xhat + alpha(fc, te) * (xt - xhat)
            out[r] = xhat.astype(np.float32)
    return out


def bone_lengths(x, edges):
    """(F, E) fp64."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    e = np.asarray(edges)
    d = x[:, e[:, 1]] - x[:, e[:, 0]]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def bone_stats(x, seq_start, edges):
    """(S, E, 2) fp64: the mean length and the sum of squared deviations from it (math.fsum: the exactly rounded sums)."""
    ln = bone_lengths(x, edges)
    s_n, e_n = len(seq_start) - 1, ln.shape[1]
    out = np.zeros((s_n, e_n, 2), dtype=np.float64)
    for s in range(s_n):
        a, b = int(seq_start[s]), int(seq_start[s + 1])
        for q in range(e_n):
            mean = math.fsum(ln[a:b, q]) / (b - a)
            out[s, q, 0] = mean
            out[s, q, 1] = math.fsum((ln[a:b, q] - mean) ** 2)
    return out


def bone_rebuild(x, seq_start, edges, stats):
    x = np.asarray(x, dtype=np.float32)
    out = x.copy()
    for s in range(len(seq_start) - 1):
        for r in range(int(seq_start[s]), int(seq_start[s + 1])):
            pos = x[r].astype(np.float64)
            orig = x[r].astype(np.float64)
            for q, (pa, ch) in enumerate(edges):
                d = orig[ch] - orig[pa]
                n = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                pos[ch] = pos[pa] + (d if n == 0.0 else (stats[s, q, 0] * d) / n)
                out[r, ch] = pos[ch].astype(np.float32)
    return out


def bone_std_mm(x, seq_start, edges, seqs=None):
    """The pooled bone-length standard deviation over time, in mm: sqrt(sum of squared deviations from the own sequence's mean / terms)."""
    st = bone_stats(x, seq_start, edges)
    seqs = range(len(seq_start) - 1) if seqs is None else seqs
    ssd = sum(float(st[s, :, 1].sum()) for s in seqs)
    terms = sum((int(seq_start[s + 1]) - int(seq_start[s])) * st.shape[1] for s in seqs)
    return 1000.0 * math.sqrt(ssd / terms)


def ulp_distance(a, b):
    """|a - b| in units of fp32 spacing, per element (finite fp32 arrays): the distance between their ordered integer images."""
    def key(v):
        i = np.asarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
