"""numpy restatement of include/r50_resample.h: a loop over output rows, fp64 on the fp32 positions with every product, quotient and sum
rounded on its own in the order the header writes it, float32 at the end.  Test infrastructure: the product never imports it.

Also the tables the tests share: ``left_rows`` (the definition of ``out_left`` by a plain scan), ``ragged_case`` (the one ragged table of
tests/test_resample_gpu.py and of the guard-band rows) and ``holdout_rows`` (the kept rows of ``results --dense-holdout``, by a scan)."""
import numpy as np

LINEAR, CUBIC = 0, 1
IN_BREAK, OUTSIDE = 1, 2
KINDS = {"linear": LINEAR, "cubic": CUBIC}


def left_rows(seq_start, idx, out_time, out_seq):
    """``out_left`` by its definition: the last row i of the sequence with idx[i] <= tau, or the sequence's first row."""
    out = np.empty(len(out_time), dtype=np.int32)
    for g, (tau, s) in enumerate(zip(out_time, out_seq)):
        a, b = int(seq_start[s]), int(seq_start[s + 1])
        i = a
        for r in range(a, b):
            if float(idx[r]) <= tau:
                i = r
        out[g] = i
    return out


def _secant(x, idx, p, q):
    return (x[q] - x[p]) / np.float64(int(idx[q]) - int(idx[p]))


def resample(x, idx, seq_start, out_time, out_seq, out_left, kind, max_gap):
    """x (F, J, 3) fp32 -> (y (G, J, 3) fp32, flags (G,) int32)."""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    xd = x32.astype(np.float64)
    idx = np.asarray(idx)
    kind = KINDS.get(kind, kind)
    g_rows = len(out_time)
    y = np.empty((g_rows,) + x32.shape[1:], dtype=np.float32)
    flags = np.zeros(g_rows, dtype=np.int32)
    zero = np.float64(0.0)

    def bridged(p, q, a, b):
        return a <= p and q < b and int(idx[q]) - int(idx[p]) <= max_gap

    for g in range(g_rows):
        tau, s, i = np.float64(out_time[g]), int(out_seq[g]), int(out_left[g])
        a, b = int(seq_start[s]), int(seq_start[s + 1])
        t0 = np.float64(int(idx[i]))
        if tau == t0:
            y[g] = x32[i]
            continue
        if tau < t0 or i + 1 >= b:
            y[g], flags[g] = x32[i], OUTSIDE
            continue
        if not bridged(i, i + 1, a, b):
            left = (tau - t0) <= (np.float64(int(idx[i + 1])) - tau)
            y[g], flags[g] = x32[i if left else i + 1], IN_BREAK
            continue
        h = np.float64(int(idx[i + 1]) - int(idx[i]))
        u = (tau - t0) / h
        x0, x1 = xd[i], xd[i + 1]
        if kind == LINEAR:
            y[g] = ((x0 + u * (x1 - x0)) + zero).astype(np.float32)
            continue
        u2 = u * u
        u3 = u2 * u
        two, three, one = np.float64(2.0), np.float64(3.0), np.float64(1.0)
        h00 = ((two * u3) - (three * u2)) + one
        h10 = (u3 - (two * u2)) + u
        h01 = (-(two * u3)) + (three * u2)
        h11 = u3 - u2
        has_left, has_right = bridged(i - 1, i, a, b), bridged(i + 1, i + 2, a, b)
        d01 = _secant(xd, idx, i, i + 1)
        if has_left:
            hl = np.float64(int(idx[i]) - int(idx[i - 1]))
            dm = _secant(xd, idx, i - 1, i)
        if has_right:
            hr = np.float64(int(idx[i + 2]) - int(idx[i + 1]))
            dp = _secant(xd, idx, i + 1, i + 2)
        if has_left:                         # knot i: both neighbours
            m0 = (h * dm + hl * d01) / (hl + h)
        elif has_right:                      # only the right one, and [i+1, i+2] is bridged too
            m0 = (((two * h) + hr) * d01 - h * dp) / (h + hr)
        else:
            m0 = d01
        if has_right:                        # knot i+1: both neighbours
            m1 = (hr * d01 + h * dp) / (h + hr)
        elif has_left:                       # only the left one, and [i-1, i] is bridged too
            m1 = (((two * h) + hl) * d01 - h * dm) / (h + hl)
        else:
            m1 = d01
        y[g] = ((((h00 * x0 + (h10 * h) * m0) + h01 * x1) + (h11 * h) * m1) + zero).astype(np.float32)
    return y, flags


def table(seq_start, idx, out_time, out_seq):
    """The four tables as the arrays the op reads."""
    out_time = np.asarray(out_time, dtype=np.float64)
    out_seq = np.asarray(out_seq, dtype=np.int32)
    return dict(seq_start=np.asarray(seq_start, dtype=np.int32), idx=np.asarray(idx, dtype=np.int32), out_time=out_time, out_seq=out_seq,
                out_left=left_rows(seq_start, idx, out_time, out_seq))


MAX_GAP = 3
LENS = (1, 2, 3, 4, 7, 130)
# gaps per sequence: of exactly MAX_GAP (bridged) and MAX_GAP + 1 (a break), the latter also directly beside a run end.
#   7 rows: 0 1 | 5 6 9 | 13 14   -> the run {0, 1} of two knots (secant), the run {5, 6, 9} with a gap of exactly 3 and both one-sided rules,
#                                    the run {13, 14} ending the sequence right behind a break
_STEPS = {1: [], 2: [4], 3: [1, 3], 4: [3, 4, 1], 7: [1, 4, 1, 3, 4, 1]}


def ragged_case(joints, seed=0, shift=0, quantum=None):
    """Sequences of 1, 2, 3, 4, 7 and 130 rows (the long one: steps 1 2 3 with a break of 4 every 23rd step and right before its last row)
    and output times that hit every case of the header.  G is odd, so G * 3 J is no multiple of 256 for any J: the last workgroup is
    ragged.  With ``quantum`` the times are rounded to its multiples (a power of two: they then survive a ``shift`` of 2^30 exactly);
    ``shift`` is added to every stamp and time."""
    rng = np.random.default_rng(seed)
    idx, seq_start = [], [0]
    for n in LENS:
        if n in _STEPS:
            steps = _STEPS[n]
        else:
            steps = [(1, 2, 3)[k % 3] for k in range(n - 1)]
            for k in range(11, n - 1, 23):
                steps[k] = MAX_GAP + 1
            steps[-1] = MAX_GAP + 1
        stamps = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64) + 7 * len(seq_start) - 20      # some stamps negative
        idx.append(stamps)
        seq_start.append(seq_start[-1] + n)
    idx = np.concatenate(idx)
    times, seqs = [], []
    for s in range(len(LENS)):
        t = idx[seq_start[s]:seq_start[s + 1]].astype(np.float64)
        cand = [t, t[:1] - 2.5, t[:1] - 1e-9, t[-1:] + 1e-9, t[-1:] + 40.0, t[-1:]]                       # knots, outside, the last knot again
        if t.size > 1:
            cand += [(t[:-1] + t[1:]) / 2.0, t[:-1] + 1e-9, t[1:] - 1e-9, t[:-1] + 0.25 * (t[1:] - t[:-1]),     # midpoints (a break's tie point)
                     t[:-1] + rng.uniform(0.0, 1.0, t.size - 1) * (t[1:] - t[:-1])]
        cand = np.concatenate(cand)
        times.append(cand)
        seqs.append(np.full(cand.size, s))
    times, seqs = np.concatenate(times), np.concatenate(seqs)
    if quantum is not None:
        times = np.round(times / quantum) * quantum
    order = rng.permutation(times.size)                                     # output rows come in any order
    times, seqs = times[order], seqs[order]
    if times.size % 2 == 0:
        times, seqs = times[:-1], seqs[:-1]
    f = int(seq_start[-1])
    x = (rng.standard_normal((f, joints, 3)) * 0.3 + np.array([0.0, 0.0, 5.0])).astype(np.float32)
    x[::5, :, 0] = np.float32(-0.0)                                          # a copied row keeps its -0; an interpolated one stores +0
    out = table(seq_start, idx + shift, times + float(shift), seqs)
    out.update(x=x, f=f, s=len(LENS), g=int(times.size), j=joints, max_gap=MAX_GAP)
    return out


def holdout_rows(seq_start, idx, k):
    """The kept rows of ``results --dense-holdout K`` by a scan: in every segment (a maximal run of consecutive stamps of one sequence)
    the rows whose stamp is K * n past the segment's first, and the segment's last row."""
    keep = np.zeros(len(idx), dtype=bool)
    for s in range(len(seq_start) - 1):
        a, b = int(seq_start[s]), int(seq_start[s + 1])
        first = a
        for r in range(a, b):
            if r > a and int(idx[r]) != int(idx[r - 1]) + 1:
                first = r
            if (int(idx[r]) - int(idx[first])) % k == 0:
                keep[r] = True
            if r + 1 == b or int(idx[r + 1]) != int(idx[r]) + 1:
                keep[r] = True
    return keep
