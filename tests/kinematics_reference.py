"""The definition of INTEGRATION.md section Y (include/r50_kinematics.h) in plain numpy fp64, joint by joint and frame by frame: the
oracle of tests/test_kinematics_cpu.py and tests/test_kinematics_gpu.py, and the generator of their articulated figures.  Nothing in
the product imports this file."""
import numpy as np

EDGES17 = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14), (14, 15),
           (15, 16))
FRAMES17 = ((0, 1, 4, 0, 7), (8, 14, 11, 8, 9))
SIGN_H36M = (1.0, -1.0, -1.0)


def rest_dirs17():
    d = np.zeros((17, 3))
    d[[1, 14, 15, 16]] = (-1.0, 0.0, 0.0)
    d[[4, 11, 12, 13]] = (1.0, 0.0, 0.0)
    d[[2, 3, 5, 6]] = (0.0, -1.0, 0.0)
    d[[7, 8, 9, 10]] = (0.0, 1.0, 0.0)
    return d


def norm3(v):
    return float(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def frame_of(xw, row):
    """R = [ex ey ez] of the frame row (a0, a1, b0, b1) on one world-frame pose, or None where a norm is exactly 0."""
    a0, a1, b0, b1 = row
    e = xw[a1] - xw[a0]
    n = norm3(e)
    if n == 0.0:
        return None
    ex = e / n
    z = cross(ex, xw[b1] - xw[b0])
    n = norm3(z)
    if n == 0.0:
        return None
    ez = z / n
    return np.stack([ex, cross(ez, ex), ez], axis=1)


def topology(edges, joints):
    parent = {int(c): int(p) for p, c in edges}
    root = [j for j in range(joints) if j not in parent]
    assert len(root) == 1, "one root"
    children = {j: [int(c) for p, c in edges if p == j] for j in range(joints)}
    return root[0], parent, children


def rest_offsets(x, seq_start, edges, frames, rest_dirs, sign):
    """rest (S, J, 3): sums over the rows in row order."""
    x = np.asarray(x, dtype=np.float64) * np.asarray(sign, dtype=np.float64)
    joints = x.shape[1]
    root, parent, _ = topology(edges, joints)
    framed = {int(f[0]): tuple(int(v) for v in f[1:]) for f in frames}
    rest = np.zeros((len(seq_start) - 1, joints, 3))
    for s in range(len(seq_start) - 1):
        rows = range(int(seq_start[s]), int(seq_start[s + 1]))
        for p, c in edges:
            length, vec, cnt = 0.0, np.zeros(3), 0
            for r in rows:
                d = x[r, c] - x[r, p]
                length += norm3(d)
                if p in framed:
                    m = frame_of(x[r], framed[p])
                    if m is not None:
                        vec = vec + m.T @ d
                        cnt += 1
            rest[s, c] = vec / cnt if cnt else np.asarray(rest_dirs[c]) * (length / len(rows))
    return rest


def skew(k):
    return np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])


def quat_of(m):
    """(w, x, y, z), Shepperd's largest pivot (the trace, then m00, m11, m22; a later one only if strictly larger), w >= 0."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    pick = int(np.argmax([t, m[0, 0], m[1, 1], m[2, 2]]))                          # argmax: the first of equal maxima
    if pick == 0:
        w = 0.5 * np.sqrt(1.0 + t)
        q = [w, (m[2, 1] - m[1, 2]) / (4 * w), (m[0, 2] - m[2, 0]) / (4 * w), (m[1, 0] - m[0, 1]) / (4 * w)]
    elif pick == 1:
        a = 0.5 * np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2])
        q = [(m[2, 1] - m[1, 2]) / (4 * a), a, (m[0, 1] + m[1, 0]) / (4 * a), (m[0, 2] + m[2, 0]) / (4 * a)]
    elif pick == 2:
        b = 0.5 * np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2])
        q = [(m[0, 2] - m[2, 0]) / (4 * b), (m[0, 1] + m[1, 0]) / (4 * b), b, (m[1, 2] + m[2, 1]) / (4 * b)]
    else:
        c = 0.5 * np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1])
        q = [(m[1, 0] - m[0, 1]) / (4 * c), (m[0, 2] + m[2, 0]) / (4 * c), (m[1, 2] + m[2, 1]) / (4 * c), c]
    q = np.array(q)
    return (-q if q[0] < 0.0 else q) + 0.0                                         # + 0.0: a -0 becomes +0


def quat_matrix(q):
    """The rotation of the quaternion q (w, x, y, z), renormalised first."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def euler_zxy_deg(m):
    """Degrees (Z, X, Y) with m = Rz(a) Rx(b) Ry(c)."""
    b = np.arcsin(min(1.0, max(-1.0, m[2, 1])))
    if abs(m[2, 1]) > 1.0 - 1e-12:
        a, c = np.arctan2(m[1, 0], m[0, 0]), 0.0
    else:
        a, c = np.arctan2(-m[0, 1], m[1, 1]), np.arctan2(-m[2, 0], m[2, 2])
    return np.degrees(np.array([a, b, c])) + 0.0


def rot_zxy_deg(e):
    a, b, c = np.radians(np.asarray(e, dtype=np.float64))
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    ry = np.array([[np.cos(c), 0.0, np.sin(c)], [0.0, 1.0, 0.0], [-np.sin(c), 0.0, np.cos(c)]])
    return rz @ rx @ ry


def pose_rotations(x, seq_start, edges, frames, rest_dirs, sign, rest=None):
    """Every output of the per-frame pass, and what the generator's conditioning is judged by.  Returns a dict: ``R`` and ``L``
    (F, J, 3, 3), ``P`` (F, J, 3) in the world frame, ``quat`` (F, J, 4), ``euler`` (F, J, 3), ``rigid`` (F, J, 3) in the input's frame,
    ``resid`` (F,), ``flags`` (F,), all fp64 / int; ``rest``; ``min_1pd``, ``min_reach`` (the least |x_c - P[j]| over the bone's rest
    length) and ``frame_angles`` (degrees between every frame-defining pair of vectors)."""
    sign = np.asarray(sign, dtype=np.float64)
    xw = np.asarray(x, dtype=np.float64) * sign
    f, joints, _ = xw.shape
    if rest is None:
        rest = rest_offsets(x, seq_start, edges, frames, rest_dirs, sign)
    root, parent, children = topology(edges, joints)
    framed = {int(fr[0]): tuple(int(v) for v in fr[1:]) for fr in frames}
    order = [root] + [int(c) for _, c in edges]
    row_seq = np.repeat(np.arange(len(seq_start) - 1), np.diff(np.asarray(seq_start)))
    out = dict(R=np.zeros((f, joints, 3, 3)), L=np.zeros((f, joints, 3, 3)), P=np.zeros((f, joints, 3)), quat=np.zeros((f, joints, 4)),
               euler=np.zeros((f, joints, 3)), resid=np.zeros(f), flags=np.zeros(f, dtype=np.int32), rest=rest)
    min_1pd, min_reach, angles = np.inf, np.inf, []
    for r in range(f):
        off = rest[row_seq[r]]
        rot, pos, flag = {}, {}, 0
        for j in order:
            rp = np.eye(3) if j == root else rot[parent[j]]
            pos[j] = xw[r, root].copy() if j == root else pos[parent[j]] + rp @ off[j]
            rj = rp
            if j in framed:
                m = frame_of(xw[r], framed[j])
                if m is None:
                    flag |= 1
                else:
                    rj = m
                    a0, a1, b0, b1 = framed[j]
                    e, g = xw[r, a1] - xw[r, a0], xw[r, b1] - xw[r, b0]
                    angles.append(np.degrees(np.arccos(np.clip(e @ g / (norm3(e) * norm3(g)), -1.0, 1.0))))
            elif len(children[j]) == 1:
                c = children[j][0]
                u = rp @ np.asarray(rest_dirs[c], dtype=np.float64)
                v = xw[r, c] - pos[j]
                n = norm3(v)
                if n == 0.0:
                    flag |= 2
                else:
                    if norm3(off[c]) > 0.0:
                        min_reach = min(min_reach, n / norm3(off[c]))
                    v = v / n
                    d = float(u @ v)
                    min_1pd = min(min_1pd, 1.0 + d)
                    if 1.0 + d <= 1e-8:
                        flag |= 4
                        a = cross(u, np.eye(3)[int(np.argmin(np.abs(u)))])         # argmin: the lowest index on a tie
                        a = a / norm3(a)
                        rj = (2.0 * np.outer(a, a) - np.eye(3)) @ rp
                    else:
                        k = skew(cross(u, v))
                        rj = (np.eye(3) + k + (k @ k) / (1.0 + d)) @ rp
            rot[j] = rj
            loc = rj if j == root else rp.T @ rj
            out["R"][r, j], out["L"][r, j], out["P"][r, j] = rj, loc, pos[j]
            out["quat"][r, j], out["euler"][r, j] = quat_of(loc), euler_zxy_deg(loc)
        out["resid"][r] = sum(norm3(out["P"][r, j] - xw[r, j]) for j in range(joints)) / joints
        out["flags"][r] = flag
    out["rigid"] = out["P"] * sign
    out.update(min_1pd=min_1pd, min_reach=min_reach, frame_angles=np.array(angles))
    return out


# ---- the generator: an articulated figure, exactly rigid, in camera coordinates ----
TPOSE17 = np.array([[0, 0, 0], [-0.13, 0, 0], [0, -0.45, 0], [0, -0.45, 0], [0.13, 0, 0], [0, -0.45, 0], [0, -0.45, 0], [0, 0.24, 0], [0, 0.26, 0],
                    [0, 0.11, 0], [0, 0.12, 0], [0.17, -0.03, 0], [0.28, 0, 0], [0.25, 0, 0], [-0.17, -0.03, 0], [-0.28, 0, 0], [-0.25, 0, 0]],
                   dtype=np.float64)                                               # world-frame offsets from the parent, metres


def rodrigues(w):
    t = norm3(w)
    if t == 0.0:
        return np.eye(3)
    k = skew(np.asarray(w) / t)
    return np.eye(3) + np.sin(t) * k + (1.0 - np.cos(t)) * (k @ k)


def articulated(seed, lengths, edges=EDGES17, tpose=TPOSE17, sign=SIGN_H36M, noise=0.0, sigma=0.6, dtype=np.float32):
    """Sequences of ``lengths`` rows: per sequence the T-pose offsets scaled by a factor in [0.9, 1.1], per frame a random root position
    near z = 5 m and a local rotation per joint whose rotation vector is normal with ``sigma`` rad per axis; forward kinematics gives
    exactly rigid positions, iid normal noise of ``noise`` metres is added, and the result is cast to fp32 in the input's (camera)
    frame (``dtype=np.float64`` keeps them exactly rigid).  Returns ``(x (F, J, 3) fp32, seq_start (S+1,) int32, offsets (S, J, 3) world)``."""
    rng = np.random.default_rng(seed)
    joints = tpose.shape[0]
    root, parent, _ = topology(edges, joints)
    xs, offs = [], []
    for n in lengths:
        off = tpose * rng.uniform(0.9, 1.1)
        offs.append(off)
        for _ in range(n):
            rot, pos = {}, {}
            loc = rng.normal(0.0, sigma, size=(joints, 3))
            for j in [root] + [int(c) for _, c in edges]:
                if j == root:
                    rot[j], pos[j] = rodrigues(loc[j]), rng.normal(0.0, 0.3, size=3) + (0.0, 0.0, -5.0)
                else:
                    rot[j], pos[j] = rot[parent[j]] @ rodrigues(loc[j]), pos[parent[j]] + rot[parent[j]] @ off[j]
            p = np.stack([pos[j] for j in range(joints)])
            xs.append(p + rng.normal(0.0, noise, size=p.shape) if noise > 0.0 else p)
    x = (np.stack(xs) * np.asarray(sign)).astype(dtype)
    return x, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), np.stack(offs)


def chain(joints):
    """A chain skeleton without a framed joint: edges (i, i + 1), every rest direction +y."""
    d = np.zeros((joints, 3))
    d[:, 1] = 1.0
    return tuple((i, i + 1) for i in range(joints - 1)), (), d, np.concatenate([np.zeros((1, 3)), np.tile([0.0, 0.1, 0.0], (joints - 1, 1))])


def assert_conditioned(ref):
    """The generator's own conditioning, judged on the oracle's side: what the fp64 part of every bar is derived from."""
    ang = ref["frame_angles"]
    assert ang.size == 0 or (ang.min() >= 45.0 and ang.max() <= 135.0), f"a frame-defining pair at {ang.min():.1f} / {ang.max():.1f} degrees"
    assert ref["min_1pd"] >= 0.1, f"an aim with 1 + d = {ref['min_1pd']:.3g}"
    assert ref["min_reach"] >= 0.5, f"|x_c - P[j]| down to {ref['min_reach']:.3g} of the bone's rest length"
    assert not ref["flags"].any()
