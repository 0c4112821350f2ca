"""The 2D-guided refinement of INTEGRATION.md section Z restated in plain numpy fp64, and the synthetic data of its tests.

Written from the definition, not from the kernels: whole-array operations, the second-difference term as D^T D X over the valid stencil
centres, the bone term scattered edge by edge onto both endpoints, the 3x3 systems by ``np.linalg.solve``.  The kernels gather per
(row, joint) and factorise L D L^T; the two agree to fp64 rounding, which the tests' bars are derived from."""
import numpy as np

EDGES17 = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14), (14, 15),
           (15, 16))
DEFAULTS = dict(l2d=1.0, l3d=1.0, lacc=1.0, lbone=0.0, omega=0.6, z_min=0.1)
FOCAL = 1150.0               # pixels: the focal length of the synthetic camera (Human3.6M's are 1145 .. 1150)


def chain_edges(joints):
    return tuple((k, k + 1) for k in range(joints - 1))


def row_tables(seq_start, idx):
    """(row_seq (F,), row_seg (F,)) of the ragged table: a segment ends at a sequence end or where idx does not go on by one."""
    seq_start, idx = np.asarray(seq_start, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    row_seq = np.repeat(np.arange(len(seq_start) - 1), np.diff(seq_start))
    new = np.ones(idx.size, dtype=bool)
    new[1:] = (row_seq[1:] != row_seq[:-1]) | (idx[1:] != idx[:-1] + 1)
    return row_seq, np.cumsum(new) - 1


def _centres(row_seg):
    """v[c] = 1 where rows c-1, c, c+1 exist and lie in one segment."""
    f = row_seg.size
    v = np.zeros(f)
    if f >= 3:
        v[1:-1] = (row_seg[:-2] == row_seg[1:-1]) & (row_seg[2:] == row_seg[1:-1])
    return v


def second_differences(x, row_seg):
    """a[c] = X[c-1] - 2 X[c] + X[c+1] at the valid centres, 0 elsewhere; and the mask."""
    v = _centres(row_seg)
    a = np.zeros_like(x)
    a[1:-1] = x[:-2] - 2.0 * x[1:-1] + x[2:]
    return a * v[:, None, None], v


def bone_lengths(x, seq_start, edges):
    """(S, E): the mean length of every bone over every sequence's rows."""
    e = np.asarray(edges)
    length = np.linalg.norm(x[:, e[:, 1]].astype(np.float64) - x[:, e[:, 0]].astype(np.float64), axis=2)
    return np.stack([length[a:b].mean(axis=0) for a, b in zip(seq_start[:-1], seq_start[1:])])


def sweep(x, x0, rays, conf, row_seq, row_seg, edges, bone_len, l2d, l3d, lacc, lbone, omega, z_min):
    """One damped block-Jacobi Gauss-Newton step from the iterate x (F, J, 3) fp64."""
    f, joints, _ = x.shape
    p0 = x0.astype(np.float64)
    z0 = np.maximum(p0[..., 2], z_min)
    g = np.zeros((f, joints, 3))
    h = np.zeros((f, joints, 3, 3))
    w = l2d * (np.ones((f, joints)) if conf is None else conf.astype(np.float64))
    on = (w != 0.0) & (x[..., 2] >= z_min)
    pz = np.where(on, x[..., 2], 1.0)
    q = x[..., :2] / pz[..., None]
    r = z0[..., None] * (q - rays.astype(np.float64))
    jac = np.zeros((f, joints, 2, 3))
    jac[..., 0, 0] = jac[..., 1, 1] = 1.0
    jac[..., 0, 2], jac[..., 1, 2] = -q[..., 0], -q[..., 1]
    jac *= (z0 / pz)[..., None, None]
    wm = np.where(on, w, 0.0)
    g += wm[..., None] * np.einsum("fjab,fja->fjb", jac, r)
    h += wm[..., None, None] * np.einsum("fjab,fjac->fjbc", jac, jac)
    g += l3d * (x - p0)
    h += l3d * np.eye(3)
    if lacc != 0.0:
        a, v = second_differences(x, row_seg)
        ap = np.concatenate([np.zeros((1, joints, 3)), a, np.zeros((1, joints, 3))])
        vp = np.concatenate([[0.0], v, [0.0]])
        g += lacc * (ap[:-2] - 2.0 * ap[1:-1] + ap[2:])                           # D^T (D X): row t sees the centres t-1, t, t+1
        h += lacc * (vp[:-2] + 4.0 * vp[1:-1] + vp[2:])[:, None, None, None] * np.eye(3)
    if lbone != 0.0:
        for e, (pa, ch) in enumerate(edges):
            d = x[:, ch] - x[:, pa]
            length = np.linalg.norm(d, axis=1)
            ok = length > 0.0
            u = d / np.where(ok, length, 1.0)[:, None] * ok[:, None]
            m = (length - bone_len[row_seq, e]) * ok
            uu = u[:, :, None] * u[:, None, :]
            g[:, ch] += lbone * m[:, None] * u
            g[:, pa] -= lbone * m[:, None] * u
            h[:, ch] += lbone * uu
            h[:, pa] += lbone * uu
    return x - omega * np.linalg.solve(h, g[..., None])[..., 0]


def refine(x0, rays, conf, seq_start, idx, edges=(), bone_len=None, iters=50, trace=None, **kw):
    """``iters`` sweeps from x0 (F, J, 3) fp32; returns the fp64 iterate.  ``trace`` (a list) receives every iterate, the first included."""
    p = dict(DEFAULTS, **kw)
    row_seq, row_seg = row_tables(seq_start, idx)
    x = x0.astype(np.float64)
    if trace is not None:
        trace.append(x)
    for _ in range(iters):
        x = sweep(x, x0, rays, conf, row_seq, row_seg, edges, bone_len, p["l2d"], p["l3d"], p["lacc"], p["lbone"], p["omega"], p["z_min"])
        if trace is not None:
            trace.append(x)
    return x


def energy(x, x0, rays, conf, seq_start, idx, edges=(), bone_len=None, z_min=0.1):
    """(S, 6) fp64 per sequence: [e2d, e3d, eacc, ebone, sum of conf over the included (t, j), (t, j) skipped for X_z < z_min]."""
    x, p0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    f, joints, _ = x.shape
    row_seq, row_seg = row_tables(seq_start, idx)
    z0 = np.maximum(p0[..., 2], z_min)
    cf = np.ones((f, joints)) if conf is None else conf.astype(np.float64)
    on = x[..., 2] >= z_min
    pz = np.where(on, x[..., 2], 1.0)
    r = z0[..., None] * (x[..., :2] / pz[..., None] - rays.astype(np.float64))
    rows = np.zeros((f, 6))
    rows[:, 0] = (cf * (r * r).sum(axis=2) * on).sum(axis=1)
    rows[:, 4] = (cf * on).sum(axis=1)
    rows[:, 5] = (~on).sum(axis=1)
    rows[:, 1] = ((x - p0) ** 2).sum(axis=(1, 2))
    a, _ = second_differences(x, row_seg)
    rows[:, 2] = (a * a).sum(axis=(1, 2))
    if bone_len is not None:
        e = np.asarray(edges)
        length = np.linalg.norm(x[:, e[:, 1]] - x[:, e[:, 0]], axis=2)
        rows[:, 3] = (((length - bone_len[row_seq]) ** 2) * (length > 0.0)).sum(axis=1)
    return np.stack([rows[a0:b0].sum(axis=0) for a0, b0 in zip(seq_start[:-1], seq_start[1:])])


def total(en, l2d=1.0, l3d=1.0, lacc=1.0, lbone=0.0, **_):
    """The weighted energy over all sequences from the (S, 6) terms."""
    s = np.asarray(en).sum(axis=0)
    return l2d * s[0] + l3d * s[1] + lacc * s[2] + lbone * s[3]


# ---- data --------------------------------------------------------------------------------------------------------------------------------
def figure_motion(rng, rows, joints, depth=5.0):
    """(rows, joints, 3) fp64: a figure of about half a metre that sways smoothly, ``depth`` metres in front of the camera."""
    if joints == 17:
        body = rng.standard_normal((joints, 3)) * 0.25
    else:                                                                          # a chain: a random walk of 0.1 m steps
        body = np.cumsum(rng.standard_normal((joints, 3)) * 0.06, axis=0)
        body -= body.mean(axis=0)
    t = np.arange(rows)[:, None, None]
    sway = 0.05 * np.sin(0.11 * t + rng.uniform(0.0, 6.28, (joints, 3))) + 0.1 * np.sin(0.031 * t + rng.uniform(0.0, 6.28, (1, 3)))
    return body + sway + np.array([0.0, 0.0, depth])


def project(x):
    """Rays of the poses x (..., 3): x_xy / x_z."""
    x = np.asarray(x, dtype=np.float64)
    return x[..., :2] / x[..., 2:3]


def prototype_sequence(seed=0, rows=300, joints=17, offset=0.03, jitter=0.02, noise_px=0.0):
    """The issue's synthetic sequence: one sequence of ``rows`` rows in two segments (a gap in the frame index in the middle), 5 m from
    the camera; the prediction is the ground truth plus a constant offset of ``offset`` metres per joint plus ``jitter`` metres of white
    noise; the rays are the ground truth's projection plus ``noise_px`` pixels at FOCAL.  Returns a dict of fp32 / int32 arrays and the
    fp64 ground truth."""
    rng = np.random.default_rng(seed)
    gt = figure_motion(rng, rows, joints)
    direction = rng.standard_normal((joints, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    x0 = gt + offset * direction + jitter * rng.standard_normal(gt.shape) / np.sqrt(3.0)
    rays = project(gt) + noise_px * rng.standard_normal((rows, joints, 2)) / FOCAL
    half = rows // 2
    idx = np.concatenate([np.arange(half), np.arange(half, rows) + 7]).astype(np.int32)
    return dict(gt=gt, x0=x0.astype(np.float32), rays=rays.astype(np.float32), seq_start=np.array([0, rows], dtype=np.int32), idx=idx)


CACHE_SEQ_LEN, CACHE_STRIDE = 8, 4
CACHE_VIDEOS = {("act0", 1): 20, ("act0", 2): 16, ("act1 1", 1): 12}              # (action, cam) -> frames; clips start every CACHE_STRIDE


def make_projected_cache(root, seed=0):
    """index.pt + shards under ``root`` (the project's shard packer): the clips of CACHE_VIDEOS for S9, joints3d in millimetres as the
    shards hold them, and ``joints2d`` = the projection of ``joints3d`` through the clip's ``K``.  Every clip has a crop box of its own, so
    its ``K`` (focal lengths of 1000 .. 1200 px of the crop, the principal point moved with the box) and its pixels differ from those of
    the other clips that show the same frame; the rays do not."""
    import torch
    from pathlib import Path
    from implementation_phd_lab_vision_amd.shards import ShardPacker
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    packer = ShardPacker(root, n_vars=1, shard_size=4, shuffle_pool=3, shuffle_seed=seed)
    for (action, cam), n in CACHE_VIDEOS.items():
        pose = torch.from_numpy((figure_motion(rng, n, 17) * 1000.0).astype(np.float32))
        for start in range(0, n - CACHE_SEQ_LEN + 1, CACHE_STRIDE):
            k = torch.eye(3)
            k[0, 0] = k[1, 1] = float(rng.uniform(1000.0, 1200.0))
            k[0, 2], k[1, 2] = float(rng.uniform(100.0, 124.0)), float(rng.uniform(100.0, 124.0))
            x = pose[start:start + CACHE_SEQ_LEN].numpy().astype(np.float64)
            kk = k.numpy().astype(np.float64)
            uv = project(x) * [kk[0, 0], kk[1, 1]] + [kk[0, 2], kk[1, 2]]
            packer.add_group([{"feat": torch.randn(CACHE_SEQ_LEN, 2048, generator=g).abs(), "joints3d": pose[start:start + CACHE_SEQ_LEN].clone(),
                               "joints2d": torch.from_numpy(uv.astype(np.float32)), "K": k,
                               "meta": {"subject": 9, "action": action, "cam": cam, "start": start, "end": start + CACHE_SEQ_LEN, "aug": "orig",
                                        "box": None}}])
    packer.finish()
    packer.write_index(seq_len=CACHE_SEQ_LEN, frame_skip=2, save_fp16=False, augment=False)
    return Path(root)


SEGMENTS = ((1,), (2,), (3, 4, 5), (63,), (64, 65), (130,))    # the sequences of the ragged table, each a tuple of segment lengths


def ragged_case(seed, joints, with_conf, behind=True):
    """337 rows in six sequences whose segments have 1, 2, 3, 4, 5, 63, 64, 65 and 130 rows (sequences three and five have gaps in their
    frame index).  The prediction is the ground truth plus 30 mm per joint plus 20 mm of jitter; with ``behind`` a few joints of it are
    closer than z_min = 0.1 or behind the camera.  ``conf`` (if asked for) is uniform in [0.2, 1] with every seventh value 0.
    ``bone_len`` holds the GROUND TRUTH's mean bone lengths, so no term of the bone energy is rounding noise."""
    rng = np.random.default_rng(seed)
    lens = [sum(s) for s in SEGMENTS]
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = []
    for segs in SEGMENTS:
        at = 0
        for n in segs:
            idx.append(at + np.arange(n))
            at += n + 3                                                             # a gap of three frames between a sequence's segments
    idx = np.concatenate(idx).astype(np.int32)
    rows = int(seq_start[-1])
    gt = figure_motion(rng, rows, joints)
    direction = rng.standard_normal((joints, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    x0 = gt + 0.03 * direction + 0.02 * rng.standard_normal(gt.shape) / np.sqrt(3.0)
    if behind:
        pick = rng.choice(rows * joints, size=12, replace=False)
        x0.reshape(-1, 3)[pick[:6], 2] = 0.05
        x0.reshape(-1, 3)[pick[6:], 2] = -0.4
    conf = None
    if with_conf:
        conf = rng.uniform(0.2, 1.0, (rows, joints))
        conf.reshape(-1)[::7] = 0.0
        conf = conf.astype(np.float32)
    edges = EDGES17 if joints == 17 else chain_edges(joints)
    return dict(gt=gt, x0=x0.astype(np.float32), rays=project(gt).astype(np.float32), conf=conf, seq_start=seq_start, idx=idx, edges=edges,
                bone_len=bone_lengths(gt, seq_start, edges))
