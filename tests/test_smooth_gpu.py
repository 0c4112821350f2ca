"""Smoothing and constant bone lengths of stitched sequences on the MI355X: the four ops of
include/r50_smooth.h against the numpy fp64 restatement of tests/smooth_reference.py, their exact properties (copied rows, isolation of
segments, causality, root bits), ``evaluate_dense(post=...)`` on a synthetic store, and the two command lines.

Bounds.  The FIR and the One-Euro filter accumulate in fp64 and round once, as the restatement does, so device and restatement differ
by fp64 rounding noise (about 1e-16 relative) before the one rounding to fp32: at most 1 fp32 ulp apart (the noise can move a value
across a rounding boundary, no further).  The One-Euro recurrence is a contraction -- xhat moves a fraction alpha in (0, 1] of the way
to x_t, dxhat likewise -- so a difference in fp64 does not grow along a segment and the same bound holds at every row.  The rebuild walks
at most J - 1 edges in fp64 from a root that is copied: the same argument."""
import math

import numpy as np
import pytest
import torch

from tests import smooth_reference as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGES17 = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14), (14, 15),
           (15, 16))
EDGES5 = ((0, 1), (1, 2), (0, 3), (3, 4))
EDGES = {17: EDGES17, 5: EDGES5}
BLOCK = 64                                                                      # rows per workgroup of the FIR kernel


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def layout(w):
    """(seq_start, idx) with segments of 1, W-1, W, W+1 and 3W+1 rows, a sequence with a gap in idx, a segment that ends exactly on a
    64-row block boundary, one that straddles a boundary, and a one-row sequence at the very end."""
    lens = [1] + ([w - 1] if w > 1 else []) + [w, w + 1, 3 * w + 1, 2 * w + 5]
    gap_seq, gap_at = len(lens) - 1, w + 2                                       # segments of W+2 and W+3 rows
    fill = (-sum(lens)) % BLOCK
    lens += [fill] if fill else []                                               # ends on a multiple of 64
    assert sum(lens) % BLOCK == 0
    lens += [BLOCK + 7, 1]                                                       # starts on the boundary and straddles the next one
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.arange(10, 10 + n) for n in lens]).astype(np.int32)
    idx[seq_start[gap_seq] + gap_at:seq_start[gap_seq + 1]] += 4
    return seq_start, idx


def poses(f, j, seed):
    """Camera-space metres: a body of about 0.3 m spread at z = 5."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((f, j, 3), generator=g) * 0.3 + torch.tensor([0.0, 0.0, 5.0])).numpy()


def tables(seq_start, idx):
    from implementation_phd_lab_vision_amd import smooth
    return smooth.DeviceTables(seq_start, idx, DEV)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_fir(x, seq_start, idx, coef):
    from implementation_phd_lab_vision_amd import smooth
    out, short = smooth.fir_sequences(dev(x), tables(seq_start, idx), smooth.upload_coef(coef, DEV))
    return out.cpu().numpy(), short.cpu().numpy()


# ----------------------------------------------------------------- FIR ------------------------------------------------------------------
@pytest.mark.parametrize("j", [17, 5])
@pytest.mark.parametrize("w", [1, 3, 9, 63])
def test_fir_against_the_restatement(lib, w, j):
    from implementation_phd_lab_vision_amd import smooth
    seq_start, idx = layout(w)
    f = int(seq_start[-1])
    assert f <= 600
    x = poses(f, j, 10 * w + j)
    coef = smooth.savgol_table(w, min(2, w - 1)) if w in (1, 3) else smooth.gauss_table((w - 1) / 6.0)
    assert coef.shape == (w, w)
    want, want_short = SR.fir(x, seq_start, idx, coef)
    got, short = run_fir(x, seq_start, idx, coef)
    again, short_again = run_fir(x, seq_start, idx, coef)
    assert np.array_equal(bits(got), bits(again)) and np.array_equal(short, short_again), "two runs differ"
    segs = SR.segments(seq_start, idx)
    lens = sorted(b - a for a, b in segs)
    assert {1, w, w + 1, 3 * w + 1} <= set(lens) and (w == 1 or w - 1 in lens)
    assert any(a % BLOCK == 0 and b - a > BLOCK for a, b in segs) and any(b % BLOCK == 0 and a % BLOCK for a, b in segs)
    assert len(segs) > len(seq_start) - 1, "no gap in idx"
    ulps = SR.ulp_distance(got, want)
    print(f"fir W={w} J={j}: F={f}, max ulp distance {int(ulps.max())}, rows differing {int((ulps.reshape(f, -1).max(1) > 0).sum())}")
    assert int(ulps.max()) <= 1
    n_short = 0
    for a, b in segs:
        if b - a < w:
            assert np.array_equal(bits(got[a:b]), bits(x[a:b])), f"short segment [{a}, {b}) was not copied"
            n_short += 1
    assert short.tolist() == [want_short, n_short]
    if w == 1:
        assert np.array_equal(bits(got), bits(x)) and short.tolist() == [0, 0]


@pytest.mark.parametrize("kind", ["gauss", "savgol"])
def test_fir_constant_segment_and_isolation(lib, kind):
    from implementation_phd_lab_vision_amd import smooth
    coef = smooth.gauss_table(1.5) if kind == "gauss" else smooth.savgol_table(9, 2)
    w = coef.shape[0]
    lens = [3 * w, 2 * w + 3, 3 * w + 1]
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.arange(n) for n in lens]).astype(np.int32)
    x = poses(int(seq_start[-1]), 17, 5)
    x[seq_start[1]:seq_start[2]] = x[seq_start[1]]                                # the middle segment: one pose held still
    got, _ = run_fir(x, seq_start, idx, coef)
    mid = slice(int(seq_start[1]), int(seq_start[2]))
    assert np.array_equal(bits(got[mid]), bits(x[mid])), "a constant segment must come back bit for bit"
    hostile = x.copy()
    hostile[mid] = 1e30
    got_h, _ = run_fir(hostile, seq_start, idx, coef)
    for s in (slice(0, mid.start), slice(mid.stop, None)):
        assert np.array_equal(bits(got_h[s]), bits(got[s])), "a neighbouring segment leaked into this one"
    assert np.all(np.isfinite(got_h)) and np.all(got_h[mid] > 9e29)


def test_fir_savgol_reproduces_a_sampled_quadratic_at_every_row(lib):
    from implementation_phd_lab_vision_amd import smooth
    w, j = 9, 5
    coef = smooth.savgol_table(w, 2)
    lens = [w, w + 1, 70]
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.arange(n) for n in lens]).astype(np.int32)
    rng = np.random.default_rng(4)
    a, b, c = rng.uniform(-1, 1, (j, 3)) + np.array([0, 0, 5.0]), rng.uniform(-0.05, 0.05, (j, 3)), rng.uniform(-2e-3, 2e-3, (j, 3))
    t = np.concatenate([np.arange(n) for n in lens]).astype(np.float64)[:, None, None]
    exact = a + b * t + c * t * t                                                # fp64: the analytic values
    x = exact.astype(np.float32)
    got, short = run_fir(x, seq_start, idx, coef)
    assert short.tolist() == [0, 0]
    # each input is off by at most half an fp32 spacing at its magnitude, the filter passes that on times sum_k |coef[e][k]|, the
    # store adds half a spacing; a degree-2 fit reproduces the quadratic itself up to the table's own 1e-10 (tests/test_smooth_cpu.py)
    top = float(np.abs(exact).max())
    half = 0.5 * float(np.spacing(np.float32(top)))
    gain = float(np.abs(coef).sum(axis=1).max())
    tol = gain * half + half + 3e-10 * top
    err = np.abs(got.astype(np.float64) - exact)
    print(f"savgol quadratic: max error {err.max():.3e} m, tolerance {tol:.3e} m (sum |coef| up to {gain:.3f})")
    assert err.max() <= tol
    assert err[[0, w - 1, w, 2 * w, 2 * w + 1, -1]].max() <= tol                  # the edge rows of every segment by name


# -------------------------------------------------------------- One-Euro ----------------------------------------------------------------
def run_euro(x, seq_start, idx, **kw):
    from implementation_phd_lab_vision_amd import smooth
    return smooth.one_euro_sequences(dev(x), tables(seq_start, idx), **kw).cpu().numpy()


@pytest.mark.parametrize("j", [17, 5, 33])
@pytest.mark.parametrize("params", [dict(rate=25.0, min_cutoff=1.0, beta=0.0, d_cutoff=1.0), dict(rate=50.0, min_cutoff=0.5, beta=0.7, d_cutoff=2.0)],
                         ids=["defaults", "beta0.7"])
def test_one_euro_against_the_restatement(lib, params, j):
    seq_start, idx = layout(9)
    f = int(seq_start[-1])
    x = poses(f, j, 3 + j)
    want = SR.one_euro(x, seq_start, idx, **params)
    got = run_euro(x, seq_start, idx, **params)
    assert np.array_equal(bits(got), bits(run_euro(x, seq_start, idx, **params))), "two runs differ"
    ulps = SR.ulp_distance(got, want)
    print(f"one_euro J={j} {params}: max ulp distance {int(ulps.max())}")
    assert int(ulps.max()) <= 1
    segs = SR.segments(seq_start, idx)
    firsts = [a for a, _ in segs]
    assert np.array_equal(bits(got[firsts]), bits(x[firsts])), "a segment's first row must pass through"
    assert not np.array_equal(got, x)

    # causality: a change at row r leaves every earlier row, and every other segment, as it was
    a, b = max(segs, key=lambda s: s[1] - s[0])
    r = a + (b - a) // 2
    changed = x.copy()
    changed[r] += 0.25
    got_c = run_euro(changed, seq_start, idx, **params)
    assert np.array_equal(bits(got_c[:r]), bits(got[:r])) and np.array_equal(bits(got_c[b:]), bits(got[b:]))
    assert np.all(got_c[r] != got[r]) and np.any(got_c[b - 1] != got[b - 1])


def test_one_euro_returns_a_constant_segment(lib):
    seq_start, idx = np.array([0, 40, 41, 90], dtype=np.int32), np.concatenate([np.arange(40), [0], np.arange(49)]).astype(np.int32)
    x = poses(90, 17, 9)
    x[:40] = x[0]
    got = run_euro(x, seq_start, idx, beta=0.0)
    assert np.array_equal(bits(got[:41]), bits(x[:41]))
    assert not np.array_equal(got[41:], x[41:])


# ---------------------------------------------------------------- bones -----------------------------------------------------------------
def rigid(f, j, scale, seed):
    """A skeleton of fixed bone lengths turning slowly about the vertical and drifting, in fp64 metres around z = 5."""
    rng = np.random.default_rng(seed)
    rest = rng.uniform(-0.4, 0.4, (j, 3)) * scale
    ang = 0.02 * np.arange(f) + rng.uniform(0, 1)
    rot = np.stack([np.stack([np.cos(ang), np.zeros(f), np.sin(ang)], -1), np.tile([0.0, 1.0, 0.0], (f, 1)),
                    np.stack([-np.sin(ang), np.zeros(f), np.cos(ang)], -1)], -2)
    return np.einsum("fab,jb->fja", rot, rest) + np.array([0.0, 0.0, 5.0]) + 0.003 * np.arange(f)[:, None, None]


@pytest.mark.parametrize("j", [17, 5, 33])
def test_bone_stats_and_rebuild(lib, j):
    from implementation_phd_lab_vision_amd import smooth
    edges = EDGES.get(j) or tuple((i, i + 1) for i in range(j - 1))
    lens = [1, 300, 37, 64, 2]                                                  # one row; more rows than threads; a 64-row block exactly
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    f = int(seq_start[-1])
    idx = np.concatenate([np.arange(n) for n in lens]).astype(np.int32)
    rng = np.random.default_rng(j)
    # two adjacent sequences of different limb lengths (1.0 and 1.3), every pose jittered by 5 mm
    x64 = np.concatenate([rigid(n, j, 1.0 + 0.3 * (s % 2), s) for s, n in enumerate(lens)]) + rng.normal(0, 0.005, (f, j, 3))
    x = x64.astype(np.float32)
    pa0, ch0 = edges[1]
    x[5, ch0] = x[5, pa0]                                                        # a bone of length exactly 0
    assert float(np.abs(x).max()) < 8.0
    t = tables(seq_start, idx)
    stats = smooth.bone_stats(dev(x), t, edges)
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), smooth.bone_stats(dev(x), t, edges).cpu().numpy().view(np.uint64))
    got_stats = stats.cpu().numpy()
    want_stats = SR.bone_stats(x, seq_start, edges)
    assert got_stats.shape == (len(lens), len(edges), 2)
    rel = np.abs(got_stats - want_stats) / np.maximum(np.abs(want_stats), 1e-300)
    print(f"bone_stats J={j}: max rel error of the mean {rel[..., 0].max():.2e}, of the squared deviations {rel[..., 1].max():.2e}")
    assert rel[..., 0].max() <= 1e-12
    assert rel[..., 1].max() <= 1e-12
    assert np.all(got_stats[0, :, 1] == 0.0), "a sequence of one row has no deviation"

    out, used = smooth.fix_bone_lengths(dev(x), t, edges)
    assert used.data_ptr() != stats.data_ptr() and np.array_equal(used.cpu().numpy().view(np.uint64), got_stats.view(np.uint64))
    again, _ = smooth.fix_bone_lengths(dev(x), t, edges, stats)
    got = out.cpu().numpy()
    assert np.array_equal(bits(got), bits(again.cpu().numpy())), "two runs differ"
    want = SR.bone_rebuild(x, seq_start, edges, want_stats)
    ulps = SR.ulp_distance(got, want)
    print(f"bone_rebuild J={j}: max ulp distance {int(ulps.max())}")
    assert int(ulps.max()) <= 1
    children = {c for _, c in edges}
    roots = [k for k in range(j) if k not in children]
    assert roots and np.array_equal(bits(got[:, roots]), bits(x[:, roots])), "a joint that is no edge's child keeps its bits"

    # every bone of every frame has its sequence's length.  child' and parent' are each stored within half an fp32 spacing per
    # coordinate of the fp64 chain (every |coordinate| < 8 m: spacing 2^-21 below 8), so each coordinate of the stored bone vector is off
    # by at most one spacing and the vector by sqrt(3) spacings; the fp64 chain itself adds nothing visible at that scale
    assert float(np.abs(got).max()) < 8.0
    bound = math.sqrt(3.0) * float(np.spacing(np.float32(4.0)))
    ln = SR.bone_lengths(got, edges)
    target = np.repeat(want_stats[:, :, 0], np.diff(seq_start), axis=0)
    zero = np.zeros_like(ln, dtype=bool)
    zero[5, 1] = True
    print(f"bone_rebuild J={j}: max |length - sequence mean| {np.abs(ln - target)[~zero].max():.3e} m, bound {bound:.3e} m")
    assert np.abs(ln - target)[~zero].max() <= bound
    e = np.asarray(edges)
    d_in = x[:, e[:, 1]].astype(np.float64) - x[:, e[:, 0]].astype(np.float64)
    d_out = got[:, e[:, 1]].astype(np.float64) - got[:, e[:, 0]].astype(np.float64)
    n_in = np.linalg.norm(d_in, axis=-1, keepdims=True)
    unit_gap = np.linalg.norm(d_out - target[..., None] * d_in / np.where(n_in > 0, n_in, 1.0), axis=-1)
    assert unit_gap[~zero].max() <= bound, "a bone's direction moved"
    # the zero-length bone keeps its offset: child' sits on parent'
    assert np.abs(d_out[5, 1]).max() <= float(np.spacing(np.float32(4.0)))
    # the two limb scales stay apart: sequence 1 (scale 1.3) and sequence 2 (scale 1.0) keep their own means
    m1, m2 = want_stats[1, :, 0], want_stats[2, :, 0]
    assert np.all(np.abs(m1 - m2) > 100 * bound)
    assert np.abs(ln[seq_start[2] - 1] - m1).max() <= bound and np.abs(ln[seq_start[2]] - m2).max() <= bound


# -------------------------------------------------------------- end to end --------------------------------------------------------------
T = 8
AMP = 0.004                                                                     # metres: the stand-in head's alternating error


class Store:
    """An in-memory stand-in for a DeviceFeatureStore: overlapping clips of rigid-skeleton videos.  ``get_batch`` hands the stand-in
    head its answer: the ground truth plus AMP * (-1)^frame along a fixed per-joint direction."""
    augment = False

    def __init__(self):
        self.videos = {("act0", 1): 60, ("act0_1", 2): 33, ("act1", 1): 41, ("act2 1", 1): 12}
        rng = np.random.default_rng(11)
        self.truth = {k: torch.from_numpy(rigid(n, 17, 1.0 + 0.1 * i, 20 + i).astype(np.float32)) for i, (k, n) in enumerate(self.videos.items())}
        self.pattern = torch.from_numpy(rng.standard_normal((17, 3)).astype(np.float32))
        self.pattern[0] = 0.0
        self.clips = [{"subject": 9, "action": a, "cam": c, "start": s, "end": s + T} for (a, c), n in self.videos.items()
                      for s in list(range(0, n - T + 1, 3)) + ([n - T] if (n - T) % 3 else [])]
        self.feats = torch.zeros(len(self.clips), T, 1)

    def __len__(self):
        return len(self.clips)

    def item_clips(self):
        return [dict(c) for c in self.clips]

    def get_batch(self, items):
        gt = torch.stack([self.truth[(self.clips[i]["action"], self.clips[i]["cam"])][self.clips[i]["start"]:self.clips[i]["end"]] for i in items])
        frame = torch.tensor([[self.clips[i]["start"] + t for t in range(T)] for i in items])
        sign = (1.0 - 2.0 * (frame % 2)).to(torch.float32)[:, :, None, None]
        return (gt + AMP * sign * self.pattern).to(DEV), gt.to(DEV)


class Head:
    joints_num, number_blocks, _device = 17, 2, torch.device(DEV)

    def joints(self, answer):
        return answer.clone()


@pytest.fixture(scope="module")
def dense(lib):
    """The raw pass, computed once and shared."""
    from implementation_phd_lab_vision_amd import sequences as sq
    store, head = Store(), Head()
    return store, head, sq.evaluate_dense(head, store, fuse="mean", keep_poses=True)


def same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def test_dense_without_post_is_what_it_was(dense):
    from implementation_phd_lab_vision_amd import sequences as sq
    store, head, raw = dense
    res = sq.evaluate_dense(head, store, fuse="mean", keep_poses=True, post=None)
    assert list(res) == list(raw) and not any(k.startswith(("post", "bone_std")) or k == "pred_post" for k in res)
    for k in raw:
        assert same(res[k], raw[k]), k


def test_dense_identity_filter_changes_nothing(dense):
    from implementation_phd_lab_vision_amd import sequences as sq, smooth
    store, head, raw = dense
    post = smooth.PostProcess(kind="savgol", window=1, degree=0)
    res = sq.evaluate_dense(head, store, fuse="mean", keep_poses=True, post=post)
    for k in raw:
        assert same(res[k], raw[k]), f"{k}: the raw results moved"
    for m in ("p1", "p2", "mpjve", "accel"):
        for suffix in ("", "_all", "_mean"):
            assert same(res["post_" + m + suffix], raw[m + suffix]), m + suffix
    assert np.array_equal(bits(res["pred_post"]), bits(raw["pred"])) and res["post_short_rows"] == 0
    assert same(res["bone_std_post"], res["bone_std_raw"]) and res["bone_std_post_all"] == res["bone_std_raw_all"]
    assert "causal" in res["post"] and "R=0" in res["post"]


def _accel_all(pred, raw, store):
    from implementation_phd_lab_vision_amd import protocols, sequences as sq
    from tests import stitch_reference as ref
    table = sq.SequenceTable.from_clips(store.item_clips(), T)
    names = raw["group_names"]
    group = np.array([names.index(protocols.action_name(table.seq_keys[s][1])) for s in table.seq], dtype=np.int32)
    sums = ref.metrics(pred, raw["gt"], raw["frame_spread"], table.offsets, table.seq, table.idx, group, len(names))
    return sums[:, 5].sum() / sums[:, 4].sum(), sums


@pytest.mark.parametrize("chunk_clips", [8192, 6])
def test_dense_gauss_lowers_the_acceleration_error_to_the_restatements(dense, chunk_clips):
    from implementation_phd_lab_vision_amd import sequences as sq, smooth
    store, head, raw = dense
    post = smooth.PostProcess(kind="gauss", sigma=1.0)
    res = sq.evaluate_dense(head, store, fuse="mean", keep_poses=True, post=post, chunk_clips=chunk_clips)
    assert chunk_clips > 100 or len(sq.SequenceTable.from_clips(store.item_clips(), T).chunks(chunk_clips)) > 1
    for k in raw:
        assert same(res[k], raw[k]) or k in ("p1", "p2", "mpjve", "accel", "spread", "position_p1", "position_p2") or k.endswith(("_all", "_mean")), k
    want_pred, want_short = SR.fir(raw["pred"], raw["seq_start"], raw["frame_idx"], SR.gauss_table(1.0))
    assert int(SR.ulp_distance(res["pred_post"], want_pred).max()) <= 1 and res["post_short_rows"] == want_short
    want, sums = _accel_all(want_pred, raw, store)
    print(f"dense gauss: accel_all raw {raw['accel_all'] * 1e3:.4f} -> post {res['post_accel_all'] * 1e3:.4f} mm/frame^2, restatement {want * 1e3:.4f}")
    assert res["post_accel_all"] == pytest.approx(want, rel=1e-6) and res["post_accel_all"] < 0.25 * raw["accel_all"]
    assert res["post_mpjve_all"] == pytest.approx(sums[:, 3].sum() / sums[:, 2].sum(), rel=1e-6)
    assert res["post_p1_all"] == pytest.approx(sums[:, 1].sum() / sums[:, 0].sum(), rel=1e-6)
    assert "not causal" in res["post"] and "R=3" in res["post"]


@pytest.mark.parametrize("chunk_clips", [8192, 6])
def test_dense_fix_bones_drives_the_bone_deviation_to_rounding(dense, chunk_clips):
    from implementation_phd_lab_vision_amd import sequences as sq, smooth
    store, head, raw = dense
    res = sq.evaluate_dense(head, store, fuse="mean", keep_poses=True, post=smooth.PostProcess(fix_bones=True), chunk_clips=chunk_clips)
    # a stored bone vector is within sqrt(3) fp32 spacings (at |coordinate| < 8 m) of its fp64 value, so every length is within that of
    # the sequence's mean and so is their standard deviation; in mm
    assert float(np.abs(res["pred_post"]).max()) < 8.0
    bound_mm = 1000.0 * math.sqrt(3.0) * float(np.spacing(np.float32(4.0)))
    want_raw = SR.bone_std_mm(raw["pred"], raw["seq_start"], EDGES17)
    print(f"dense fix-bones: bone std raw {res['bone_std_raw_all']:.4f} mm (restatement {want_raw:.4f}), post {res['bone_std_post_all']:.3e} mm, "
          f"gt {res['bone_std_gt_all']:.3e} mm, bound {bound_mm:.3e} mm")
    assert res["bone_std_raw_all"] == pytest.approx(want_raw, rel=1e-9) and want_raw > 1000 * bound_mm
    assert res["bone_std_post_all"] <= bound_mm and res["bone_std_gt_all"] <= bound_mm
    assert np.all(res["bone_std_post"] <= bound_mm) and res["bone_std_raw"].shape == (len(raw["group_names"]),)
    names = raw["group_names"]
    from implementation_phd_lab_vision_amd import protocols
    for g, name in enumerate(names):
        seqs = [s for s, k in enumerate(raw["seq_keys"]) if protocols.action_name(k[1]) == name]
        assert res["bone_std_raw"][g] == pytest.approx(SR.bone_std_mm(raw["pred"], raw["seq_start"], EDGES17, seqs), rel=1e-9), name
    want_post = SR.bone_rebuild(raw["pred"], raw["seq_start"], EDGES17, SR.bone_stats(raw["pred"], raw["seq_start"], EDGES17))
    assert int(SR.ulp_distance(res["pred_post"], want_post).max()) <= 1
    assert res["post_short_rows"] == 0 and "constant bone lengths" in res["post"]


def test_results_cli_with_the_flags(lib, tmp_path, capsys):
    from implementation_phd_lab_vision_amd import results
    from oracle import lifting_oracle as lo
    from tests import results_data as rd
    features = rd.make_results_cache(tmp_path / "features")
    videos = rd.make_preprocessed_tree(tmp_path / "videos")
    torch.save(lo.synthetic_head_state_dict(1024, 2, seed=2), tmp_path / "model.pt")
    base = ["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(tmp_path / "model.pt"), "--seq-len",
            str(rd.SEQ_LEN), "--batch-size", "4", "--save-n", "2", "--video-size", "32", "--video-reader", "tests.results_data:read_video",
            "--dense"]
    results.main(base + ["--out", str(tmp_path / "plain.npz"), "--dense-out", str(tmp_path / "plain_seq.npz")])
    plain_lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Dense |")]
    results.main(base + ["--out", str(tmp_path / "post.npz"), "--dense-out", str(tmp_path / "post_seq.npz"), "--dense-smooth", "gauss",
                         "--smooth-sigma", "0.6", "--dense-fix-bones"])
    post_lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Dense |")]
    assert not any("post" in l for l in plain_lines)
    extra = [l for l in post_lines if l.startswith("Dense | post")]
    assert len(extra) == 1 + 3 and "gauss sigma=0.6 W=5" in extra[0] and "not causal, look-ahead R=2" in extra[0] and "bone std (mm)" in extra[1]
    assert [l for l in post_lines if not l.startswith("Dense | post") and "saved to" not in l] == [l for l in plain_lines if "saved to" not in l]
    a, b = np.load(tmp_path / "plain.npz", allow_pickle=True), np.load(tmp_path / "post.npz", allow_pickle=True)
    new = set(b.files) - set(a.files)
    assert new == {"dense_post", "dense_post_short"} | {f"dense_post_{m}{s}" for m in ("p1", "p2", "mpjve", "accel") for s in ("", "_all")} | \
        {f"dense_post_bone_std_{k}{s}" for k in ("raw", "post", "gt") for s in ("", "_all")}
    for k in a.files:
        if k.startswith("dense_"):
            assert np.array_equal(a[k], b[k]), k
    assert float(b["dense_post_bone_std_post_all"]) < 1e-2 * float(b["dense_post_bone_std_raw_all"])
    sa, sb = np.load(tmp_path / "plain_seq.npz"), np.load(tmp_path / "post_seq.npz")
    assert set(sb.files) - set(sa.files) == {"pred_post", "post"}
    for k in sa.files:
        assert np.array_equal(sa[k], sb[k]), k
    # the file holds what the library gives on the raw poses of the file, bit for bit (the ops themselves are held to the restatement above)
    from implementation_phd_lab_vision_amd import smooth
    want, _ = smooth.PostProcess(kind="gauss", sigma=0.6, fix_bones=True).apply(dev(sa["pred"]), (sa["seq_start"], sa["frame_idx"]))
    assert np.array_equal(bits(sb["pred_post"]), bits(want.cpu().numpy())) and not np.array_equal(sb["pred_post"], sa["pred"])
    assert "gauss sigma=0.6" in str(sb["post"])


def test_predict_cli_with_the_flags(lib, tmp_path):
    from implementation_phd_lab_vision_amd import predict
    from oracle.lifting_oracle import synthetic_head_state_dict
    video = torch.randint(0, 256, (23, 64, 48, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    np.save(tmp_path / "walk.npy", video.numpy())
    torch.save(synthetic_head_state_dict(64, 2, seed=1), tmp_path / "head.pt")
    argv = ["--frames", str(tmp_path / "walk.npy"), "--model_path", str(tmp_path / "head.pt"), "--synthetic-weights", "--seq-len", "8", "--stride",
            "3", "--frame-batch", "16", "--pred-len", "3", "--input-len", "4"]
    plain = np.load(predict.main(argv + ["--out", str(tmp_path / "a")])[0])
    written = predict.main(argv + ["--out", str(tmp_path / "b"), "--smooth", "savgol", "--smooth-window", "5", "--fix-bones", "--render",
                                   "--render-frames", "4"])
    z = np.load(written[0])
    assert set(z.files) - set(plain.files) == {"joints3d_raw", "post", "post_short_rows"} and len(written) == 3
    for k in plain.files:
        assert np.array_equal(z["joints3d_raw" if k == "joints3d" else k], plain[k]), k      # the forecast included: left as it is
    assert "savgol W=5 degree=2" in str(z["post"]) and "constant bone lengths" in str(z["post"]) and int(z["post_short_rows"]) == 0
    n = plain["joints3d"].shape[0]
    from implementation_phd_lab_vision_amd import smooth
    want, _ = smooth.PostProcess(kind="savgol", window=5, fix_bones=True).apply(dev(plain["joints3d"]), (np.array([0, n]), np.arange(n)))
    assert z["joints3d"].shape == (n, 17, 3) and not np.array_equal(z["joints3d"], plain["joints3d"])
    assert np.array_equal(bits(z["joints3d"]), bits(want.cpu().numpy()))          # one sequence, one segment, the library's own bits
    from tests import png_reader
    anim, info = png_reader.decode(written[1])
    assert info["animated"] and anim.shape[0] == 4 + 3                            # 4 frames with the processed poses, then the forecast
