"""Smoothing and bone lengths of stitched sequences without a GPU: the third public header
include/r50_smooth.h is bound, exported and guard-banded; every refusal of its ops returns before any launch; the host tables
(``segment_table``, ``gauss_table``, ``savgol_table``), the edge check and the parsers; and the numpy restatement the GPU tests lean on."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import smooth_reference as SR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "r50_smooth.h"
OPS = {"r50_op_fir_sequences", "r50_op_one_euro_sequences", "r50_op_bone_stats", "r50_op_bone_rebuild"}
EDGES5 = ((0, 1), (1, 2), (0, 3), (3, 4))


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = re.findall(r"^\s*(?:int|int64_t|size_t)\s+(r50_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    assert protos, "no prototypes parsed from include/r50_smooth.h"
    return [(name, len([a for a in args.split(",") if a.strip()])) for name, args in protos]


def test_every_prototype_of_the_smooth_header_is_bound_exported_and_guard_banded(lib_built):
    from implementation_phd_lab_vision_amd import _lib
    from tests.rows import smooth as T
    protos = _prototypes()
    names = [n for n, _ in protos]
    assert set(names) == OPS == set(_lib._SIGNATURES_SMOOTH) and len(names) == len(set(names))
    assert set(re.findall(r"\b(r50_op_[a-z0-9_]+)\s*\(", HEADER.read_text())) == OPS, "a name in a comment is a prototype too"
    covered = set()
    for row in T.ROWS_SMOOTH:
        covered.update(row.ops)
    assert covered == OPS
    main_header, hal_header = (ROOT / "include" / "r50.h").read_text(), (ROOT / "include" / "r50_hal.h").read_text()
    for name, arity in protos:
        assert len(_lib._SIGNATURES_SMOOTH[name][1]) == arity, name
        assert hasattr(lib_built, name), f"{name} declared in r50_smooth.h but not exported by libr50hip.so"
        assert getattr(lib_built, name).argtypes == _lib._SIGNATURES_SMOOTH[name][1]
        assert name not in _lib._SIGNATURES and name not in _lib.EXPORTED_SYMBOLS and name not in _lib._SIGNATURES_HAL
        assert name not in main_header and name not in hal_header
    ids = [row.id for row in T.ROWS_SMOOTH]
    assert len(ids) == len(set(ids))
    assert "r50_smooth.h" in (ROOT / "implementation_phd_lab_vision_amd" / "_lib.py").read_text().split("def _source_digest")[1].split("def ")[0]


def _edges(pairs):
    flat = [v for e in pairs for v in e]
    return (ctypes.c_int * len(flat))(*flat)


BAD_EDGES = {"parent placed later": ((1, 2), (0, 1)), "child twice": ((0, 1), (2, 1)), "out of range": ((0, 5),), "negative": ((-1, 1),),
             "self": ((1, 1),), "cycle": ((0, 1), (1, 0))}


def test_every_refusal_returns_before_any_launch(lib_built):
    """No device is needed: each call is refused on its arguments, with the op's name in the message.  The pointers are made-up
    addresses that nothing dereferences."""
    x, out, tab, tab2, coef, short, stats = 0x10000, 0x90000, 0x110000, 0x120000, 0x130000, 0x140000, 0x150000
    n_bytes = 12 * 5 * 3 * 4                                                         # F = 12 rows of J = 5

    def refused(name, rc, why):
        assert rc != 0, (name, why)
        assert name.encode() in lib_built.r50_last_error(None), (name, why)

    fir = lib_built.r50_op_fir_sequences
    ok = dict(x=x, seg=tab, row=tab2, F=12, G=2, J=5, coef=coef, W=3, out=out, short=short)
    for kw in (dict(x=None), dict(seg=None), dict(row=None), dict(coef=None), dict(out=None), dict(short=None), dict(W=2), dict(W=0), dict(W=-1),
               dict(W=64), dict(W=65), dict(F=0), dict(G=0), dict(G=13), dict(J=0), dict(J=65), dict(F=2 ** 31), dict(out=x),
               dict(out=x + n_bytes - 4), dict(out=x - n_bytes + 4)):
        a = dict(ok, **kw)
        refused("r50_op_fir_sequences", fir(a["x"], a["seg"], a["row"], a["F"], a["G"], a["J"], a["coef"], a["W"], a["out"], a["short"], None), kw)

    euro = lib_built.r50_op_one_euro_sequences
    ok = dict(x=x, seg=tab, F=12, G=2, J=5, rate=25.0, mc=1.0, beta=0.0, dc=1.0, out=out)
    for kw in (dict(x=None), dict(seg=None), dict(out=None), dict(F=0), dict(G=0), dict(G=13), dict(J=0), dict(J=65), dict(rate=0.0),
               dict(rate=-1.0), dict(rate=float("inf")), dict(rate=float("nan")), dict(mc=0.0), dict(mc=float("nan")), dict(beta=-0.5),
               dict(beta=float("inf")), dict(dc=0.0), dict(dc=float("nan")), dict(out=x), dict(out=x + 8)):
        a = dict(ok, **kw)
        refused("r50_op_one_euro_sequences", euro(a["x"], a["seg"], a["F"], a["G"], a["J"], a["rate"], a["mc"], a["beta"], a["dc"], a["out"], None), kw)

    bs, br = lib_built.r50_op_bone_stats, lib_built.r50_op_bone_rebuild
    ok = dict(x=x, tab=tab, F=12, S=2, J=5, edges=_edges(EDGES5), E=4, stats=stats, out=out)
    cases = [dict(x=None), dict(tab=None), dict(edges=None), dict(stats=None), dict(F=0), dict(S=0), dict(S=13), dict(J=1), dict(J=65), dict(E=0),
             dict(E=5)] + [dict(edges=_edges(e), E=len(e)) for e in BAD_EDGES.values()]
    for kw in cases:
        a = dict(ok, **kw)
        refused("r50_op_bone_stats", bs(a["x"], a["tab"], a["F"], a["S"], a["J"], a["edges"], a["E"], a["stats"], None), kw)
    for kw in cases + [dict(out=None), dict(out=x), dict(out=x + n_bytes - 4)]:
        a = dict(ok, **kw)
        refused("r50_op_bone_rebuild", br(a["x"], a["tab"], a["F"], a["S"], a["J"], a["edges"], a["E"], a["stats"], a["out"], None), kw)


def test_host_validation_refuses_without_a_device():
    import torch
    from implementation_phd_lab_vision_amd import smooth
    for name, e in BAD_EDGES.items():
        with pytest.raises(ValueError):
            smooth.check_edges(e, 5)
    with pytest.raises(ValueError, match="J - 1"):
        smooth.check_edges(EDGES5, 4)
    with pytest.raises(ValueError):
        smooth.check_edges([], 5)
    assert smooth.check_edges(EDGES5, 5).tolist() == [list(e) for e in EDGES5]
    from implementation_phd_lab_vision_amd.train import H36M_EDGES
    assert smooth.check_edges(H36M_EDGES, 17).shape == (16, 2)
    for bad in (dict(window=8), dict(window=65), dict(window=0), dict(window=9, degree=9), dict(window=9, degree=-1), dict(window=3, degree=5)):
        with pytest.raises(ValueError):
            smooth.savgol_table(**{"window": 9, "degree": 2, **bad})
    for sigma in (0.0, -1.0, float("nan"), float("inf"), 10.5):
        with pytest.raises(ValueError):
            smooth.gauss_table(sigma)
    for bad in (dict(kind="median"), dict(kind="savgol", window=4), dict(kind="savgol", window=5, degree=5), dict(kind="one_euro", rate=0.0),
                dict(kind="one_euro", beta=-1.0), dict(kind="gauss", sigma=0.0), dict(fix_bones=True, edges=((1, 2), (0, 1)))):
        with pytest.raises(ValueError):
            smooth.PostProcess(**bad)
    with pytest.raises(ValueError, match="no CPU fallback"):                    # poses on the host: refused, not computed there
        smooth.PostProcess(kind="gauss").apply(torch.zeros(4, 17, 3), (np.array([0, 4]), np.arange(4)))
    for coef in (np.ones((2, 2)), np.ones((3, 2)), np.ones((65, 65)), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            smooth.check_coef(coef)


def test_tables_pass_through_device_tables():
    """``DeviceTables.of`` hands an instance back unchanged; here a stand-in of the right class."""
    import torch
    from implementation_phd_lab_vision_amd import smooth
    t = object.__new__(smooth.DeviceTables)
    t.device, t.rows = torch.device("cpu"), 4
    assert smooth.DeviceTables.of(t, "cpu") is t
    with pytest.raises(ValueError, match="uploaded"):
        smooth.DeviceTables.of(t, "cuda:0")


def test_segment_table_on_hand_written_tables():
    from implementation_phd_lab_vision_amd import smooth
    cases = [
        # a gap in idx inside one sequence
        (([0, 6], [3, 4, 5, 9, 10, 11]), ([0, 3, 6], [0, 0, 0, 1, 1, 1])),
        # a one-row sequence between two others
        (([0, 2, 3, 5], [0, 1, 7, 0, 1]), ([0, 2, 3, 5], [0, 0, 1, 2, 2])),
        # two sequences back to back whose idx happen to go on: the sequence boundary still cuts
        (([0, 3, 6], [0, 1, 2, 3, 4, 5]), ([0, 3, 6], [0, 0, 0, 1, 1, 1])),
        # idx running backwards or repeating: every row its own segment
        (([0, 3], [5, 5, 4]), ([0, 1, 2, 3], [0, 1, 2])),
        (([0, 1], [9]), ([0, 1], [0])),
    ]
    for (seq_start, idx), (want_start, want_seg) in cases:
        got = smooth.segment_table(np.array(seq_start, dtype=np.int32), np.array(idx, dtype=np.int32))
        assert got[0].dtype == got[1].dtype == np.int32
        assert got[0].tolist() == want_start and got[1].tolist() == want_seg, (seq_start, idx)
        ref = SR.segment_table(seq_start, idx)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    for bad in (([0, 0, 3], [0, 1, 2]), ([1, 3], [0, 1, 2]), ([0, 2], [0, 1, 2]), ([0, 3, 2, 3], [0, 1, 2]), ([0], [])):
        with pytest.raises(ValueError):
            smooth.segment_table(np.array(bad[0], dtype=np.int32), np.array(bad[1], dtype=np.int32))
    rng = np.random.default_rng(0)
    lens = rng.integers(1, 9, size=20)
    idx = np.concatenate([np.sort(rng.choice(30, size=n, replace=False)) for n in lens]).astype(np.int32)
    seq_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    got, ref = smooth.segment_table(seq_start, idx), SR.segment_table(seq_start, idx)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("sigma", [0.4, 1.0, 1.5, 3.3, 10.0])
def test_gauss_table(sigma):
    from implementation_phd_lab_vision_amd import smooth
    coef = smooth.gauss_table(sigma)
    w = 2 * int(np.ceil(3 * sigma)) + 1
    r = (w - 1) // 2
    assert coef.shape == (w, w) and coef.dtype == np.float64 and w <= 63
    assert np.abs(coef.sum(axis=1) - 1.0).max() <= 1e-14
    assert np.allclose(coef, SR.gauss_table(sigma), rtol=1e-14, atol=0.0)
    assert np.all(coef >= 0.0) and np.allclose(coef, coef[::-1, ::-1], rtol=1e-14, atol=0.0)
    centre = np.exp(-np.arange(-r, r + 1) ** 2 / (2 * sigma * sigma))
    assert np.allclose(coef[r], centre / centre.sum(), rtol=1e-14, atol=0.0)
    assert np.all(coef[0, r + 1:] == 0.0) and np.all(coef[0, :r + 1] > 0.0)       # the first row sees positions 0 .. R only


@pytest.mark.parametrize("window,degree", [(1, 0), (3, 1), (5, 2), (5, 4), (9, 2), (9, 3), (21, 3), (63, 2), (63, 5)])
def test_savgol_table(window, degree):
    from implementation_phd_lab_vision_amd import smooth
    coef = smooth.savgol_table(window, degree)
    assert coef.shape == (window, window) and coef.dtype == np.float64
    assert np.abs(coef.sum(axis=1) - 1.0).max() <= 1e-14
    assert np.allclose(coef, SR.savgol_table(window, degree), rtol=0.0, atol=1e-12)
    # rows reproduce the monomials up to the degree at every evaluation position; positions scaled to [-1, 1] so that 1e-10 means the
    # same at every window (k^5 at k = 62 is 9e8)
    r = (window - 1) // 2
    t = (np.arange(window) - r) / max(r, 1)
    for m in range(degree + 1):
        assert np.abs(coef @ t ** m - t ** m).max() <= 1e-10, m
    if window <= 9:                                                                 # and unscaled where the powers are small
        k = np.arange(window, dtype=np.float64)
        for m in range(degree + 1):
            assert np.abs(coef @ k ** m - k ** m).max() <= 1e-10 * max(1.0, float(k[-1] ** m)), m
    if degree == window - 1:
        assert np.allclose(coef, np.eye(window), rtol=0.0, atol=1e-12)              # interpolation: nothing is smoothed


def test_window_one_is_the_identity_table():
    from implementation_phd_lab_vision_amd import smooth
    coef = smooth.savgol_table(1, 0)
    assert coef.tolist() == [[1.0]]
    post = smooth.PostProcess(kind="savgol", window=1, degree=0)
    assert post.look_ahead == 0 and post.causal and "look-ahead R=0" in post.describe()
    assert smooth.PostProcess(kind="gauss").look_ahead == 5 and not smooth.PostProcess(kind="gauss").causal
    assert "not causal" in smooth.PostProcess(kind="savgol").describe() and "R=4" in smooth.PostProcess(kind="savgol").describe()
    assert smooth.PostProcess(kind="one_euro").causal and "(causal" in smooth.PostProcess(kind="one_euro").describe()


def test_centred_savgol_row_is_the_textbook_filter():
    from implementation_phd_lab_vision_amd import smooth
    # Savitzky and Golay 1964, table I: quadratic / cubic smoothing over 5 and 7 points
    assert np.allclose(smooth.savgol_table(5, 2)[2] * 35.0, [-3, 12, 17, 12, -3], rtol=0, atol=1e-12)
    assert np.allclose(smooth.savgol_table(7, 3)[3] * 21.0, [-2, 3, 6, 7, 6, 3, -2], rtol=0, atol=1e-12)


RESULTS_BASE = ["--features_root", "f", "--preprocessed_root", "p", "--model_path", "m"]
PREDICT_BASE = ["--frames", "x.npy", "--model_path", "m", "--out", "o"]
PARAMS = {"gauss": [["--smooth-sigma", "2.0"]], "savgol": [["--smooth-window", "7"], ["--smooth-degree", "3"]],
          "one_euro": [["--smooth-rate", "50"], ["--one-euro-min-cutoff", "0.5"], ["--one-euro-beta", "0.01"], ["--one-euro-d-cutoff", "2"]]}


def test_results_parser():
    from implementation_phd_lab_vision_amd import results
    plain = results.parse_args(RESULTS_BASE + ["--dense"])
    assert not any(hasattr(plain, k) for k in ("dense_smooth", "dense_fix_bones", "smooth_sigma", "smooth_window", "one_euro_beta"))
    assert results.dense_post(plain) is None
    for flags in (["--dense-smooth", "gauss"], ["--dense-fix-bones"]):
        with pytest.raises(SystemExit):
            results.parse_args(RESULTS_BASE + flags)                                # without --dense
        args = results.parse_args(RESULTS_BASE + ["--dense"] + flags)
        assert {k: v for k, v in vars(args).items() if k not in ("dense_smooth", "dense_fix_bones")} == vars(plain)
    for kind, params in PARAMS.items():
        for param in params:
            with pytest.raises(SystemExit):
                results.parse_args(RESULTS_BASE + ["--dense"] + param)              # no filter at all
            with pytest.raises(SystemExit):
                results.parse_args(RESULTS_BASE + ["--dense", "--dense-fix-bones"] + param)
            for other in PARAMS:
                if other != kind:
                    with pytest.raises(SystemExit):
                        results.parse_args(RESULTS_BASE + ["--dense", "--dense-smooth", other] + param)
            assert results.dense_post(results.parse_args(RESULTS_BASE + ["--dense", "--dense-smooth", kind] + param)).kind == kind
    for bad in (["--dense-smooth", "savgol", "--smooth-window", "8"], ["--dense-smooth", "savgol", "--smooth-window", "5", "--smooth-degree", "5"],
                ["--dense-smooth", "gauss", "--smooth-sigma", "0"], ["--dense-smooth", "one_euro", "--smooth-rate", "0"],
                ["--dense-smooth", "median"]):
        with pytest.raises(SystemExit):
            results.parse_args(RESULTS_BASE + ["--dense"] + bad)
    post = results.dense_post(results.parse_args(RESULTS_BASE + ["--dense", "--dense-smooth", "one_euro", "--one-euro-beta", "0.25",
                                                                 "--dense-fix-bones"]))
    assert (post.kind, post.beta, post.rate, post.min_cutoff, post.d_cutoff, post.fix_bones) == ("one_euro", 0.25, 25.0, 1.0, 1.0, True)
    post = results.dense_post(results.parse_args(RESULTS_BASE + ["--dense", "--dense-smooth", "gauss"]))
    assert (post.sigma, post.table.shape, post.fix_bones) == (1.5, (11, 11), False)
    post = results.dense_post(results.parse_args(RESULTS_BASE + ["--dense", "--dense-smooth", "savgol"]))
    assert (post.window, post.degree) == (9, 2)


def test_predict_parser():
    from implementation_phd_lab_vision_amd import predict
    plain = predict.parse_args(PREDICT_BASE)
    assert vars(plain) == vars(predict.build_parser().parse_args(PREDICT_BASE)) and not hasattr(plain, "smooth") and not hasattr(plain, "fix_bones")
    assert predict.video_post(plain) is None
    for kind, params in PARAMS.items():
        for param in params:
            with pytest.raises(SystemExit):
                predict.parse_args(PREDICT_BASE + param)
            with pytest.raises(SystemExit):
                predict.parse_args(PREDICT_BASE + ["--fix-bones"] + param)
            assert predict.video_post(predict.parse_args(PREDICT_BASE + ["--smooth", kind] + param)).kind == kind
    post = predict.video_post(predict.parse_args(PREDICT_BASE + ["--fix-bones"]))
    assert post.kind is None and post.fix_bones


def test_bone_std_mm_pools_within_sequence_deviations():
    from implementation_phd_lab_vision_amd import smooth
    rng = np.random.default_rng(3)
    seq_start = np.array([0, 7, 8, 20])
    x = (rng.standard_normal((20, 5, 3)) + np.array([0.0, 0.0, 5.0])).astype(np.float32)
    stats = SR.bone_stats(x, seq_start, EDGES5)
    per, over = smooth.bone_std_mm(stats, np.diff(seq_start), np.array([1, 0, 1]), 3)
    assert over == pytest.approx(SR.bone_std_mm(x, seq_start, EDGES5), rel=1e-12)
    assert per[1] == pytest.approx(SR.bone_std_mm(x, seq_start, EDGES5, seqs=[0, 2]), rel=1e-12)
    assert per[0] == 0.0 and np.isnan(per[2])                                       # a one-row sequence; a group without rows
    ln = SR.bone_lengths(x, EDGES5)
    assert stats[0, :, 0] == pytest.approx(ln[:7].mean(axis=0), rel=1e-14)
    assert stats[0, :, 1] == pytest.approx(((ln[:7] - ln[:7].mean(axis=0)) ** 2).sum(axis=0), rel=1e-12)


def test_restatement_against_scipy_where_it_is_installed():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(1)
    x = rng.standard_normal((40, 2, 3)).astype(np.float32)
    seq_start, idx = np.array([0, 40]), np.arange(40)
    for w, p in ((9, 2), (5, 3), (11, 4)):
        got, short = SR.fir(x, seq_start, idx, SR.savgol_table(w, p))
        want = signal.savgol_filter(x.astype(np.float64), w, p, axis=0, mode="interp")
        assert short == 0 and np.abs(got - want).max() <= 1e-5
    # a Gaussian in the interior is scipy's truncated kernel
    sigma = 1.5
    got, _ = SR.fir(x, seq_start, idx, SR.gauss_table(sigma))
    from scipy import ndimage
    r = int(np.ceil(3 * sigma))
    want = ndimage.gaussian_filter1d(x.astype(np.float64), sigma, axis=0, truncate=r / sigma, mode="nearest")      # radius int(r + 0.5) = r
    assert np.abs(got[r:-r] - want[r:-r]).max() <= 1e-5


def test_restatement_rebuild_gives_every_bone_its_length():
    rng = np.random.default_rng(2)
    seq_start = np.array([0, 6, 11])
    x = (rng.standard_normal((11, 5, 3)) * 0.3 + np.array([0.0, 0.0, 5.0])).astype(np.float32)
    stats = SR.bone_stats(x, seq_start, EDGES5)
    out = SR.bone_rebuild(x, seq_start, EDGES5, stats)
    assert np.array_equal(out[:, 0].view(np.uint32), x[:, 0].view(np.uint32))
    ln = SR.bone_lengths(out, EDGES5)
    want = np.repeat(stats[:, :, 0], np.diff(seq_start), axis=0)
    assert np.abs(ln - want).max() <= 4 * np.spacing(np.float32(8.0))
    assert SR.bone_std_mm(out, seq_start, EDGES5) < 1e-2 < SR.bone_std_mm(x, seq_start, EDGES5)
