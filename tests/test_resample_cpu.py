"""Resampling of pose sequences (INTEGRATION.md section AB) without a GPU: the eighth public header include/r50_resample.h bound,
exported and guard-banded; every refusal of the C entry before any launch; the refusals of ``ResampleTable``; the properties of the numpy
restatement tests/resample_reference.py that the GPU comparison stands on; ``uniform_times`` and the holdout table; the parsers."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import resample_reference as RR
from tests.test_kinematics_cpu import PREDICT_KEYS, RESULTS_KEYS

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "r50_resample.h"
OPS = {"r50_op_resample_sequences"}
STAMPS = np.array([0, 1, 3, 4, 7, 8, 9, 12])


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = re.findall(r"^\s*(?:int|int64_t|size_t)\s+(r50_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    assert protos, "no prototypes parsed from include/r50_resample.h"
    return [(name, len([a for a in args.split(",") if a.strip()])) for name, args in protos]


def test_every_prototype_of_the_resample_header_is_bound_exported_and_guard_banded(lib_built):
    from implementation_phd_lab_vision_amd import _lib
    from tests.rows import resample as T
    protos = _prototypes()
    names = [n for n, _ in protos]
    assert set(names) == OPS == set(_lib._SIGNATURES_RESAMPLE) and len(names) == len(set(names))
    covered = set()
    for row in T.ROWS_RESAMPLE:
        covered.update(row.ops)
    assert covered == OPS and len({row.id for row in T.ROWS_RESAMPLE}) == len(T.ROWS_RESAMPLE)
    others = [(ROOT / "include" / h).read_text() for h in ("r50.h", "r50_hal.h", "r50_smooth.h", "r50_multiview.h", "r50_kinematics.h",
                                                            "r50_refine.h", "r50_track.h")]
    tables = (_lib._SIGNATURES, _lib._SIGNATURES_HAL, _lib._SIGNATURES_SMOOTH, _lib._SIGNATURES_MULTIVIEW, _lib._SIGNATURES_KINEMATICS,
              _lib._SIGNATURES_REFINE, _lib._SIGNATURES_TRACK)
    for name, arity in protos:
        assert len(_lib._SIGNATURES_RESAMPLE[name][1]) == arity, name
        assert hasattr(lib_built, name), f"{name} declared in r50_resample.h but not exported by libr50hip.so"
        assert getattr(lib_built, name).argtypes == _lib._SIGNATURES_RESAMPLE[name][1]
        assert not any(name in table for table in tables)
        assert name not in _lib.EXPORTED_SYMBOLS and not any(name in text for text in others)
    assert "r50_resample.h" in (ROOT / "implementation_phd_lab_vision_amd" / "_lib.py").read_text().split("def _source_digest")[1].split("def ")[0]
    abi = (ROOT / "implementation_phd_lab_vision_amd" / "csrc" / "r50_abi.hip").read_text()
    assert '#include "resample_kernels.h"' in abi and "r50_resample.h" in abi


def test_every_refusal_of_the_c_entry_returns_before_any_launch(lib_built):
    """No device is needed: each call is refused on its arguments.  The pointers are made-up addresses that nothing dereferences."""
    x, idx, seq_start, out_time, out_seq, out_left, y, flags = (0x10000000 * k for k in range(1, 9))
    ok = dict(x=x, idx=idx, seq_start=seq_start, F=100, S=3, J=17, out_time=out_time, out_seq=out_seq, out_left=out_left, G=50, kind=1,
              max_gap=2, y=y, flags=flags)
    limit = (1 << 31) // 192
    bad = [(dict(**{name: None}), "null pointer") for name in ("x", "idx", "seq_start", "out_time", "out_seq", "out_left", "y", "flags")]
    bad += [(kw, "invalid arguments") for kw in (dict(F=0), dict(F=-1), dict(S=0), dict(S=101), dict(J=0), dict(J=65), dict(G=0), dict(G=-3),
                                                 dict(F=limit + 1, S=1), dict(F=1 << 40), dict(G=limit + 1), dict(G=1 << 40))]
    bad += [(kw, "kind must be") for kw in (dict(kind=2), dict(kind=-1))]
    bad += [(kw, "max_gap must be") for kw in (dict(max_gap=0), dict(max_gap=-5))]
    bad += [(kw, "8-byte aligned") for kw in (dict(out_time=out_time + 4), dict(out_time=out_time + 1))]
    bad += [(kw, "overlaps") for kw in (dict(y=x), dict(y=x + 100 * 17 * 12 - 4), dict(y=x - 50 * 17 * 12 + 4), dict(y=idx + 396), dict(y=seq_start + 12),
                                        dict(y=out_time + 8), dict(y=out_seq), dict(y=out_left + 196), dict(flags=x + 64), dict(flags=idx),
                                        dict(flags=seq_start), dict(flags=out_time + 392), dict(flags=out_seq - 196), dict(flags=out_left),
                                        dict(flags=y), dict(flags=y + 50 * 17 * 12 - 4), dict(y=flags + 196))]
    for kw, why in bad:
        a = dict(ok, **kw)
        rc = lib_built.r50_op_resample_sequences(a["x"], a["idx"], a["seq_start"], a["F"], a["S"], a["J"], a["out_time"], a["out_seq"],
                                                 a["out_left"], a["G"], a["kind"], a["max_gap"], a["y"], a["flags"], None)
        assert rc == -1, (kw, rc)                                                    # R50_ERR_INVALID: refused, not a launch that failed
        msg = lib_built.r50_last_error(None)
        assert b"r50_op_resample_sequences" in msg and why.encode() in msg, (kw, msg)


# ---- ResampleTable -----------------------------------------------------------------------------------------------------------------------------
def test_resample_table_rows_and_refusals():
    from implementation_phd_lab_vision_amd import resample
    c = RR.ragged_case(3)
    t = resample.ResampleTable(c["seq_start"], c["idx"], c["out_time"], c["out_seq"])
    assert np.array_equal(t.out_left, c["out_left"]) and t.out_left.dtype == np.int32 and t.out_time.dtype == np.float64
    assert (t.rows, t.sequences, t.outputs) == (c["f"], c["s"], c["g"])
    assert np.array_equal(resample.left_rows(c["seq_start"], c["idx"], c["out_time"], c["out_seq"]), c["out_left"])
    same = resample.ResampleTable(c["seq_start"], c["idx"], c["out_time"], c["out_seq"], c["out_left"])
    assert np.array_equal(same.out_left, t.out_left)

    def refused(match, **kw):
        a = dict(seq_start=c["seq_start"], idx=c["idx"], out_time=c["out_time"], out_seq=c["out_seq"], out_left=c["out_left"])
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            resample.ResampleTable(a["seq_start"], a["idx"], a["out_time"], a["out_seq"], a["out_left"])

    idx = c["idx"].copy()
    idx[9] = idx[8]                                                                 # a repeated stamp (the rows 6 .. 9 are one sequence)
    refused("strictly increasing", idx=idx, out_left=None)
    idx = c["idx"].copy()
    idx[30] = idx[29] - 1
    refused("strictly increasing", idx=idx, out_left=None)
    inner = np.flatnonzero((c["out_left"] > c["seq_start"][c["out_seq"]]) & (c["out_left"] < c["seq_start"][c["out_seq"] + 1] - 1))
    for delta in (-1, 1):
        left = c["out_left"].copy()
        left[inner[3]] += delta
        refused("out_left", out_left=left)
    g = int(np.flatnonzero(c["out_seq"] == 4)[0])                                   # the same position, in the wrong sequence
    left = c["out_left"].copy()
    left[g] = c["seq_start"][5] + (left[g] - c["seq_start"][4])
    refused("out_left", out_left=left)
    refused("out_left", out_left=c["out_left"][:-1])
    for v in (np.nan, np.inf, -np.inf):
        tau = c["out_time"].copy()
        tau[5] = v
        refused("finite", out_time=tau, out_left=None)
    seq = c["out_seq"].copy()
    seq[0] = c["s"]
    refused("out_seq", out_seq=seq)
    seq[0] = -1
    refused("out_seq", out_seq=seq)
    refused("expected", out_time=c["out_time"][:-1])
    refused("expected", out_time=np.zeros(0), out_seq=np.zeros(0, np.int32), out_left=None)
    refused("seq_start", seq_start=c["seq_start"][:-1])
    with pytest.raises(ValueError, match="ResampleTable"):
        resample.resample_sequences(None, (c["seq_start"], c["idx"]))
    import torch
    with pytest.raises(ValueError, match="no CPU fallback"):
        resample.resample_sequences(torch.from_numpy(c["x"]), t, "cubic", 3)
    with pytest.raises(ValueError, match="kind"):
        resample.resample_sequences(torch.from_numpy(c["x"]), t, "quintic", 3)
    for bad in (dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(step=float("inf")), dict(step=1.0, kind="nearest")):
        with pytest.raises(ValueError):
            resample.ResampleSettings(**bad)
    assert resample.ResampleSettings(1).describe() == "step=1 kind=cubic" and resample.ResampleSettings(5 / 3, "linear").describe() == "step=1.66667 kind=linear"
    assert resample.ResampleSettings(0.75).times(np.array([0, 2, 4])).tolist() == [0.0, 0.75, 1.5, 2.25, 3.0, 3.75]
    assert resample.ResampleSettings(1).times(np.array([0, 2, 4, 6])).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]


# ---- the reference's own properties ------------------------------------------------------------------------------------------------------
def _one_sequence(stamps, times):
    return RR.table([0, len(stamps)], stamps, times, np.zeros(len(times), dtype=np.int32))


def _poly_case(coefs):
    """Integer-valued polynomials in time on STAMPS, three joints; 97 times across the whole range."""
    times = np.linspace(0.0, 12.0, 97)
    assert times.size == 97 and np.all(times * 8 == np.round(times * 8))            # multiples of 1/8: exact
    c = np.asarray(coefs, dtype=np.float64).reshape(-1, 1, 3, 3)                   # (degree + 1, 1, J, 3)
    poly = lambda t: sum(c[k] * np.asarray(t, dtype=np.float64).reshape(-1, 1, 1) ** k for k in range(c.shape[0]))   # noqa: E731
    return _one_sequence(STAMPS, times), poly(STAMPS).astype(np.float32), poly(times), times


def test_both_kinds_reproduce_an_integer_linear_trajectory_exactly():
    """The trajectory stays away from 0 (offsets in [200, 300), slopes in [-10, 10) over 12 frames): the fp64 result is then within a
    few fp64 ulp of a value that fp32 holds exactly, and the store rounds it onto that value.  At a zero crossing the cubic form's four
    terms cancel to a residue of the order 1e-15, which fp32 can represent: exact there only by luck."""
    rng = np.random.default_rng(1)
    t, x, want, _ = _poly_case(np.stack([rng.integers(200, 300, size=(3, 3)), rng.integers(-10, 10, size=(3, 3))]))
    assert want.min() > 0
    for kind in ("linear", "cubic"):
        y, flags = RR.resample(x, t["idx"], t["seq_start"], t["out_time"], t["out_seq"], t["out_left"], kind, 3)
        assert np.array_equal(y.astype(np.float64), want) and not flags.any(), kind


def test_cubic_reproduces_integer_quadratics_up_to_the_run_ends():
    rng = np.random.default_rng(2)
    t, x, want, _ = _poly_case(rng.integers(-20, 20, size=(3, 3, 3)))
    y, flags = RR.resample(x, t["idx"], t["seq_start"], t["out_time"], t["out_seq"], t["out_left"], "cubic", 3)
    err = float(np.abs(y.astype(np.float64) - want).max())
    print(f"cubic on quadratics: max error {err!r} at max |p| {np.abs(want).max()!r}")
    assert err <= 1e-12 * np.abs(want).max() and not flags.any()
    lin, _ = RR.resample(x, t["idx"], t["seq_start"], t["out_time"], t["out_seq"], t["out_left"], "linear", 3)
    assert np.abs(lin.astype(np.float64) - want).max() > 1.0                        # the property is the cubic form's


def test_a_smaller_max_gap_flags_exactly_the_times_inside_the_breaks():
    rng = np.random.default_rng(2)
    t, x, _, times = _poly_case(rng.integers(-20, 20, size=(3, 3, 3)))
    for kind in ("linear", "cubic"):
        y, flags = RR.resample(x, t["idx"], t["seq_start"], t["out_time"], t["out_seq"], t["out_left"], kind, 2)
        inside = ((times > 4) & (times < 7)) | ((times > 9) & (times < 12))
        assert np.array_equal(flags, np.where(inside, RR.IN_BREAK, 0)) and inside.sum() == 2 * 23
        for g in np.flatnonzero(inside):
            lo, hi = (3, 4) if times[g] < 7 else (6, 7)
            near = lo if times[g] - STAMPS[lo] <= STAMPS[hi] - times[g] else hi     # the left one on the tie 5.5 / 10.5
            assert np.array_equal(y[g].view(np.int32), x[near].view(np.int32))
        assert np.array_equal(y[times == 5.5][0], x[3]) and np.array_equal(y[times == 10.5][0], x[6])
    out = _one_sequence(STAMPS, [-0.5, 12.5, 0.0, 12.0])
    y, flags = RR.resample(x, out["idx"], out["seq_start"], out["out_time"], out["out_seq"], out["out_left"], "cubic", 3)
    assert flags.tolist() == [RR.OUTSIDE, RR.OUTSIDE, 0, 0] and np.array_equal(y[0], x[0]) and np.array_equal(y[1], x[-1])
    assert np.array_equal(y[2], x[0]) and np.array_equal(y[3], x[-1])


def _band_limited(n, joints, seed):
    """A seeded sum of sinusoids with periods of 12 rows and more, in metres around z = 5."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)[:, None, None, None]
    freq = rng.uniform(1.0 / 60.0, 1.0 / 12.0, size=(1, 6, joints, 3))
    amp = rng.uniform(0.02, 0.10, size=(1, 6, joints, 3))
    phase = rng.uniform(0.0, 2.0 * np.pi, size=(1, 6, joints, 3))
    return ((amp * np.sin(2.0 * np.pi * freq * t + phase)).sum(axis=1) + np.array([0.0, 0.0, 5.0])).astype(np.float32)


def test_cubic_holds_out_better_than_linear_on_a_band_limited_trajectory():
    x = _band_limited(121, 17, 3)
    stamps = np.arange(121)
    t = _one_sequence(stamps[::2], stamps.astype(np.float64))
    err = {}
    for kind in ("linear", "cubic"):
        y, flags = RR.resample(x[::2], t["idx"], t["seq_start"], t["out_time"], t["out_seq"], t["out_left"], kind, 2)
        assert not flags.any() and np.array_equal(y[::2].view(np.int32), x[::2].view(np.int32))
        err[kind] = float(np.linalg.norm(y[1::2].astype(np.float64) - x[1::2], axis=2).mean() * 1000.0)
    print(f"holdout error on the band-limited trajectory decimated by 2 (mm): {err}")
    assert err["cubic"] < err["linear"]


def test_the_ragged_table_runs_every_branch():
    """What the comparison below stands on: the case holds every case of the header and every tangent rule."""
    c = RR.ragged_case(3, seed=3)
    c["want"] = {"cubic": RR.resample(c["x"], c["idx"], c["seq_start"], c["out_time"], c["out_seq"], c["out_left"], "cubic", c["max_gap"])}
    idx, ss, mg = c["idx"].astype(np.int64), c["seq_start"], c["max_gap"]
    flags = c["want"]["cubic"][1]
    assert (flags == 0).any() and (flags == RR.IN_BREAK).any() and (flags == RR.OUTSIDE).any() and (c["g"] * 3) % 256 and c["g"] % 2
    gaps = np.concatenate([np.diff(idx[ss[s]:ss[s + 1]]) for s in range(c["s"])])
    assert (gaps == mg).any() and (gaps == mg + 1).any()
    seen = set()
    for g in np.flatnonzero(flags == 0):
        i, s, tau = int(c["out_left"][g]), int(c["out_seq"][g]), c["out_time"][g]
        a, b = int(ss[s]), int(ss[s + 1])
        if tau == idx[i]:
            seen.add("knot")
            continue
        left = i - 1 >= a and idx[i] - idx[i - 1] <= mg
        right = i + 2 < b and idx[i + 2] - idx[i + 1] <= mg
        seen.add(("both" if left else "one-sided right" if right else "secant", "both" if right else "one-sided left" if left else "secant"))
    assert seen == {"knot", ("both", "both"), ("both", "one-sided left"), ("one-sided right", "both"), ("secant", "secant")}
    tie = [g for g in np.flatnonzero(flags == RR.IN_BREAK)
           if c["out_time"][g] - idx[c["out_left"][g]] == idx[c["out_left"][g] + 1] - c["out_time"][g]]
    assert tie, "a time on the tie point of a break"
    last = ss[1:] - 1
    assert all(((c["out_left"] == r) & (c["out_time"] == idx[r])).any() for r in last), "the very last knot of every sequence"
    near = np.abs(c["out_time"] - idx[c["out_left"]])
    assert ((near > 0) & (near < 1e-8)).any()


# ---- the host tables -----------------------------------------------------------------------------------------------------------------------
def test_uniform_times_never_emits_a_time_inside_a_break():
    from implementation_phd_lab_vision_amd import resample
    c = RR.ragged_case(2)
    for step, phase in ((1.0, 0.0), (0.5, 0.0), (5 / 3, 0.0), (0.3, 0.25), (7.0, 0.0), (1.0, 0.5)):
        tau, seq = resample.uniform_times(c["seq_start"], c["idx"], step, c["max_gap"], phase)
        assert tau.dtype == np.float64 and seq.dtype == np.int32 and tau.size == seq.size and tau.size > 0
        n_all = 0
        for s in range(c["s"]):
            t = c["idx"][c["seq_start"][s]:c["seq_start"][s + 1]].astype(np.float64)
            every = t[0] + phase + np.arange(int((t[-1] - t[0]) / step) + 2) * step
            every = every[every <= t[-1]]
            n_all += every.size
            mine = tau[seq == s]
            assert np.all(np.isin(mine, every)) and np.all(np.diff(mine) > 0)
            for v in every:                                                         # left out exactly when strictly inside a break
                i = np.searchsorted(t, v, side="right") - 1
                in_break = v != t[i] and t[i + 1] - t[i] > c["max_gap"]
                assert (v in mine) == (not in_break), (s, v)
        assert tau.size <= n_all
        table = resample.ResampleTable(c["seq_start"], c["idx"], tau, seq)
        assert table.bridged(c["max_gap"]).all()
        x = c["x"]
        for kind in ("linear", "cubic"):
            _, flags = RR.resample(x, table.idx, table.seq_start, table.out_time, table.out_seq, table.out_left, kind, c["max_gap"])
            assert not flags.any()
    full = resample.ResampleTable(c["seq_start"], c["idx"], c["out_time"], c["out_seq"])
    _, flags = RR.resample(c["x"], c["idx"], c["seq_start"], c["out_time"], c["out_seq"], c["out_left"], "cubic", c["max_gap"])
    assert np.array_equal(full.bridged(c["max_gap"]), flags == 0) and (flags == RR.IN_BREAK).any() and (flags == RR.OUTSIDE).any()
    for bad in (dict(step=0.0), dict(step=-1.0), dict(step=1.0, phase=-0.5), dict(step=1.0, max_gap=0), dict(step=float("nan"))):
        with pytest.raises(ValueError):
            resample.uniform_times(c["seq_start"], c["idx"], **{"max_gap": 3, **bad})


def test_the_holdout_table_keeps_segment_ends_and_bridges_every_held_out_row():
    from implementation_phd_lab_vision_amd import resample, smooth
    # sequences of 1, 2, 9, 10 and 30 rows; the stamps jump by 2 and by 5 inside the last two (segments of their own)
    lens = [1, 2, 9, 10, 30]
    seq_start = np.concatenate([[0], np.cumsum(lens)])
    idx = np.concatenate([np.arange(n) + 3 * k for k, n in enumerate(lens)])
    idx[seq_start[3] + 4:seq_start[4]] += 1
    idx[seq_start[4] + 7:] += 4
    idx[seq_start[4] + 8:] += 1                                                     # a segment of one row
    for k in (2, 3, 4, 7):
        keep, table = resample.holdout_table(seq_start, idx, k)
        assert np.array_equal(keep, RR.holdout_rows(seq_start, idx, k))
        seg_start, _ = smooth.segment_table(seq_start, idx)
        assert keep[seg_start[:-1]].all() and keep[seg_start[1:] - 1].all() and not keep.all()
        assert table.rows == int(keep.sum()) and table.outputs == idx.size and table.sequences == len(lens)
        assert np.array_equal(table.idx, idx[keep]) and np.array_equal(table.out_time, idx.astype(np.float64))
        assert table.bridged(k).all()
        kept_rows = np.flatnonzero(keep)
        assert np.array_equal(kept_rows[table.out_left[keep]], kept_rows)           # a kept row is its own left row: copied bit for bit
        _, flags = RR.resample(np.zeros((table.rows, 1, 3), np.float32), table.idx, table.seq_start, table.out_time, table.out_seq,
                               table.out_left, "cubic", k)
        assert not flags.any()
    for bad in (1, 0, -2):
        with pytest.raises(ValueError, match="K >= 2"):
            resample.holdout_table(seq_start, idx, bad)


# ---- the parsers -----------------------------------------------------------------------------------------------------------------------------
def test_parser_flag_rules_and_unchanged_default_namespaces(capsys):
    from implementation_phd_lab_vision_amd import predict, resample, results
    base_p = ["--frames", "a.npz", "--model_path", "m", "--out", "o"]
    base_r = ["--features_root", "f", "--preprocessed_root", "v", "--model_path", "m"]
    plain = predict.parse_args(base_p)
    assert sorted(vars(plain)) == PREDICT_KEYS and predict.video_resample(plain) is None
    assert sorted(vars(results.parse_args(base_r))) == RESULTS_KEYS and sorted(vars(results.parse_args(base_r + ["--dense"]))) == RESULTS_KEYS
    a = predict.parse_args(base_p + ["--resample", "1"])
    assert a.resample == 1.0 and sorted(vars(a)) == sorted(PREDICT_KEYS + ["resample"])
    assert predict.video_resample(a) == resample.ResampleSettings(1.0, "cubic")
    a = predict.parse_args(base_p + ["--resample", "1.6666666666666667", "--resample-kind", "linear"])
    assert sorted(vars(a)) == sorted(PREDICT_KEYS + ["resample", "resample_kind"])
    assert predict.video_resample(a) == resample.ResampleSettings(2 * 25 / 30, "linear")
    a = results.parse_args(base_r + ["--dense", "--dense-holdout", "2"])
    assert a.dense_holdout == 2 and sorted(vars(a)) == sorted(RESULTS_KEYS + ["dense_holdout"])
    a = results.parse_args(base_r + ["--dense", "--dense-holdout", "5", "--dense-holdout-kind", "linear"])
    assert (a.dense_holdout, a.dense_holdout_kind) == (5, "linear") and sorted(vars(a)) == sorted(RESULTS_KEYS + ["dense_holdout", "dense_holdout_kind"])
    for bad in (["--resample-kind", "linear"], ["--resample", "0"], ["--resample", "-1"], ["--resample", "nan"], ["--resample", "inf"],
                ["--resample", "1", "--resample-kind", "nearest"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base_p + bad)
    for bad in (["--dense-holdout", "2"], ["--dense", "--dense-holdout", "1"], ["--dense", "--dense-holdout", "0"], ["--dense", "--dense-holdout", "-3"],
                ["--dense", "--dense-holdout", "2.5"], ["--dense", "--dense-holdout-kind", "linear"]):
        with pytest.raises(SystemExit):
            results.parse_args(base_r + bad)
    err = capsys.readouterr().err
    assert "--resample-kind needs --resample" in err and "--dense-holdout needs --dense" in err and "K >= 2" in err
    assert "--dense-holdout-kind needs --dense-holdout" in err and "--resample: the step must be finite and > 0" in err


def test_the_product_never_imports_the_test_restatement():
    pkg = ROOT / "implementation_phd_lab_vision_amd"
    for path in [pkg / "resample.py", pkg / "predict.py", pkg / "results.py", ROOT / "scripts" / "bench_resample.py"]:
        text = path.read_text()
        assert "resample_reference" not in text and "from tests" not in text and "import tests" not in text, path
