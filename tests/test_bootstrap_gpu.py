"""The stratified cluster bootstrap on the MI355X (INTEGRATION.md section AC): ``r50_op_bootstrap_sums`` against the numpy restatement
tests/bootstrap_reference.py -- the multiplicities exactly, the sums bit for bit (the bar is 1 fp64 ulp per element; the observed maximum
is printed) --, the same bits under different windows, cuts of the replicate range, runs and with ``counts`` NULL, and the report end to end
on the synthetic cache of tests/results_data.py with a tiny head."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import bootstrap_reference as BR
from tests import results_data as rd
from tests.rows.bootstrap import unit_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
SEED_HIGH = 0xFEDCBA9876543210                                                      # bits set in both key words
F64, I32 = torch.float64, torch.int32


@functools.lru_cache(maxsize=None)
def _lib():
    from implementation_phd_lab_vision_amd import _lib as L
    L.build_library()
    return L.load_library()


def _op(v, start, reps, seed, r0=0, window=32768, counts=True):
    """The C entry itself (the wrapper lowers ``window`` to the largest stratum): (out, counts or None) as numpy."""
    vd, sd = torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.asarray(start, dtype=np.int32)).to(DEV)
    u, m, g = v.shape[0], v.shape[1], len(start) - 1
    out = torch.full((reps, g, m), float("nan"), dtype=F64, device=DEV)
    cnt = torch.full((reps, u), -1, dtype=I32, device=DEV) if counts else None
    rc = _lib().r50_op_bootstrap_sums(vd.data_ptr(), sd.data_ptr(), u, g, m, r0, reps, seed, window, out.data_ptr(),
                                      None if cnt is None else cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib().r50_last_error(None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def _ulps(got, want):
    """The distance in fp64 ulps, element by element (both finite or bit-equal)."""
    a, b = got.view(np.int64).copy(), want.view(np.int64).copy()
    a[a < 0] = np.iinfo(np.int64).min - a[a < 0]
    b[b < 0] = np.iinfo(np.int64).min - b[b < 0]
    return np.abs(a - b)


def _start(strata):
    return np.concatenate([[0], np.cumsum(strata)]).astype(np.int32)


@pytest.mark.parametrize("m", [1, 7, 300])
@pytest.mark.parametrize("reps", [1, 257])
@pytest.mark.parametrize("strata", [(1,), (1, 5, 70)], ids=["U1", "strata-1-5-70"])
def test_counts_and_sums_equal_the_restatement(strata, reps, m):
    """U = 1 alone, and strata of 1, 5 and 70 (a_g = 1 and 6 are no multiples of 4: a Philox block straddles two strata); a seed with
    high bits set; v with mixed signs, zeros and, from M = 7 on, a column of the order 1e300 and one of the order 1e-300; M = 300 takes
    two column chunks."""
    start = _start(strata)
    v = unit_rows(int(start[-1]), m, 10 * m + len(strata))
    want, want_c = BR.bootstrap_sums(v, start, reps, SEED_HIGH)
    got, got_c = _op(v, start, reps, SEED_HIGH, window=16)
    assert np.array_equal(got_c, want_c)
    d = _ulps(got, want)
    print(f"strata {strata} R {reps} M {m}: max {int(d.max())} ulp, {int((d > 0).sum())} of {d.size} elements differ")
    assert np.isfinite(got).all() and d.max() <= 1
    assert np.array_equal(got.view(np.int64), want.view(np.int64))                  # observed: bit for bit


def test_the_replicate_counter_carries_into_its_high_word():
    start = _start((1, 5, 70))
    v = unit_rows(76, 7, 5)
    r0 = 2 ** 32 - 3
    want, want_c = BR.bootstrap_sums(v, start, 8, 11, r0=r0)
    got, got_c = _op(v, start, 8, 11, r0=r0)
    assert np.array_equal(got_c, want_c) and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert not np.array_equal(got_c[3], _op(v, start, 1, 11, r0=0)[1][0])          # rho = 2^32 is not rho = 0


def test_the_same_bits_under_different_launches():
    start = _start((1, 5, 70))
    v = unit_rows(76, 300, 6)
    base, base_c = _op(v, start, 10, SEED_HIGH, window=32768)
    for window in (16, 70, 1, 69):                                                 # 16: five passes over the 70-stratum; 70: exactly one
        out, cnt = _op(v, start, 10, SEED_HIGH, window=window)
        assert np.array_equal(out.view(np.int64), base.view(np.int64)) and np.array_equal(cnt, base_c), window
    a, ac = _op(v, start, 4, SEED_HIGH, r0=0, window=16)                           # chunk invariance: [0, 10) = [0, 4) + [4, 10)
    b, bc = _op(v, start, 6, SEED_HIGH, r0=4, window=16)
    assert np.array_equal(np.concatenate([a, b]).view(np.int64), base.view(np.int64)) and np.array_equal(np.concatenate([ac, bc]), base_c)
    again, again_c = _op(v, start, 10, SEED_HIGH, window=32768)
    assert np.array_equal(again.view(np.int64), base.view(np.int64)) and np.array_equal(again_c, base_c)
    alone, none = _op(v, start, 10, SEED_HIGH, window=16, counts=False)
    assert none is None and np.array_equal(alone.view(np.int64), base.view(np.int64))


def test_the_wrapper_gives_the_op_and_refuses_what_it_must():
    from implementation_phd_lab_vision_amd import bootstrap as bs
    table = bs.UnitTable.from_sizes([1, 5, 70])
    v = unit_rows(76, 7, 8)
    vd = torch.from_numpy(v).to(DEV)
    want, want_c = _op(v, table.stratum_start, 9, 5, r0=2)
    out, cnt = bs.bootstrap_sums(vd, table, 9, 5, r0=2, counts=True)
    assert out.dtype == F64 and cnt.dtype == I32 and tuple(out.shape) == (9, 3, 7) and tuple(cnt.shape) == (9, 76)
    assert np.array_equal(out.cpu().numpy().view(np.int64), want.view(np.int64)) and np.array_equal(cnt.cpu().numpy(), want_c)
    only = bs.bootstrap_sums(vd, table, 9, 5, r0=2, window=3)
    assert isinstance(only, torch.Tensor) and torch.equal(only, out)
    with pytest.raises(ValueError, match="contiguous"):
        bs.bootstrap_sums(torch.zeros((76, 14), dtype=F64, device=DEV)[:, ::2], table, 4, 0)
    with pytest.raises(ValueError, match="rows"):
        bs.bootstrap_sums(vd[:70], table, 4, 0)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp("bootstrap")
    return rd.make_results_cache(base / "features"), rd.make_preprocessed_tree(base / "videos")


@pytest.fixture(scope="module")
def heads(trees):
    from implementation_phd_lab_vision_amd import results
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    _lib()
    store = DeviceFeatureStore(str(trees[0]), subjects=[9], test_set=True, device=DEV)
    sd = lo.synthetic_head_state_dict(1024, 2, seed=2)
    g = torch.Generator().manual_seed(5)
    sd2 = {k: v + 0.02 * v.abs().mean() * torch.randn(v.shape, generator=g) if v.is_floating_point() else v for k, v in sd.items()}
    return store, sd, sd2, results.build_head(sd, DEV), results.build_head(sd2, DEV)


I_LEN, P_LEN, REPS = 4, 3, 64


def test_point_estimates_equal_the_protocol_report(heads):
    from implementation_phd_lab_vision_amd import bootstrap as bs
    from implementation_phd_lab_vision_amd.protocols import action_groups, evaluate_protocols
    store, _sd, _sd2, head, _other = heads
    names, ids = action_groups(store.item_actions())
    want = evaluate_protocols(head, store, ids, names, I_LEN, P_LEN, batch_size=4)
    for unit in bs.UNIT_KINDS:
        res = bs.evaluate_bootstrap(head, store, None, REPS, unit, 3, 0.9, I_LEN, P_LEN, batch_size=4)
        assert res["rows"] == ["all", "action mean"] + names and res["metrics"] == ["p1", "p2", "p1@1", "p2@1", "p1@3", "p2@3"]
        assert np.array_equal(res["clips"], want["clips"]) and res["clips"].sum() == rd.N_S9
        hs = [0, 2]
        exp = np.concatenate([np.concatenate([want["recon_all"][None], want["recon_mean"][None], want["recon"]]),
                              np.concatenate([want["future_all"][hs].reshape(1, 4), want["future_mean"][hs].reshape(1, 4),
                                              want["future"][:, hs].reshape(-1, 4)])], axis=1)
        rel = np.abs(res["point"] - exp) / np.abs(exp)
        print(f"unit {unit}: point estimates against evaluate_protocols, max relative difference {rel.max():.3g}")
        assert rel.max() <= 1e-12
        assert np.all(res["lo"] <= res["hi"]) and res["point"].shape == (len(names) + 2, 6)
        assert (res["design_effect"] is None) == (unit == "clip")
    assert res["units"].tolist() == [4, 4, 3]                                       # clip units: one per clip


def test_a_head_compared_with_itself_is_a_tie(heads):
    from implementation_phd_lab_vision_amd import bootstrap as bs
    store, _sd, _sd2, head, _other = heads
    res = bs.evaluate_bootstrap(head, store, None, REPS, "sequence", 3, 0.9, I_LEN, P_LEN, batch_size=4, compare=head)
    assert np.array_equal(res["point"], res["b_point"]) and np.array_equal(res["lo"], res["b_lo"])
    for name in ("diff", "diff_lo", "diff_hi", "diff_se"):
        assert np.all(res[name] == 0.0), name
    assert np.all(res["p_better"] == 0.5) and np.all(res["p_two_sided"] == 1.0)


def test_a_paired_comparison_equals_the_restatement_on_the_unit_table(heads):
    """Every number from the restatement applied to the unit table as it was uploaded.  Exact, but for the two standard errors, whose
    reduction over R is the library's: 64 ulp * log2(R + 1) relative, as in tests/test_bootstrap_cpu.py."""
    from implementation_phd_lab_vision_amd import bootstrap as bs
    store, _sd, _sd2, head, other = heads
    res = bs.evaluate_bootstrap(head, store, None, REPS, "sequence", 3, 0.9, I_LEN, P_LEN, batch_size=4, compare=other)
    v, table, k = res["unit_table"], res["table"], 6
    assert v.shape == (11, 2 * k + 1) and v[:, -1].sum() == rd.N_S9
    sums, _ = BR.bootstrap_sums(v, table.stratum_start, REPS, 3)
    want = BR.statistics(sums, BR.point_sums(v, table.stratum_start), 0.9, pairs=k)
    got = {"point": np.concatenate([res["point"], res["b_point"]], axis=1), "lo": np.concatenate([res["lo"], res["b_lo"]], axis=1),
           "hi": np.concatenate([res["hi"], res["b_hi"]], axis=1), "se": np.concatenate([res["se"], res["b_se"]], axis=1)}
    got.update({name: res[name] for name in ("diff", "diff_se", "diff_lo", "diff_hi", "p_better", "p_two_sided")})
    for name in ("point", "lo", "hi", "diff", "diff_lo", "diff_hi", "p_better", "p_two_sided"):
        assert np.array_equal(got[name], want[name]), name
    bound = 64 * np.finfo(np.float64).eps * np.log2(REPS + 1)
    for name in ("se", "diff_se"):
        assert np.all(np.abs(got[name] - want[name]) <= bound * np.abs(want[name])), name
    assert np.any(res["diff"] != 0.0) and np.any(res["diff_hi"] > res["diff_lo"])
    lines = bs.bootstrap_lines(res)
    assert len(lines) == 1 + 2 + 3 + 1 and "design effect" in lines[-1] and "paired: B - A" in lines[0]


def _cli(*argv, timeout=600):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "implementation_phd_lab_vision_amd.results", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"results exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


def test_cli_prints_the_lines_and_writes_the_keys_only_with_the_flags(heads, trees, tmp_path):
    from implementation_phd_lab_vision_amd import bootstrap as bs
    store, sd, sd2, head, other = heads
    torch.save(sd, tmp_path / "a.pt")
    torch.save(sd2, tmp_path / "b.pt")
    base = ["--features_root", str(trees[0]), "--preprocessed_root", str(trees[1]), "--model_path", str(tmp_path / "a.pt"),
            "--seq-len", str(rd.SEQ_LEN), "--batch-size", "4", "--save-n", "2", "--video-size", "32", "--video-reader",
            "tests.results_data:read_video", "--input-len", str(I_LEN), "--pred-len", str(P_LEN)]
    r = _cli(*base, "--out", str(tmp_path / "with.npz"), "--bootstrap", str(REPS), "--bootstrap-seed", "3", "--bootstrap-level", "0.9",
             "--compare", str(tmp_path / "b.pt"))
    res = bs.evaluate_bootstrap(head, store, None, REPS, "sequence", 3, 0.9, I_LEN, P_LEN, compare=other)
    printed = [line for line in r.stdout.splitlines() if line.lstrip().startswith("Bootstrap |")]
    assert printed == bs.bootstrap_lines(res)
    z = np.load(tmp_path / "with.npz", allow_pickle=True)
    keys = bs.bootstrap_npz(res)
    assert {f for f in z.files if f.startswith("bootstrap_")} == set(keys) and "bootstrap_p_better" in keys
    for name, want in keys.items():
        assert np.array_equal(z[name], want), name
    plain = _cli(*base, "--out", str(tmp_path / "without.npz"))
    assert "Bootstrap" not in plain.stdout
    assert not [f for f in np.load(tmp_path / "without.npz", allow_pickle=True).files if f.startswith("bootstrap")]
