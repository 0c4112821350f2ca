"""Forecast baselines without a GPU: the ``results`` flags and their parse errors, the printed lines and the
``.npz`` keys from a hand-made result, and the self-checks of tests/baselines_reference.py that the GPU tests lean on."""
import numpy as np
import pytest

from tests import baselines_reference as br

BASE = ["--features_root", "f", "--preprocessed_root", "p", "--model_path", "m"]
NEW_FLAGS = ("baselines", "baseline_anchor", "nn_k", "nn_subjects", "nn_features_root", "nn_max_clips")


# ------------------------------------------------------------------ parser ----------------------------------------------------
def test_flags_are_absent_unless_given():
    from implementation_phd_lab_vision_amd import results
    args = results.parse_args(BASE + ["--pred-len", "5", "--input-len", "3", "--seq-len", "8"])
    assert not any(hasattr(args, f) for f in NEW_FLAGS)
    args = results.parse_args(BASE + ["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--baselines"])
    assert args.baselines == [] and not any(hasattr(args, f) for f in NEW_FLAGS[1:])
    assert results.baseline_options(args) == (("const_pose", "const_vel", "nn"), "pred", 1)
    args = results.parse_args(BASE + ["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--baselines", "nn", "const_pose", "nn",
                                      "--baseline-anchor", "gt", "--nn-k", "8", "--nn-subjects", "1", "5", "--nn-features-root", "d",
                                      "--nn-max-clips", "7"])
    assert results.baseline_options(args) == (("const_pose", "nn"), "gt", 8)
    assert (args.nn_subjects, args.nn_features_root, args.nn_max_clips) == ([1, 5], "d", 7)
    from implementation_phd_lab_vision_amd import baselines
    assert results.BASELINE_NAMES == baselines.BASELINES


@pytest.mark.parametrize("argv,msg", [
    (["--baselines"], "--baselines needs --pred-len"),
    (["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--baselines", "nn", "--nn-subjects", "1", "9"], "overlaps --test-subjects"),
    (["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--baselines", "--test-subjects", "1"], "overlaps --test-subjects"),
    (["--pred-len", "5", "--input-len", "1", "--seq-len", "8", "--baselines"], "const_vel needs --input-len >= 2"),
    (["--pred-len", "5", "--input-len", "1", "--seq-len", "8", "--baselines", "const_vel"], "const_vel needs --input-len >= 2"),
    (["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--baselines", "--nn-k", "9"], "--nn-k must lie in [1, 8]"),
    (["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--baselines", "--nn-k", "0"], "--nn-k must lie in [1, 8]"),
    (["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--baselines", "--nn-max-clips", "0"], "--nn-max-clips must be >= 1"),
    (["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--nn-k", "2"], "--nn-k needs --baselines"),
    (["--pred-len", "5", "--input-len", "3", "--seq-len", "8", "--baselines", "median"], "invalid choice"),
])
def test_parse_errors(argv, msg, capsys):
    from implementation_phd_lab_vision_amd import results
    with pytest.raises(SystemExit) as e:
        results.parse_args(BASE + argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_input_len_1_is_fine_without_const_vel():
    from implementation_phd_lab_vision_amd import results
    args = results.parse_args(BASE + ["--pred-len", "5", "--input-len", "1", "--seq-len", "8", "--baselines", "const_pose", "nn"])
    assert results.baseline_options(args)[0] == ("const_pose", "nn")


# ------------------------------------------------------------------ lines and arrays ------------------------------------------
def _hand_made(p=12, g=2):
    rng = np.random.default_rng(4)
    names = ("model", "const_pose", "nn")
    res = {"names": names, "group_names": ["sit", "walk"], "clips": np.array([3, 8], dtype=np.int64), "anchor": "gt", "nn_k": 2,
           "nn_dist2_mean": 123.456789}
    for i, n in enumerate(names):
        res[n] = {"mpjpe": rng.random(p) * 0.1 + 0.05 * i, "p1": rng.random(p) * 0.1 + 0.05 * i, "p2": rng.random(p) * 0.05,
                  "per_action": rng.random((g, p, 2))}
    return res


def _numbers(line, key):
    """{'@h' or 'mean': value} of one metric of a printed line."""
    part = [s for s in line.split(f"{key} (mm) ")[1].split(" | ")]
    out = {}
    for tok in part:
        if ": " not in tok or tok.startswith(("mpjpe", "p1", "p2", "model")):
            break
        name, val = tok.split(": ")
        out[name] = float(val)
        if name == "mean":
            break
    return out


def test_lines_and_arrays_from_a_hand_made_result():
    from implementation_phd_lab_vision_amd import baselines
    res = _hand_made()
    lines = baselines.baseline_lines(res, 3, 12)
    assert len(lines) == 4 and lines[0] == ("Baselines | input 3 | pred 12 | clips 11 | anchor gt | predictors 3 | nn k 2 | "
                                            "nn strip dist2 mean 123.457")
    assert [l.split(" | ")[0] for l in lines[1:]] == ["  model", "  const_pose", "  nn"]
    for line, name in zip(lines[1:], res["names"]):
        for key in ("mpjpe", "p1", "p2"):
            got = _numbers(line, key)
            assert list(got) == ["@1", "@5", "@10", "@12", "mean"]
            for h in (1, 5, 10, 12):
                assert got[f"@{h}"] == float(f"{res[name][key][h - 1] * 1000.0:.2f}")
            assert got["mean"] == float(f"{res[name][key].mean() * 1000.0:.2f}")
        if name == "model":
            assert "skill" not in line
        else:
            skill = 1.0 - res["model"]["p1"].mean() / res[name]["p1"].mean()
            assert line.endswith(f" | model skill on p1: {skill:+.4f}")
    short = baselines.baseline_lines({**res, "names": ("model", "const_pose")}, 3, 4)
    assert "nn k" not in short[0] and "@10" not in short[1] and "@4: " in short[1] and len(short) == 3

    z = baselines.baseline_arrays(res)
    assert set(z) == {"baseline_names", "baseline_mpjpe", "baseline_p1", "baseline_p2", "baseline_actions", "baseline_per_action",
                      "baseline_anchor"}
    assert z["baseline_names"].tolist() == list(res["names"]) and z["baseline_actions"].tolist() == ["sit", "walk"]
    assert str(z["baseline_anchor"]) == "gt" and z["baseline_per_action"].shape == (3, 2, 12, 2)
    for key in ("mpjpe", "p1", "p2"):
        assert z["baseline_" + key].dtype == np.float32 and z["baseline_" + key].shape == (3, 12)
        for i, n in enumerate(res["names"]):
            assert np.array_equal(z["baseline_" + key][i], res[n][key].astype(np.float32))
    assert np.array_equal(z["baseline_per_action"][2], res["nn"]["per_action"].astype(np.float32))


# ------------------------------------------------------------------ the reference's self-checks -------------------------------
def test_search_oracle_against_brute_force_with_ties():
    x = br.rows16((60, 32), 1)
    x[7] = x[3]
    x[41] = x[3]                                               # equal scores: the smaller index first
    q = br.rows16((9, 32), 2)
    q[0] = x[3]
    idx, score, dist2 = br.search(q, x, 5)
    assert np.array_equal(idx, br.brute_force(q, x, 5))
    assert idx[0, :3].tolist() == [3, 7, 41] and dist2[0, 0] == 0.0 and np.all(np.diff(score, axis=1) >= 0)
    assert not br.separated(q, x, 5)[0]                        # tied rows are never "separated"


@pytest.mark.parametrize("d,n,nq,precision", [(64, 1000, 48, "fp16"), (1024, 200, 8, "fp16"), (64, 300, 8, "bf16"), (1024, 100, 4, "bf16")])
def test_bound_covers_the_fp32_emulated_error(d, n, nq, precision):
    x, q = br.rows16((n, d), 0, precision), br.rows16((nq, d), 1, precision)
    x[5] = (x[5].float() * 30.0).to(x.dtype)                   # one row of large norm
    err = np.abs(br.fp32_scores(q, x).astype(np.float64) - br.true_scores(q, x))
    e = br.bound_e(q, x)
    print(f"d {d} {precision}: largest fp32 error / bound {np.max(err / e):.3e}")
    assert np.all(err <= e)


@pytest.mark.parametrize("d,n,nq,k", [(64, 1000, 48, 4), (256, 3000, 80, 1)])
def test_index_cases_stay_inside_the_cap(d, n, nq, k):
    """The index check may leave out at most 5 % of the queries: these cases, by the oracle alone."""
    x, q = br.rows16((n, d), 0), br.rows16((nq, d), 1)
    out = int((~br.separated(q, x, k)).sum())
    print(f"d {d} n {n} nq {nq} k {k}: {out} of {nq} queries left out")
    assert out <= 0.05 * nq


def test_forecast_restatement_on_a_hand_case():
    a1 = np.array([[[1.0, 2.0, 3.0], [0.5, 0.25, -1.0]]], dtype=np.float32)
    a0 = np.array([[[0.5, 2.0, 4.0], [0.5, 0.0, -1.5]]], dtype=np.float32)
    dbj = np.zeros((2, 4, 2, 3), dtype=np.float32)
    dbj[0, 1] = [[10, 10, 10], [11, 11, 11]]
    dbj[0, 2] = [[12, 10, 10], [13, 11, 12]]
    dbj[1, 1] = [[0, 0, 0], [1, 1, 1]]
    dbj[1, 2] = [[4, 0, 0], [1, 3, 1]]
    out = br.forecasts(a1, a0, np.array([[0, 1]]), dbj, 2, 2, ("const_pose", "const_vel", "nn"))
    assert np.array_equal(out["const_pose"][0, 1], a1[0])
    assert np.array_equal(out["const_vel"][0, 1], a1[0] + 2 * (a1[0] - a0[0]))
    # horizon 0 = frame 2, relative to each clip's root at frame 1: clip 0 [[2,0,0],[3,1,2]], clip 1 [[4,0,0],[1,3,1]]; mean, + a1 root
    assert np.array_equal(out["nn"][0, 0], np.array([[3, 0, 0], [2, 2, 1.5]], dtype=np.float32) + a1[0, 0])
    assert "const_vel" not in br.forecasts(a1, None, np.array([[0]]), dbj, 2, 1, ("nn",))
