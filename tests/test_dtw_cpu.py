"""The forecast error after dynamic time warping without a GPU: the numpy oracle's properties (exact zeros
on equal and on plateau inputs, the tie rule, warped <= plain, the band, single rows and columns, the sign of the lag), the
accumulator's layout and aggregation, the results CLI's ``--dtw`` flags and its printed lines / ``.npz`` arrays from a hand-made result,
the wrapper's refusals, and the exported symbol."""
import numpy as np
import pytest
import torch

from implementation_phd_lab_vision_amd import dtw, results
from tests import dtw_reference as dr

J = 17


def _inputs(seed, b, p, q, t, i0, j=J, similarity=False):
    rng = np.random.default_rng(seed)
    gt = dr.walk_clips(rng, b, t, j)
    return dr.slowed_predictions(rng, gt, i0, p, q, similarity), gt


def test_equal_inputs_cost_nothing_and_walk_the_diagonal():
    rng = np.random.default_rng(0)
    gt = dr.walk_clips(rng, 2, 9, J)
    i0, p = 2, 6
    results_, clip_out, path_out, margins = dr.dtw_batch(gt[:, i0:i0 + p], gt, i0, p)
    for r in results_:
        assert r[0]["total"] == 0.0 and r[0]["L"] == p and r[0]["path"] == [(k, k) for k in range(p)]
        assert r[1]["total"] < 1e-12 * p
        assert np.array_equal(r[0]["cells"], np.ones(p)) and np.array_equal(r[0]["lag_sum"], np.zeros(p))
    assert clip_out.shape == (2, 2, 2 + 3 * p) and path_out.shape == (2, 2, 2 * p - 1, 2) and (path_out[:, 0, p:] == -1).all()
    assert (margins[:, 0] > 0).all()


def test_exact_plateaus_follow_the_tie_rule():
    pred, gt, want = dr.plateau_inputs()
    (r1, _), c = dr.dtw_clip(pred[0], gt[0])
    assert r1["total"] == 0.0 and r1["path"] == want and r1["L"] == len(want)
    assert np.trace(c[0]) > 0.0                                        # the plain, frame-by-frame P1 is not 0
    zero = c[0] == 0.0
    assert all(zero[i, j] for i, j in want) and zero.sum() == len(want)         # exact zeros against positives decide the path
    assert c[0][~zero].min() > 1e-2 and r1["margin"] > 1e-2
    assert r1["cells"].tolist() == [1, 1, 2, 2, 1, 1] and r1["lag_sum"].tolist() == [0, 1, 1, -1, -1, 0]
    # an all-equal cost matrix: every candidate ties, so the path is the diagonal and then, P != Q, up / left along the border
    flat = dr.dtw_path(np.ones((3, 3)))
    assert flat["path"] == [(0, 0), (1, 1), (2, 2)]
    assert dr.dtw_path(np.ones((4, 2)))["path"] == [(0, 0), (1, 0), (2, 0), (3, 1)]          # diagonal first from the end, then up
    assert dr.dtw_path(np.ones((2, 4)))["path"] == [(0, 0), (0, 1), (0, 2), (1, 3)]
    nan = np.ones((3, 3))
    nan[1, 1] = np.nan                                                 # a NaN that came first is never replaced
    assert np.isnan(dr.dtw_path(nan)["total"])


@pytest.mark.parametrize("seed,p,similarity", [(1, 7, False), (2, 12, True), (3, 25, False)])
def test_warped_never_exceeds_plain(seed, p, similarity):
    pred, gt = _inputs(seed, 3, p, p, p + 3, 2, similarity=similarity)
    moved = 0
    for i in range(len(pred)):
        res, c = dr.dtw_clip(pred[i], gt[i, 2:2 + p])
        for m in (0, 1):
            plain = sum(np.diag(c[m]).tolist())                        # in the DP's own order: rounding cannot lift the warped sum above it
            assert res[m]["total"] <= plain and res[m]["total"] / res[m]["L"] <= plain / p
            assert max(p, p) <= res[m]["L"] <= 2 * p - 1
            assert res[m]["cells"].sum() == res[m]["L"] and (res[m]["cells"] >= 1).all()
            assert res[m]["cost_sum"].sum() == pytest.approx(res[m]["total"], rel=1e-13)
            moved += any(a != b for a, b in res[m]["path"])
    assert moved > 0                                                   # the inputs do warp


def test_band():
    pred, gt = _inputs(4, 2, 8, 8, 8, 0)
    for i in range(2):
        res0, c = dr.dtw_clip(pred[i], gt[i], band=0)
        free, _ = dr.dtw_clip(pred[i], gt[i], band=-1)
        wide, _ = dr.dtw_clip(pred[i], gt[i], band=8)
        for m in (0, 1):
            assert res0[m]["path"] == [(k, k) for k in range(8)] and res0[m]["L"] == 8
            assert res0[m]["total"] == sum(np.diag(c[m]).tolist())
            assert np.array_equal(res0[m]["cost_sum"], np.diag(c[m])) and not res0[m]["lag_sum"].any()
            assert wide[m]["path"] == free[m]["path"] and wide[m]["total"] == free[m]["total"]
            mid = dr.dtw_path(c[m], band=2)
            assert all(abs(a - b) <= 2 for a, b in mid["path"]) and free[m]["total"] <= mid["total"] <= res0[m]["total"]
    c = np.ones((5, 3))
    assert all(abs(a - b) <= 2 for a, b in dr.dtw_path(c, band=2)["path"])
    with pytest.raises(ValueError, match="band"):
        dr.dtw_path(c, band=1)
    with pytest.raises(ValueError, match="band"):
        dr.dtw_path(c.T, band=0)


def test_single_row_and_single_column():
    pred, gt = _inputs(5, 1, 1, 6, 6, 0)
    res, c = dr.dtw_clip(pred[0], gt[0])
    for m in (0, 1):
        assert res[m]["L"] == 6 and res[m]["path"] == [(0, j) for j in range(6)] and res[m]["margin"] == np.inf
        assert res[m]["total"] == pytest.approx(c[m].sum(), rel=1e-14) and res[m]["cells"].tolist() == [6]
        assert res[m]["lag_sum"].tolist() == [-15]
    pred, gt = _inputs(6, 1, 6, 1, 4, 3)
    res, c = dr.dtw_clip(pred[0], gt[0, 3:4])
    for m in (0, 1):
        assert res[m]["L"] == 6 and res[m]["path"] == [(i, 0) for i in range(6)]
        assert res[m]["cells"].tolist() == [1] * 6 and res[m]["lag_sum"].tolist() == list(range(6))
    one, _ = dr.dtw_clip(pred[0, :1], gt[0, :1])
    assert one[0]["L"] == 1 and one[0]["path"] == [(0, 0)] and one[0]["margin"] == np.inf


def test_a_slow_prediction_has_positive_lag_growing_with_the_horizon():
    """The prediction shows the ground truth at 0.7x speed: its frame k shows what the ground truth showed at frame 0.7 k, so it is
    0.3 k frames behind.  The last row is left out: the closed end ties it to the ground truth's last frames."""
    rng = np.random.default_rng(7)
    p = 20
    gt = dr.walk_clips(rng, 1, p, J)[0]
    pred = dr.resample(gt.astype(np.float64), np.arange(p) * 0.7).astype(np.float32)
    res, _ = dr.dtw_clip(pred, gt)
    for m in (0, 1):
        lag = res[m]["lag_sum"] / res[m]["cells"]
        assert lag[0] <= 0.5 and (lag[2:p - 1] > 0).all() and lag[:p - 1].mean() > 1.0
        assert lag[p // 4] < lag[p // 2] < lag[3 * p // 4]
        assert np.abs(lag[:p - 1] - 0.3 * np.arange(p - 1)).max() <= 1.0
    fast, _ = dr.dtw_clip(gt[::2][:8], gt[:12])                        # twice the speed: the prediction is ahead, the lag negative
    assert (fast[0]["lag_sum"][1:7] < 0).all()


def test_sums_layout_and_aggregation():
    pred, gt = _inputs(8, 5, 4, 5, 8, 2, j=5, similarity=True)
    group, g, p = np.array([2, 0, 2, 3, 0]), 5, 4
    results_, clip_out, _, _ = dr.dtw_batch(pred, gt, 2, 5)
    acc = dr.dtw_sums(clip_out, group, g)
    v = 1 + 2 * p
    assert acc.shape == (dtw.acc_size(g, p),) == (g * 2 * v + g,)
    assert acc[g * 2 * v:].tolist() == [2.0, 0.0, 2.0, 1.0, 0.0]
    for gg in range(g):
        members = [i for i in range(5) if group[i] == gg]
        for m in (0, 1):
            base = (gg * 2 + m) * v
            assert acc[base] == pytest.approx(sum(results_[i][m]["total"] / results_[i][m]["L"] for i in members), rel=1e-14, abs=0)
            for k in range(p):
                rs = [results_[i][m] for i in members]
                assert acc[base + 1 + k] == pytest.approx(sum(r["cost_sum"][k] / r["cells"][k] for r in rs), rel=1e-14, abs=0)
                assert acc[base + 1 + p + k] == pytest.approx(sum(r["lag_sum"][k] / r["cells"][k] for r in rs), rel=1e-14, abs=0)
    vals = dr.values_from_sums(acc, g, p)
    assert np.isnan(vals["dtw"][[1, 4]]).all() and np.isnan(vals["lag"][1]).all() and vals["clips"].tolist() == [2, 0, 2, 1, 0]
    assert vals["dtw_future"].shape == (g, p, 2) and vals["lag_all"].shape == (p, 2) and vals["dtw_all"].shape == (2,)
    assert np.allclose(vals["dtw_mean"], vals["dtw"][[0, 2, 3]].mean(axis=0), rtol=1e-15)
    assert vals["dtw_all"][0] == pytest.approx(sum(r[0]["total"] / r[0]["L"] for r in results_) / 5, rel=1e-14)
    assert vals["dtw_future"][3, 1, 1] == pytest.approx(results_[3][1]["cost_sum"][1] / results_[3][1]["cells"][1], rel=1e-14)
    d, da, f, fa, lag, la, clips = dtw._values(acc, g, p)              # the module's own aggregation
    for got, key in ((d, "dtw"), (da, "dtw_all"), (f, "dtw_future"), (fa, "dtw_future_all"), (lag, "lag"), (la, "lag_all"), (clips, "clips")):
        assert got.shape == vals[key].shape and np.array_equal(got, vals[key], equal_nan=True), key


# ------------------------------------------------------------------ CLI -------------------------------------------------------
BASE = ["--features_root", "F", "--preprocessed_root", "P", "--model_path", "M"]


def test_parse_dtw_flags(capsys):
    a = results.parse_args(BASE)
    assert a.dtw is False and a.dtw_band == -1
    a = results.parse_args(BASE + ["--dtw", "--pred-len", "25"])
    assert (a.dtw, a.dtw_band, a.pred_len, a.protocols) == (True, -1, 25, False)
    a = results.parse_args(BASE + ["--dtw", "--dtw-band", "4", "--seq-len", "8", "--input-len", "3", "--pred-len", "5"])
    assert (a.dtw, a.dtw_band, a.input_len, a.pred_len) == (True, 4, 3, 5)
    with pytest.raises(SystemExit) as e:
        results.parse_args(BASE + ["--dtw"])
    assert e.value.code != 0 and "--dtw needs --pred-len" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        results.parse_args(BASE + ["--dtw", "--seq-len", "80", "--pred-len", "65"])          # the op's limit
    assert results.parse_args(BASE + ["--dtw", "--seq-len", "80", "--pred-len", "64"]).pred_len == 64


def _fake_result(p_len, band=-1):
    fut = np.linspace(0.01, 0.2, 2 * p_len * 2).reshape(2, p_len, 2)
    lag = np.linspace(-0.5, 3.0, 2 * p_len * 2).reshape(2, p_len, 2)
    w = np.array([3, 1])[:, None, None] / 4
    return {"group_names": ["Directions", "Walking"], "clips": np.array([3, 1], dtype=np.int64), "band": band,
            "dtw": np.array([[0.05, 0.04], [0.07, 0.05]]), "dtw_all": np.array([0.055, 0.0425]), "dtw_mean": np.array([0.06, 0.045]),
            "dtw_future": fut, "dtw_future_all": (fut * w).sum(0), "lag": lag, "lag_all": (lag * w).sum(0),
            "plain_future_all": (fut * w).sum(0) * 1.5, "plain_all": np.array([0.0801, 0.0602])}


def test_dtw_lines_and_arrays():
    res = _fake_result(12)
    lines = dtw.dtw_lines(res, 3, 12)
    assert lines[0] == ("DTW metrics | input 3 | pred 12 | band none | clips 4 | all: p1 (mm) 55.00 | p2 (mm) 42.50 | plain p1 (mm) 80.10 "
                        "| p2 (mm) 60.20")
    assert lines[1:3] == ["  Directions | clips 3 | dtw p1 (mm) 50.00 | dtw p2 (mm) 40.00",
                          "  Walking | clips 1 | dtw p1 (mm) 70.00 | dtw p2 (mm) 50.00"]
    assert len(lines) == 4 and lines[3].startswith("DTW horizons | p1 (mm) @1: ")
    fa, la = res["dtw_future_all"] * 1000.0, res["lag_all"]
    assert f"@10: {fa[9, 0]:.2f} | @12: {fa[11, 0]:.2f} | p2 (mm) @1: {fa[0, 1]:.2f}" in lines[3]
    assert f"lag p1 (frames) @1: {la[0, 0]:+.2f} | @5: {la[4, 0]:+.2f}" in lines[3] and f"lag p2 (frames) @1: {la[0, 1]:+.2f}" in lines[3]
    assert "@25" not in lines[3] and lines[3].count("@") == 16
    assert " -0." in lines[3] and " +" in lines[3]                      # the lag carries its sign
    assert "band 4 |" in dtw.dtw_lines(_fake_result(3, band=4), 2, 3)[0]
    assert dtw.dtw_lines(_fake_result(3), 2, 3)[-1].count("@") == 8                  # horizons 1 and 3, four series

    arr = dtw.dtw_arrays(res)
    assert set(arr) == {"dtw_actions", "dtw_clips", "dtw", "dtw_all", "dtw_future", "dtw_future_all", "dtw_lag", "dtw_lag_all", "dtw_band"}
    assert arr["dtw_actions"].dtype.kind == "U" and arr["dtw_actions"].tolist() == ["Directions", "Walking"]
    assert arr["dtw_clips"].dtype == np.int64 and arr["dtw_band"].dtype == np.int64 and int(arr["dtw_band"]) == -1
    for key, shape, src in (("dtw", (2, 2), "dtw"), ("dtw_all", (2,), "dtw_all"), ("dtw_future", (2, 12, 2), "dtw_future"),
                            ("dtw_future_all", (12, 2), "dtw_future_all"), ("dtw_lag", (2, 12, 2), "lag"), ("dtw_lag_all", (12, 2), "lag_all")):
        assert arr[key].dtype == np.float32 and arr[key].shape == shape and np.array_equal(arr[key], res[src].astype(np.float32)), key


# ------------------------------------------------------------------ wrapper ---------------------------------------------------
def test_add_dtw_sums_refusals_that_need_no_gpu():
    p, q, t = 3, 4, 6
    pred, gt = torch.zeros(2, p, J, 3), torch.zeros(2, t, J, 3)
    grp = torch.zeros(2, dtype=torch.int32)
    acc = torch.zeros(dtw.acc_size(1, p), dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        dtw.add_dtw_sums(pred, gt, 0, q, grp, 1, acc)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        dtw.add_dtw_sums(pred, gt, 0, q, torch.tensor([0, 1], dtype=torch.int32), 1, acc)
    with pytest.raises(ValueError, match="band"):
        dtw.add_dtw_sums(pred, gt, 0, q, grp, 1, acc, band=0)                               # below |P - Q| = 1
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt, 3, q, grp, 1, acc)                                       # i0 + Q > T
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt, 0, 0, grp, 1, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(torch.zeros(2, 65, J, 3), torch.zeros(2, 70, J, 3), 0, 4, grp, 1, torch.zeros(dtw.acc_size(1, 65), dtype=torch.float64))
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred.double(), gt, 0, q, grp, 1, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt, 0, q, grp.long(), 1, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt, 0, q, grp, 1, acc[:-1])
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt, 0, q, grp, 1, acc, root=J)
    with pytest.raises(ValueError, match="clip_out"):
        dtw.add_dtw_sums(pred, gt, 0, q, grp, 1, acc, clip_out=torch.zeros(2, 2, 3 * p, dtype=torch.float64))
    with pytest.raises(ValueError, match="path_out"):
        dtw.add_dtw_sums(pred, gt, 0, q, grp, 1, acc, path_out=torch.zeros(2, 2, p + q, 2, dtype=torch.int32))


def test_library_refuses_bad_arguments_without_a_gpu(lib_built):
    """The argument checks come before any launch: they answer on a machine without a GPU as well, and name the op."""
    assert lib_built.r50_op_dtw_protocols(None, None, None, 1, 3, 3, 0, 3, 17, 0, -1, 1, None, None, None, None) != 0
    assert b"r50_op_dtw_protocols" in lib_built.r50_last_error(None)
    buf = torch.zeros(4096, dtype=torch.float64)
    ptr = buf.data_ptr()
    for p, q, band in ((65, 3, -1), (3, 65, -1), (0, 3, -1), (5, 3, 1)):
        assert lib_built.r50_op_dtw_protocols(ptr, ptr, ptr, 1, p, 70, 0, q, 17, 0, band, 1, ptr, None, ptr, None) != 0, (p, q, band)
        assert b"r50_op_dtw_protocols" in lib_built.r50_last_error(None)
    assert not buf.any()
