"""Resampling of pose sequences on the MI355X (INTEGRATION.md section AB): ``r50_op_resample_sequences`` against the numpy restatement
tests/resample_reference.py on one ragged table (every case and every tangent branch of include/r50_resample.h), shifted stamps,
``predict --resample`` end to end and ``evaluate_holdout`` against its written-out composition."""
import re

import numpy as np
import pytest
import torch

from implementation_phd_lab_vision_amd import model, predict, resample, smooth
from tests import bvh_reader
from tests import resample_reference as RR
from tests import results_data as rd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def ulps(a, b):
    """The distance of two fp32 arrays in units in the last place, on the ordered-integer line (+0 and -0 coincide)."""
    def line(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(line(a) - line(b))


def bits(v):
    return np.ascontiguousarray(v).view(np.int32)


# ---------------------------------------------------------------- the op -------------------------------------------------------------
_REFERENCE = {}


def _case(joints):
    """The ragged case and the reference's answers for both kinds, computed once and shared."""
    if joints not in _REFERENCE:
        c = RR.ragged_case(joints, seed=joints)
        c["want"] = {kind: RR.resample(c["x"], c["idx"], c["seq_start"], c["out_time"], c["out_seq"], c["out_left"], kind, c["max_gap"])
                     for kind in ("linear", "cubic")}
        for v in c["want"].values():
            for a in v:
                a.setflags(write=False)
        _REFERENCE[joints] = c
    return _REFERENCE[joints]


@pytest.mark.parametrize("kind", ["linear", "cubic"])
@pytest.mark.parametrize("joints", [17, 1, 3, 64])
def test_the_op_is_the_reference_on_a_ragged_table(lib, joints, kind):
    c = _case(joints)
    want, want_flags = c["want"][kind]
    table = resample.ResampleTable(c["seq_start"], c["idx"], c["out_time"], c["out_seq"], c["out_left"])
    x = torch.from_numpy(c["x"]).to(DEV)
    y, flags = resample.resample_sequences(x, table, kind, c["max_gap"])
    again, flags_again = resample.resample_sequences(x, table, kind, c["max_gap"])
    torch.cuda.synchronize()
    y, flags = y.cpu().numpy(), flags.cpu().numpy()
    assert y.shape == (c["g"], joints, 3) and y.dtype == np.float32 and flags.dtype == np.int32
    d = ulps(y, want)
    print(f"J={joints} {kind}: max distance to the reference {int(d.max())} ulp over {d.size} values, {int((d > 0).sum())} differ")
    assert np.array_equal(flags, want_flags)
    assert d.max() <= 1
    copied = (want_flags != 0) | (c["out_time"] == c["idx"][c["out_left"]])
    assert copied.sum() > c["f"] and np.array_equal(bits(y[copied]), bits(want[copied]))       # knot, break and outside rows: the source row's bits
    src = np.where(want_flags == RR.IN_BREAK, -1, c["out_left"])
    plain = copied & (src >= 0)
    assert np.array_equal(bits(y[plain]), bits(c["x"][src[plain]]))
    assert np.array_equal(bits(y), bits(again.cpu().numpy())) and np.array_equal(flags, flags_again.cpu().numpy())
    assert not (np.signbit(y[~copied]) & (y[~copied] == 0)).any(), "an interpolated element stores no -0"


@pytest.mark.parametrize("shift", [-(2 ** 30), 2 ** 30 - 2000])
def test_shifted_stamps_give_the_same_poses(lib, shift):
    """Stamps near +-2^30: the stamp differences and tau - idx[i] are exact in fp64 (the times are multiples of 2^-16), so the result
    holds the bits of the same table at 0."""
    base, far = RR.ragged_case(17, seed=4, quantum=2.0 ** -16), RR.ragged_case(17, seed=4, quantum=2.0 ** -16, shift=shift)
    assert np.array_equal(far["out_left"], base["out_left"]) and np.array_equal(far["out_time"] - shift, base["out_time"])
    assert np.abs(far["idx"]).max() > 2 ** 30 - 2100
    x = torch.from_numpy(base["x"]).to(DEV)
    for kind in ("linear", "cubic"):
        got = []
        for c in (base, far):
            table = resample.ResampleTable(c["seq_start"], c["idx"], c["out_time"], c["out_seq"], c["out_left"])
            y, flags = resample.resample_sequences(x, table, kind, c["max_gap"])
            got.append((y.cpu().numpy(), flags.cpu().numpy()))
        assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and np.array_equal(got[0][1], got[1][1])
        want, want_flags = RR.resample(far["x"], far["idx"], far["seq_start"], far["out_time"], far["out_seq"], far["out_left"], kind, far["max_gap"])
        assert ulps(got[1][0], want).max() <= 1 and np.array_equal(got[1][1], want_flags)


def test_refusals_on_the_device(lib):
    c = _case(3)
    table = resample.ResampleTable(c["seq_start"], c["idx"], c["out_time"], c["out_seq"])
    x = torch.from_numpy(c["x"]).to(DEV)
    for bad, match in ((x[:-1], "rows"), (x.double(), "fp32"), (x[:, :, :2], "fp32 expected"), (x.transpose(0, 1).contiguous().transpose(0, 1), "contiguous")):
        with pytest.raises(ValueError, match=match):
            resample.resample_sequences(bad, table, "cubic", 3)
    with pytest.raises(ValueError, match="max_gap"):
        resample.resample_sequences(x, table, "cubic", 0)


# ---------------------------------------------------------------- predict ------------------------------------------------------------
N, H, W, T, STRIDE = 23, 64, 48, 8, 3


@pytest.fixture(scope="module")
def head():
    from oracle.lifting_oracle import synthetic_head_state_dict
    return model.PHDFor3DJoints(64, 17, 2, precision="fp16").load_state_dict(synthetic_head_state_dict(64, 2, seed=1)).to(DEV).eval()


@pytest.fixture(scope="module")
def backbone(lib):
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_state_dict
    bb = ResNet50Backbone(state_dict=synthetic_state_dict(0), max_batch=16).to(DEV).eval()
    yield bb
    bb.close()


@pytest.fixture(scope="module")
def video():
    return torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8).numpy()


def _video_reference(joints3d, frame_idx, step, kind, skip):
    tau = np.arange(int(frame_idx[-1] / step) + 2) * step
    tau = tau[tau <= frame_idx[-1]]
    t = RR.table([0, len(frame_idx)], frame_idx, tau, np.zeros(tau.size, dtype=np.int32))
    return tau, RR.resample(joints3d, t["idx"], t["seq_start"], t["out_time"], t["out_seq"], t["out_left"], kind, skip)


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_predict_with_resample_keeps_the_knots_and_fills_the_frames_between(backbone, head, video):
    p = predict.VideoPredictor(backbone, head, seq_len=T, stride=STRIDE, frame_batch=16)
    plain = p.predict(video, frame_skip=2)
    res = p.predict(video, frame_skip=2, resample=resample.ResampleSettings(1.0))
    assert set(res) - set(plain) == {"resampled3d", "resampled_time", "resampled_flags", "resample", "bone_std_mm", "resampled_bone_std_mm"}
    for key in plain:
        assert res[key] == plain[key] if key == "stats" else _same_bytes(res[key], plain[key]), key
    n = plain["joints3d"].shape[0]
    assert n == 12 and res["frame_idx"].tolist() == list(range(0, N, 2)) and res["resampled3d"].shape == (N, 17, 3)
    assert res["resampled_time"].dtype == np.float64 and res["resampled_time"].tolist() == [float(v) for v in range(N)]
    assert not res["resampled_flags"].any() and str(res["resample"]) == "step=1 kind=cubic"
    assert np.array_equal(bits(res["resampled3d"][::2]), bits(res["joints3d"]))
    tau, (want, _) = _video_reference(res["joints3d"], res["frame_idx"], 1.0, "cubic", 2)
    d = ulps(res["resampled3d"][1::2], want[1::2])
    print(f"predict --resample 1: odd frames against the reference, max {int(d.max())} ulp")
    assert d.max() <= 1 and np.array_equal(tau, res["resampled_time"])
    assert not np.array_equal(res["resampled3d"][1], res["resampled3d"][0])
    # without --fix-bones the file says what interpolation did to the bone lengths: both figures are bone_stats' own
    for key, poses in (("bone_std_mm", res["joints3d"]), ("resampled_bone_std_mm", res["resampled3d"])):
        rows = poses.shape[0]
        tables = smooth.DeviceTables(np.array([0, rows], dtype=np.int32), np.arange(rows, dtype=np.int32), DEV)
        stats = smooth.bone_stats(torch.from_numpy(poses).to(DEV), tables).cpu().numpy()
        assert float(res[key]) == smooth.bone_std_mm(stats, np.array([rows]), np.array([0]), 1)[1] and float(res[key]) > 0.0
    # another step and the linear kind: 30 fps out of 25
    step = 2 * 25 / 30
    lin = p.predict(video, frame_skip=2, resample=resample.ResampleSettings(step, "linear"))
    tau, (want, want_flags) = _video_reference(lin["joints3d"], lin["frame_idx"], step, "linear", 2)
    assert np.array_equal(lin["resampled_time"], tau) and tau.size == 14 and np.array_equal(lin["resampled_flags"], want_flags)
    assert ulps(lin["resampled3d"], want).max() <= 1 and _same_bytes(lin["joints3d"], plain["joints3d"])


def test_predict_with_fix_bones_rebuilds_the_resampled_rows(backbone, head, video):
    p = predict.VideoPredictor(backbone, head, seq_len=T, stride=STRIDE, frame_batch=16)
    post = smooth.PostProcess(kind="gauss", fix_bones=True)
    plain = p.predict(video, frame_skip=2, post=post)
    res = p.predict(video, frame_skip=2, post=post, resample=resample.ResampleSettings(1.0))
    assert set(res) - set(plain) == {"resampled3d", "resampled_time", "resampled_flags", "resample"}
    for key in plain:
        assert res[key] == plain[key] if key == "stats" else _same_bytes(res[key], plain[key]), key
    # the composition: the op on the poses of the file, then fix_bone_lengths over the resampled rows as one sequence
    table = resample.ResampleTable([0, 12], res["frame_idx"], np.arange(N, dtype=np.float64), np.zeros(N, dtype=np.int32))
    y, _ = resample.resample_sequences(torch.from_numpy(res["joints3d"]).to(DEV), table, "cubic", 2)
    tables = smooth.DeviceTables(np.array([0, N], dtype=np.int32), np.arange(N, dtype=np.int32), DEV)
    want, stats = smooth.fix_bone_lengths(y, tables)
    assert np.array_equal(bits(res["resampled3d"]), bits(want.cpu().numpy()))
    # the spread of the bone lengths is what fix_bone_lengths leaves: the store's rounding, and less than interpolation alone leaves
    e = np.asarray(smooth.H36M_EDGES)
    length = lambda v: np.linalg.norm(v[:, e[:, 1]].astype(np.float64) - v[:, e[:, 0]].astype(np.float64), axis=2)          # noqa: E731
    bar = 2.0 * np.sqrt(3.0) * float(np.spacing(np.float32(np.abs(res["resampled3d"]).max())))
    spread = np.abs(length(res["resampled3d"]) - stats.cpu().numpy()[0, :, 0]).max()
    print(f"--fix-bones --resample: bone lengths within {spread:.3e} of the means (bar {bar:.3e}); interpolation alone "
          f"{np.abs(length(y.cpu().numpy()) - stats.cpu().numpy()[0, :, 0]).max():.3e}")
    assert spread <= bar


def test_cli_writes_the_resampled_sequence_and_its_bvh(tmp_path, backbone, head, video, capsys):
    from oracle.lifting_oracle import synthetic_head_state_dict
    np.save(tmp_path / "clip.npy", video)
    torch.save(synthetic_head_state_dict(64, 2, seed=1), tmp_path / "head.pt")
    step = 0.5
    written = predict.main(["--frames", str(tmp_path / "clip.npy"), "--model_path", str(tmp_path / "head.pt"), "--synthetic-weights",
                            "--seq-len", str(T), "--stride", str(STRIDE), "--frame-skip", "2", "--frame-batch", "16", "--out",
                            str(tmp_path / "out"), "--resample", str(step), "--resample-kind", "linear", "--bvh", "--bvh-fps", "20"])
    assert written == [str(tmp_path / "out" / "clip_poses.npz"), str(tmp_path / "out" / "clip.bvh")]
    z = np.load(written[0])
    want = predict.VideoPredictor(backbone, head, seq_len=T, stride=STRIDE, frame_batch=16).predict(
        video, frame_skip=2, resample=resample.ResampleSettings(step, "linear"))
    for key in ("joints3d", "frame_idx", "resampled3d", "resampled_time", "resampled_flags", "bone_std_mm", "resampled_bone_std_mm"):
        assert _same_bytes(z[key], np.asarray(want[key])), key
    m = z["resampled3d"].shape[0]
    assert m == 2 * 22 + 1 and str(z["resample"]) == "step=0.5 kind=linear" and z["joints3d"].shape[0] == 12
    assert z["rotations_quat"].shape == (m, 17, 4) and z["joints3d_rigid"].shape == (m, 17, 3)
    bvh = bvh_reader.parse(open(written[1]).read())
    assert bvh["frames"] == m and bvh["frame_time"] == step / (2 * 20.0)


# ---------------------------------------------------------------- the holdout report -------------------------------------------------
@pytest.fixture(scope="module")
def dense(lib, tmp_path_factory):
    from implementation_phd_lab_vision_amd import results, sequences
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    features = rd.make_results_cache(tmp_path_factory.mktemp("holdout") / "features")
    store = DeviceFeatureStore(str(features), subjects=[9], test_set=True, device=DEV)
    head = results.build_head(lo.synthetic_head_state_dict(1024, 2, 4), DEV)
    return sequences.evaluate_dense(head, store, fuse="context", keep_poses=True)


@pytest.mark.parametrize("k,kind", [(2, "cubic"), (3, "linear"), (5, "cubic")])
def test_evaluate_holdout_is_its_written_out_composition(dense, k, kind):
    from implementation_phd_lab_vision_amd import protocols, sequences
    res = resample.evaluate_holdout(dense, k, kind, DEV, keep=True)
    pred, gt = np.ascontiguousarray(dense["pred"], dtype=np.float32), np.ascontiguousarray(dense["gt"], dtype=np.float32)
    seq_start, frame_idx = np.asarray(dense["seq_start"]), np.asarray(dense["frame_idx"])
    f, n_seq, names = pred.shape[0], len(seq_start) - 1, list(dense["group_names"])
    keep = RR.holdout_rows(seq_start, frame_idx, k)
    held = np.flatnonzero(~keep)
    assert 0 < held.size < f and res["holdout_rows_all"] == held.size and res["holdout_kept_all"] == int(keep.sum())
    # index-select the kept rows, run the reference
    kept_start = np.concatenate([[0], np.cumsum([keep[seq_start[s]:seq_start[s + 1]].sum() for s in range(n_seq)])])
    seq = np.repeat(np.arange(n_seq, dtype=np.int32), np.diff(seq_start))
    t = RR.table(kept_start, frame_idx[keep], frame_idx.astype(np.float64), seq)
    want, want_flags = RR.resample(pred[keep], t["idx"], t["seq_start"], t["out_time"], t["out_seq"], t["out_left"], kind, k)
    got = res["pred_holdout"]
    assert not want_flags.any() and res["holdout_flagged"].tolist() == [0, 0]
    assert np.array_equal(bits(got[keep]), bits(pred[keep])), "kept rows are the input's bits"
    d = ulps(got, want)
    print(f"K={k} {kind}: {held.size} of {f} rows held out; interpolated rows within {int(d.max())} ulp of the reference")
    assert d.max() <= 1 and not np.array_equal(got[held], pred[held])
    # score the reference's poses with the existing launches
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)               # noqa: E731
    group = np.array([names.index(protocols.action_name(dense["seq_keys"][s][1])) for s in seq], dtype=np.int32)
    g = len(names)
    dist = np.linalg.norm(want.astype(np.float64) - pred, axis=2).mean(axis=1).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(np.asarray(dense["count"]), dtype=np.int64)]).astype(np.int32)
    part = sequences.sequence_metrics(dev(want), dev(gt), dev(dist), dev(offsets), dev(seq), dev(frame_idx.astype(np.int32)), dev(group), g)
    vals = sequences.metric_values(sequences.sum_blocks(part.cpu().numpy().reshape(-1, g, sequences.METRIC_SLOTS)), np.zeros(g))
    # one ulp of the largest coordinate moves a joint by at most sqrt(3) ulp; the means inherit that, P2's alignment at most doubles it
    bar = 4.0 * np.sqrt(3.0) * float(np.spacing(np.float32(max(np.abs(pred).max(), np.abs(gt).max()))))
    for m in ("mpjve", "accel"):
        assert abs(res["holdout_" + m + "_all"] - vals[m + "_all"]) <= 2 * bar, m
        assert np.allclose(res["holdout_" + m], vals[m], rtol=0, atol=2 * bar, equal_nan=True), m
    assert abs(res["holdout_distance_all"] - vals["spread_all"]) <= bar
    for prefix, poses in (("holdout_full_", pred), ("holdout_", want)):
        acc = torch.zeros(3 * g, dtype=torch.float64, device=DEV)
        protocols._launch(dev(poses[held]).view(-1, 1, 17, 3), dev(gt[held]).view(-1, 1, 17, 3), 0, dev(group[held]), g, acc, protocols.ROOT_JOINT)
        acc = acc.cpu().numpy()
        sums, count = acc[:2 * g].reshape(g, 2), acc[2 * g:]
        assert np.array_equal(res["holdout_rows"], count.round().astype(np.int64))
        for col, m in enumerate(("p1", "p2")):
            assert abs(res[prefix + m + "_all"] - sums[:, col].sum() / count.sum()) <= bar, prefix + m
            ok = count > 0
            assert np.allclose(res[prefix + m][ok], sums[ok, col] / count[ok], rtol=0, atol=bar), prefix + m
    assert res["holdout_p1_all"] != res["holdout_full_p1_all"]
    # the printed lines parse, and carry these numbers
    lines = resample.holdout_lines(dense, res)
    assert len(lines) == 1 + g + 1 and all(line.startswith("Dense | holdout") for line in lines)
    head_line = re.fullmatch(r"Dense \| holdout K=(\d+) kind=(\w+) \(section AB\) \| kept rows (\d+) \| flagged rows in a break (\d+), outside the "
                             r"sequence (\d+) \| full rate -> interpolated, all: held-out rows (\d+) \| p1 \(mm\) ([-\d.naninf]+) -> ([-\d.naninf]+) \| "
                             r"p2 \(mm\) ([-\d.naninf]+) -> ([-\d.naninf]+) \| all rows: vel \(mm/frame\) ([-\d.naninf]+) -> ([-\d.naninf]+) \| "
                             r"accel \(mm/frame\^2\) ([-\d.naninf]+) -> ([-\d.naninf]+) \| distance \(mm\) ([-\d.naninf]+)", lines[0])
    assert head_line, lines[0]
    v = head_line.groups()
    assert (int(v[0]), v[1], int(v[2]), int(v[3]), int(v[4]), int(v[5])) == (k, kind, int(keep.sum()), 0, 0, held.size)
    assert v[6] == f"{res['holdout_full_p1_all'] * 1000.0:.2f}" and v[7] == f"{res['holdout_p1_all'] * 1000.0:.2f}"
    assert v[10] == f"{dense['mpjve_all'] * 1000.0:.2f}" and v[11] == f"{res['holdout_mpjve_all'] * 1000.0:.2f}"
    for line, name in zip(lines[1:-1], names):
        assert re.fullmatch(rf"Dense \| holdout   {re.escape(name)} \| held-out rows \d+ \| p1 \(mm\) .* \| distance \(mm\) [-\d.naninf]+", line), line
    assert lines[-1].startswith("Dense | holdout   action mean | p1 (mm) ")
    z = resample.holdout_npz(res)
    assert set(z) == {"dense_holdout", "dense_holdout_rows", "dense_holdout_flagged"} | {f"dense_holdout_{m}{s}" for m in
                                                                                       ("full_p1", "full_p2", "p1", "p2", "mpjve", "accel", "distance")
                                                                                       for s in ("", "_all")}
    assert set(resample.holdout_export(res)) == {"pred_holdout", "holdout"} and "pred_holdout" not in resample.evaluate_holdout(dense, k, kind, DEV)
