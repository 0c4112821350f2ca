"""The detail metrics on the MI355X: ``r50_op_pose_detail_metrics`` against the numpy fp64 oracle
(tests/detail_reference.py: sums within the protocols' bounds, hit counts exactly, on inputs the CPU suite shows to be tie-free) and
against ``r50_op_pose_protocols``, its degenerate poses, determinism, accumulation and refusals; ``detail_metrics.evaluate_detail``
against the oracle on the device's own head outputs; the results CLI's ``--detail-metrics``.  CLI runs are fresh child processes
under a time limit."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import detail_reference as dr
from tests import protocols_reference as pr
from tests import results_data as rd
from tests.rollout_reference import rollout_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(lib, pred, gt, i0, group, n_groups, root, n_thr, thr_max, acc):
    b, p, j, _ = pred.shape
    return lib.r50_op_pose_detail_metrics(pred.data_ptr(), gt.data_ptr(), group.data_ptr(), b, p, gt.shape[1], i0, j, root, n_groups,
                                          n_thr, thr_max, acc.data_ptr(), _stream())


def _run(lib, pred, gt, i0, group, n_groups, root=0, n_thr=31, thr_max=dr.THR_MAX):
    """One launch into a zeroed accumulator; pred / gt / group numpy.  Returns the fp64 sums on the host."""
    pd, gd = torch.from_numpy(np.array(pred)).to(DEV).contiguous(), torch.from_numpy(np.array(gt)).to(DEV).contiguous()
    grp = torch.as_tensor(np.array(group), dtype=torch.int32).to(DEV)
    acc = torch.zeros(dr.acc_size(n_groups, pd.shape[1], pd.shape[2]), dtype=torch.float64, device=DEV)
    assert _call(lib, pd, gd, i0, grp, n_groups, root, n_thr, thr_max, acc) == 0, lib.r50_last_error(None)
    return acc.cpu().numpy()


def _sections(acc, n_groups, p, j):
    a_end = 2 * n_groups * p * j
    return (acc[:a_end].reshape(n_groups, p, j, 2), acc[a_end:a_end + 6 * n_groups * p].reshape(n_groups, p, 6),
            acc[a_end + 6 * n_groups * p:])


# ------------------------------------------------------------------ kernel ----------------------------------------------------
@pytest.mark.parametrize("case", dr.CASES)
def test_kernel_matches_oracle(lib, case):
    b, p, t_gt, i0, j, n_groups, root, n_thr = case
    pred, gt, group = dr.case_inputs(case)
    got = _run(lib, pred, gt, i0, group, n_groups, root, n_thr)
    sec_a, sec_b, clips = _sections(got, n_groups, p, j)
    want_a, want_b, want_clips = _sections(dr.case_sums(case), n_groups, p, j)
    rel = np.abs(sec_a - want_a) / np.maximum(np.abs(want_a), 1e-300)
    print(f"{case}: largest relative difference of the d1 / d2 sums {rel.max():.2e}, of the ev / ea sums "
          f"{(np.abs(sec_b[..., 4:] - want_b[..., 4:]) / np.maximum(np.abs(want_b[..., 4:]), 1e-300)).max():.2e}")
    np.testing.assert_allclose(sec_a, want_a, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(sec_b[..., 4:], want_b[..., 4:], rtol=1e-9, atol=1e-12)
    assert np.array_equal(sec_b[..., :4], want_b[..., :4])            # the hit counts, exactly (the inputs are tie-free)
    counts = np.bincount(group, minlength=n_groups)
    assert np.array_equal(clips, want_clips) and np.array_equal(clips, counts.astype(np.float64))
    empty = np.flatnonzero(counts == 0)
    assert np.all(sec_a[empty] == 0.0) and np.all(sec_b[empty] == 0.0)
    assert np.all(sec_b[:, 0, 4:] == 0.0) and np.all(sec_b[:, p - 1, 5] == 0.0)      # the undefined motion slots
    if p >= 2:
        assert np.all(sec_b[counts > 0, 1:, 4] > 0.0) or j == 1
    if j == 1:                                                         # exact zeros: every positive threshold, nothing else
        assert np.all(sec_a == 0.0) and np.all(sec_b[..., 4:] == 0.0)
        assert np.array_equal(sec_b[..., 0], np.tile(counts[:, None] * (n_thr - 1.0), (1, p)))


@pytest.mark.parametrize("case", dr.CASES)
def test_agrees_with_pose_protocols(lib, case):
    b, p, t_gt, i0, j, n_groups, root, n_thr = case
    pred, gt, group = dr.case_inputs(case)
    sec_a, _, clips = _sections(_run(lib, pred, gt, i0, group, n_groups, root, n_thr), n_groups, p, j)
    pd, gd = torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV)
    grp = torch.as_tensor(np.array(group), dtype=torch.int32).to(DEV)
    acc = torch.zeros(2 * n_groups * p + n_groups, dtype=torch.float64, device=DEV)
    assert lib.r50_op_pose_protocols(pd.data_ptr(), gd.data_ptr(), grp.data_ptr(), b, p, t_gt, i0, j, root, n_groups, acc.data_ptr(),
                                     _stream()) == 0
    proto = acc.cpu().numpy()
    np.testing.assert_allclose(sec_a.sum(axis=2) / j, proto[:2 * n_groups * p].reshape(n_groups, p, 2), rtol=1e-9, atol=0)
    assert np.array_equal(clips, proto[2 * n_groups * p:])


def _degenerate_cases(rng, j=17):
    """(name, pred, gt) single poses whose optimum is unique: the degenerate cases of tests/test_protocols_gpu.py."""
    gt = dr.clips(rng, 1, 1, j)[0, 0]
    k = np.arange(j, dtype=np.float64) - 8.0
    return [("zero", np.zeros((j, 3), np.float32), gt),
            ("all_equal", np.tile(np.float32([0.25, -0.5, 3.75]), (j, 1)), gt),
            ("collinear", (np.float32([1.0, 2.0, 3.0]) + np.outer(k / 8.0, [1.0, 2.0, -1.0])).astype(np.float32), gt),   # exact in fp32
            ("planar", np.concatenate([rng.standard_normal((j, 2)), np.full((j, 1), 4.5)], axis=1).astype(np.float32), gt),
            ("mirror", gt * np.float32([-1.0, 1.0, 1.0]), gt),
            ("gt_all_equal", gt, np.tile(np.float32([0.1, 0.2, 4.0]), (j, 1)))]


@pytest.mark.parametrize("root", [0, 9])
def test_degenerate_poses(lib, root):
    """One pose per group, so every slot is one pose's value; sums over joints against the protocols' oracle within 1e-8 m."""
    j, n_thr = 17, 31
    cases = _degenerate_cases(np.random.default_rng(7 + root), j)
    n = len(cases)
    pred = np.stack([c[1] for c in cases])[:, None]                    # (n, 1, J, 3)
    gt = np.stack([c[2] for c in cases])[:, None]
    got = _run(lib, pred, gt, 0, np.arange(n), n, root, n_thr)
    sec_a, sec_b, clips = _sections(got, n, 1, j)
    assert np.isfinite(got).all() and np.array_equal(clips, np.ones(n))
    assert np.all(sec_b[..., 4:] == 0.0)                               # p = 1: no motion terms
    hits = sec_b[:, 0, :4]
    assert np.array_equal(hits, np.round(hits)) and np.all(hits >= 0)
    assert np.all(hits[:, [0, 2]] <= n_thr * j) and np.all(hits[:, [1, 3]] <= j) and np.all(hits[:, [1, 3]] * (n_thr - 1) >= hits[:, [0, 2]])
    for i, (name, y, x) in enumerate(cases):
        s1, s2 = sec_a[i, 0, :, 0].sum(), sec_a[i, 0, :, 1].sum()
        want = (pr.p1_pose(y, x, root) * j, pr.p2_pose(y, x) * j)
        print(f"{name}: sum d1 {s1:.6e} (oracle {want[0]:.6e}) sum d2 {s2:.6e} (oracle {want[1]:.6e}) hits {hits[i].tolist()}")
        assert abs(s1 - want[0]) <= 1e-8 and abs(s2 - want[1]) <= 1e-8, name
        assert sec_a[i, 0, root, 0] == 0.0 and hits[i, 1] >= 1                       # the root's own d1: an exact zero, a hit
        if name == "mirror":
            assert s2 > 1e-2 * j                                       # no reflections: not aligned away
        if name == "gt_all_equal":
            assert s2 == 0.0 and hits[i, 2] == (n_thr - 1) * j and hits[i, 3] == j


def test_deterministic_and_adds(lib):
    rng = np.random.default_rng(11)
    b, t, i0, p, j, g = 600, 6, 1, 5, 17, 5                            # three passes of 256
    gt = dr.clips(rng, b, t, j)
    pd, gd = torch.from_numpy(dr.predictions(rng, gt, i0, p)).to(DEV), torch.from_numpy(gt).to(DEV)
    grp = torch.from_numpy(rng.integers(0, g, size=b).astype(np.int32)).to(DEV)
    runs = []
    for _ in range(2):
        acc = torch.zeros(dr.acc_size(g, p, j), dtype=torch.float64, device=DEV)
        assert _call(lib, pd, gd, i0, grp, g, 0, 31, dr.THR_MAX, acc) == 0
        runs.append(acc.cpu())
    assert torch.equal(runs[0], runs[1])                               # fixed order: the same bits
    assert runs[0][:2 * g * p * j].reshape(g, p, j, 2)[:, :, 1:].min() > 0
    acc = runs[0].to(DEV)
    assert _call(lib, pd, gd, i0, grp, g, 0, 31, dr.THR_MAX, acc) == 0   # it ADDS, once per slot: exactly twice the sums
    assert torch.equal(acc.cpu(), 2 * runs[0])


def test_refusals_launch_nothing(lib):
    from implementation_phd_lab_vision_amd import detail_metrics
    b, t, p, j, g = 4, 6, 3, 17, 2
    pred = torch.zeros(b, p, j, 3, device=DEV)
    gt = torch.zeros(b, t, j, 3, device=DEV)
    grp = torch.zeros(b, dtype=torch.int32, device=DEV)
    acc = torch.full((dr.acc_size(g, p, j),), 7.0, dtype=torch.float64, device=DEV)
    good = dict(pred=pred.data_ptr(), gt=gt.data_ptr(), group=grp.data_ptr(), b=b, p=p, t_gt=t, i0=1, joints=j, root=0, n_groups=g,
                n_thr=31, thr_max=0.150, acc=acc.data_ptr())
    bad = [dict(b=0), dict(p=0), dict(n_groups=0), dict(joints=0), dict(joints=65), dict(root=-1), dict(root=j), dict(i0=-1),
           dict(i0=t - p + 1), dict(t_gt=p - 1, i0=0), dict(n_thr=1), dict(n_thr=0), dict(n_thr=1025), dict(thr_max=0.0),
           dict(thr_max=-0.15), dict(thr_max=float("inf")), dict(thr_max=float("nan")), dict(pred=None), dict(gt=None),
           dict(group=None), dict(acc=None)]
    for change in bad:
        args = dict(good, **change)
        assert lib.r50_op_pose_detail_metrics(*args.values(), _stream()) != 0, change
        assert b"r50_op_pose_detail_metrics" in lib.r50_last_error(None), change
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full_like(acc, 7.0))                 # no refused call reached a launch
    with pytest.raises(ValueError, match=r"\[0, 2\)"):                 # the wrapper checks the group values on the host
        detail_metrics.add_detail_sums(pred, gt, 1, torch.tensor([0, 1, 2, 0], dtype=torch.int32, device=DEV), g, acc)
    with pytest.raises(ValueError):
        detail_metrics.add_detail_sums(pred, gt, 1, torch.tensor([0, -1, 0, 0], dtype=torch.int32, device=DEV), g, acc)
    with pytest.raises(ValueError):
        detail_metrics.add_detail_sums(pred, gt, 1, grp, g, acc, n_thr=1)
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full_like(acc, 7.0))
    assert lib.r50_op_pose_detail_metrics(*good.values(), _stream()) == 0
    detail_metrics.add_detail_sums(pred, gt, 1, grp, g, acc)
    sec_a, sec_b, clips = _sections(acc.cpu().numpy(), g, p, j)
    assert np.all(sec_a == 7.0) and np.array_equal(clips, [7.0 + 2 * b, 7.0])                        # zeros against zeros, twice
    assert np.array_equal(sec_b[0, :, 0], np.full(p, 7.0 + 2 * b * j * 30)) and np.all(sec_b[1] == 7.0)


# ------------------------------------------------------------------ evaluation ------------------------------------------------
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp("detail")
    return rd.make_results_cache(base / "features"), rd.make_preprocessed_tree(base / "videos")


def _head(d, nb, seed):
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    from oracle import lifting_oracle as lo
    sd = lo.synthetic_head_state_dict(d, nb, seed)
    h = PHDFor3DJoints(d, 17, nb)
    h.load_state_dict(sd)
    return h.to(DEV).eval(), sd


def _nanmean(a, axis):
    n = (~np.isnan(a)).sum(axis=axis)
    return np.where(n > 0, np.nansum(a, axis=axis) / np.maximum(n, 1), np.nan)


def _oracle_result(joints, gt, i0, ids, n_groups, n_thr, thr_max, over_frames):
    """The oracle's arrays from poses: per group, ``_all`` and ``_mean``; reduced over the frames when ``over_frames``."""
    p, j = joints.shape[1], joints.shape[2]
    v = dr.values_from_sums(dr.detail_sums(joints, gt, i0, ids, n_groups, 0, n_thr, thr_max), n_groups, p, j, n_thr)
    has = v["clips"] > 0
    out = {}
    for m in ("per_joint", "p1p2", "pck", "auc", "vel", "acc"):
        per_group, all_ = v[m], v[m + "_all"]
        if over_frames:
            red = _nanmean if m in ("vel", "acc") else np.mean
            per_group, all_ = red(per_group, axis=1), red(all_, axis=0)
        out.update({m: per_group, m + "_all": all_, m + "_mean": per_group[has].mean(axis=0)})
    return out


def test_evaluate_detail_against_oracle(lib, trees):
    from implementation_phd_lab_vision_amd import detail_metrics, protocols
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    store = DeviceFeatureStore(str(trees[0]), subjects=[9], test_set=True, device=DEV)
    names, ids = protocols.action_groups(store.item_actions())
    head, sd = _head(1024, 2, 6)
    i_len, p_len, g, n_thr, thr = 3, 5, len(names), 31, 0.150
    res = detail_metrics.evaluate_detail(head, store, ids, names, i_len, p_len)
    assert res["group_names"] == names and res["clips"].tolist() == np.bincount(ids).tolist() and res["clips"].dtype == np.int64
    assert res["joint_names"] == detail_metrics.H36M_JOINT_NAMES and (res["n_thr"], res["thr_max"]) == (n_thr, thr)
    assert res["recon_per_joint"].shape == (g, 17, 2) and res["recon_vel"].shape == (g,) and res["recon_pck_all"].shape == (2,)
    assert res["future_per_joint"].shape == (g, p_len, 17, 2) and res["future_acc_all"].shape == (p_len,)
    assert np.isnan(res["future_vel"][:, 0]).all() and np.isnan(res["future_acc"][:, [0, -1]]).all()
    assert not np.isnan(res["recon_vel"]).any() and not np.isnan(res["recon_acc"]).any()

    feats, gt = store.get_batch(list(range(len(store))))[:2]
    spans = (("recon", head.joints(feats).cpu(), 0), ("future", head.rollout(feats, i_len, p_len)[1].cpu(), i_len))
    for which, joints, i0 in spans:                                     # the device's own outputs: one batch of 11
        d1, d2, _, _ = dr.distances(joints, gt.cpu(), i0)
        gap = dr.smallest_threshold_gap(d1, d2, n_thr, thr)
        print(f"{which}: smallest |d - tau| of the head's outputs {gap:.3e} m")
        assert gap >= 1e-9, "a distance sits on a threshold: pick another head seed"
        want = _oracle_result(joints, gt.cpu(), i0, ids, g, n_thr, thr, over_frames=which == "recon")
        for key, value in want.items():
            np.testing.assert_allclose(res[f"{which}_{key}"], value, rtol=1e-9, atol=0, err_msg=f"{which}_{key}")
        p12 = protocols.evaluate_protocols(head, store, ids, names, i_len, p_len)
        np.testing.assert_allclose(res[f"{which}_p1p2"], p12[which], rtol=1e-9, atol=0)          # P1 / P2 without a second pass

    ref_joints = lo.forward_reference(sd, feats.cpu())[2]               # the fp64 reference head: for the record, not asserted
    ref_future = rollout_reference(sd, feats.cpu(), i_len, p_len)[1]
    for which, joints, i0 in (("recon", ref_joints, 0), ("future", ref_future, i_len)):
        want = _oracle_result(joints, gt.cpu(), i0, ids, g, n_thr, thr, over_frames=which == "recon")
        for key in ("per_joint_all", "pck_all", "auc_all", "vel_all", "acc_all"):
            diff = np.abs(res[f"{which}_{key}"] - want[key])
            print(f"{which}_{key}: device vs fp64 reference head, largest difference {np.nanmax(diff):.2e} "
                  f"(values up to {np.nanmax(np.abs(want[key])):.3e})")

    for bs in (2, 7, 256):
        other = detail_metrics.evaluate_detail(head, store, ids, names, i_len, p_len, batch_size=bs)
        assert np.array_equal(other["clips"], res["clips"])
        for key in (k for k in res if k.startswith(("recon_", "future_"))):
            np.testing.assert_allclose(other[key], res[key], rtol=1e-12, atol=0, err_msg=f"{bs} {key}")

    recon_only = detail_metrics.evaluate_detail(head, store, ids, names)   # no rollout: the same reconstruction sums
    assert not any(k.startswith("future_") for k in recon_only)
    assert all(np.array_equal(recon_only[k], res[k], equal_nan=True) for k in res if k.startswith("recon_"))
    padded = detail_metrics.evaluate_detail(head, store, ids, names + ["zz_empty"])      # a group without clips: NaN, out of the means
    assert padded["clips"][-1] == 0
    for m in detail_metrics.METRICS:
        assert np.isnan(padded[f"recon_{m}"][-1]).all(), m
        assert np.array_equal(padded[f"recon_{m}"][:-1], res[f"recon_{m}"]) and np.array_equal(padded[f"recon_{m}_mean"], res[f"recon_{m}_mean"])
    with pytest.raises(ValueError):
        detail_metrics.evaluate_detail(head, store, ids, names, 4, 5)                    # 9 > seq_len 8
    with pytest.raises(ValueError):
        detail_metrics.evaluate_detail(head, store, ids[:-1], names)
    with pytest.raises(ValueError):
        detail_metrics.evaluate_detail(head, store, [3] * len(store), names)


# ------------------------------------------------------------------ CLI -------------------------------------------------------
def _cli(argv):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "implementation_phd_lab_vision_amd.results", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"results exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def _same_array(a, b) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != object:
        return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return all(set(x) == set(y) and all(torch.equal(x[k], y[k]) if isinstance(x[k], torch.Tensor) else x[k] == y[k] for k in x)
               for x, y in zip(a, b))


def test_results_cli_detail_metrics(lib, trees, tmp_path):
    from implementation_phd_lab_vision_amd import detail_metrics, protocols, results
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    features, videos = trees
    sd = lo.synthetic_head_state_dict(1024, 2, seed=2)
    ckpt = tmp_path / "model.pt"
    torch.save(sd, ckpt)
    base = ["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(ckpt), "--seq-len", str(rd.SEQ_LEN),
            "--batch-size", "4", "--save-n", "3", "--video-size", "32", "--video-reader", "tests.results_data:read_video",
            "--input-len", "3", "--pred-len", "5"]
    out_off, out_on, out_100 = tmp_path / "off.npz", tmp_path / "on.npz", tmp_path / "on100.npz"
    so_off = _cli(base + ["--out", str(out_off)])
    so_on = _cli(base + ["--out", str(out_on), "--detail-metrics"])
    _cli(base + ["--out", str(out_100), "--detail-metrics", "--pck-threshold-mm", "100", "--auc-steps", "11"])

    store = DeviceFeatureStore(str(features), subjects=[9], test_set=True, device=DEV)
    head = results.build_head(sd, DEV)
    names, ids = protocols.action_groups(store.item_actions())
    res = detail_metrics.evaluate_detail(head, store, ids, names, 3, 5)
    lines = detail_metrics.detail_lines(res, 3, 5)
    assert lines[0].startswith("Detail metrics | clips 11 | actions 3 | all: pck@150 (%) ") and len(lines) == 6
    assert lines[1].startswith("Per-joint p1 / p2 (mm) | pelvis 0.00 / ")
    assert lines[-1].startswith("Rollout detail metrics | input 3 | pred 5 | clips 11 | pck@150 (%) @1: ")
    prefixes = ("Detail metrics", "Per-joint", "Rollout detail metrics", "  ")
    on_lines = so_on.replace(str(out_on), str(out_off)).splitlines()
    assert [l for l in on_lines if l.startswith(prefixes)] == lines
    assert not any(l.startswith(prefixes) for l in so_off.splitlines())
    timing = ("Results time",)
    assert [l for l in on_lines if l not in lines and not l.startswith(timing)] == \
           [l for l in so_off.splitlines() if not l.startswith(timing)]                  # the rest of stdout as without the flag

    z_off, z_on, z_100 = (np.load(f, allow_pickle=True) for f in (out_off, out_on, out_100))
    want = detail_metrics.detail_npz(res)
    assert set(z_on.files) == set(z_off.files) | set(want) and not set(want) & set(z_off.files)
    assert all(k.startswith("detail_") for k in want) and not any(k.startswith("detail_") for k in z_off.files)
    for key in z_off.files:
        assert _same_array(z_off[key], z_on[key]), key
    assert z_on["detail_actions"].dtype.kind == "U" and z_on["detail_actions"].tolist() == names
    assert z_on["detail_clips"].dtype == np.int64 and z_on["detail_clips"].tolist() == res["clips"].tolist()
    floats = [k for k in want if want[k].dtype == np.float32]
    assert len(floats) == 24
    for key in floats:
        assert z_on[key].dtype == np.float32 and np.array_equal(z_on[key], res[key[len("detail_"):]].astype(np.float32), equal_nan=True), key

    assert set(z_100.files) == set(z_on.files)                          # another threshold and step count: pck / auc and nothing else
    for key in z_on.files:
        if "_pck" in key or "_auc" in key:
            assert z_100[key].shape == z_on[key].shape and not np.array_equal(z_100[key], z_on[key]), key
        else:
            assert _same_array(z_100[key], z_on[key]), key
    res_100 = detail_metrics.evaluate_detail(head, store, ids, names, 3, 5, n_thr=11, thr_max=0.1)
    assert np.array_equal(z_100["detail_future_pck"], res_100["future_pck"].astype(np.float32))
    assert np.array_equal(z_100["detail_recon_auc_all"], res_100["recon_auc_all"].astype(np.float32))
