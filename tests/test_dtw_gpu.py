"""The forecast error after dynamic time warping on the MI355X: ``r50_op_dtw_protocols`` against the numpy
fp64 oracle (tests/dtw_reference.py), band 0 against ``r50_op_pose_protocols``, warped <= plain, exact ties, determinism, accumulation,
refusals and a non-finite input; ``dtw.evaluate_dtw`` against the oracle on the device's own rollouts; the results CLI's ``--dtw``.  CLI
runs are fresh child processes under a time limit.

Totals are held to ``rtol 1e-9, atol 1e-12``, the bar tests/test_protocols_gpu.py holds sums of the same per-cell costs to: the optimum
of a DP over sums moves by at most the sum of the cost changes along a path.  Two candidates can swap only when they are closer than
twice that bar, so the path, ``L``, ``cells`` and everything that depends on them is compared on the clips whose oracle decision margin
is at least ``1e-7 * total`` (fifty times that) -- and on the seeded kernel cases no clip may fall under it."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import dtw_reference as dr
from tests import results_data as rd
from tests.kernel_cases import _case_inputs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
MARGIN = 1e-7                                   # of the clip's total

CASES = [(5, 7, 7, 9, 2, 17, 4, 0, -1), (300, 3, 5, 6, 1, 3, 3, 2, -1), (4, 5, 3, 3, 0, 17, 2, 0, 2), (3, 1, 6, 6, 0, 17, 1, 0, -1),
         (3, 6, 1, 4, 3, 17, 2, 0, -1), (2, 64, 64, 64, 0, 17, 2, 0, -1), (6, 25, 25, 40, 15, 17, 15, 0, -1), (7, 9, 9, 9, 0, 32, 3, 31, 3),
         (2, 4, 4, 4, 0, 1, 1, 0, -1)]


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _acc_size(n_groups, p):
    return n_groups * 2 * (1 + 2 * p) + n_groups


def _run(lib, pred, gt, i0, q, group, n_groups, root=0, band=-1, acc=None, paths=True):
    """One call; pred / gt / group numpy or CPU tensors.  Returns (clip_out, path_out or None, acc) as device tensors."""
    pd, gd = torch.as_tensor(pred).to(DEV).contiguous(), torch.as_tensor(gt).to(DEV).contiguous()
    grp = torch.as_tensor(np.asarray(group), dtype=torch.int32).to(DEV)
    b, p, j, _ = pd.shape
    if acc is None:
        acc = torch.zeros(_acc_size(n_groups, p), dtype=torch.float64, device=DEV)
    clip_out = torch.full((b, 2, 2 + 3 * p), -7.0, dtype=torch.float64, device=DEV)
    path_out = torch.full((b, 2, p + q - 1, 2), -7, dtype=torch.int32, device=DEV) if paths else None
    rc = lib.r50_op_dtw_protocols(pd.data_ptr(), gd.data_ptr(), grp.data_ptr(), b, p, gd.shape[1], i0, q, j, root, band, n_groups,
                                  clip_out.data_ptr(), path_out.data_ptr() if paths else None, acc.data_ptr(), _stream())
    assert rc == 0, lib.r50_last_error(None)
    torch.cuda.synchronize()
    return clip_out, path_out, acc


_ORACLE = {}


def _oracle(case):
    """The oracle of one case, computed once and shared: per prediction set (results, clip_out, path_out, margins), and the inputs."""
    if case not in _ORACLE:
        b, p, q, t_gt, i0, j, n_groups, root, band = case
        plain, fitted, gt, group = _case_inputs(case)
        _ORACLE[case] = (plain, fitted, gt, group, dr.dtw_batch(plain, gt, i0, q, root, band), dr.dtw_batch(fitted, gt, i0, q, root, band))
    return _ORACLE[case]


def _compare(got_clip, got_path, want_clip, want_path, margins, metrics, p, what):
    """Totals on every clip; the path and what depends on it on the clips above the margin.  Returns the number of excluded
    (clip, metric) pairs."""
    got_clip, got_path = got_clip.cpu().numpy(), got_path.cpu().numpy()
    excluded = 0
    np.testing.assert_allclose(got_clip[:, :, 0], want_clip[:, :, 0], rtol=1e-9, atol=1e-12, err_msg=f"{what} totals")
    for m in metrics:
        for i in range(len(got_clip)):
            if not margins[i, m] >= MARGIN * want_clip[i, m, 0]:
                excluded += 1
                continue
            assert np.array_equal(got_path[i, m], want_path[i, m]), (what, i, m)
            assert got_clip[i, m, 1] == want_clip[i, m, 1], (what, i, m)
            assert np.array_equal(got_clip[i, m, 2 + p:2 + 2 * p], want_clip[i, m, 2 + p:2 + 2 * p]), (what, i, m)
            np.testing.assert_allclose(got_clip[i, m, 2:2 + p], want_clip[i, m, 2:2 + p], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(got_clip[i, m, 2 + 2 * p:], want_clip[i, m, 2 + 2 * p:], rtol=1e-9, atol=0)
    return excluded


# ------------------------------------------------------------------ kernel ----------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_kernel_matches_oracle(lib, case):
    b, p, q, t_gt, i0, j, n_groups, root, band = case
    plain, fitted, gt, group, want_plain, want_fitted = _oracle(case)
    counts = np.bincount(group, minlength=n_groups)
    v = 1 + 2 * p
    for what, pred, want, metrics in (("plain", plain, want_plain, (0, 1)), ("fitted", fitted, want_fitted, (1,))):
        _, want_clip, want_path, margins = want
        clip_out, path_out, acc = _run(lib, pred, gt, i0, q, group, n_groups, root, band)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.nan_to_num(margins / want_clip[:, :, 0], nan=np.inf)
        print(f"{what}: smallest margin / total per metric {rel.min(axis=0)}")
        excluded = _compare(clip_out, path_out, want_clip, want_path, margins, metrics, p, what)
        assert excluded == 0, f"{what}: {excluded} clips under the margin: pick another seed"
        got_clip = clip_out.cpu().numpy()
        assert ((got_clip[:, :, 1] >= max(p, q)) & (got_clip[:, :, 1] <= p + q - 1)).all()
        acc_np = acc.cpu().numpy()
        want_acc = dr.dtw_sums(want_clip, group, n_groups)
        sums, want_sums = acc_np[:n_groups * 2 * v].reshape(n_groups, 2, v), want_acc[:n_groups * 2 * v].reshape(n_groups, 2, v)
        for m in metrics:
            np.testing.assert_allclose(sums[:, m], want_sums[:, m], rtol=1e-9, atol=1e-12, err_msg=f"{what} acc m={m}")
        assert np.array_equal(acc_np[n_groups * 2 * v:], counts.astype(np.float64))
        assert np.all(sums[counts == 0] == 0.0)
        if p > 1 and q > 1 and j > 1:                                   # the inputs do warp: an off-diagonal cell in each checked metric
            path = path_out.cpu().numpy()
            for m in metrics:
                assert ((path[:, m, :, 0] != path[:, m, :, 1]) & (path[:, m, :, 0] >= 0)).any(), (what, m)
        if j == 1:                                                      # one joint: every cost is exactly 0, every choice a tie
            assert np.all(got_clip[:, :, 0] == 0.0) and np.array_equal(path_out.cpu().numpy()[:, :, :p, 0], np.tile(np.arange(p), (b, 2, 1)))
            assert np.all(got_clip[:, :, 1] == p)


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == c[2]], ids=lambda c: "-".join(str(v) for v in c))
def test_band_zero_is_the_plain_protocol_and_bounds_the_warped_error(lib, case):
    b, p, q, t_gt, i0, j, n_groups, root, band = case
    plain, fitted, gt, group = _oracle(case)[:4]
    v = 1 + 2 * p
    for pred in (plain, fitted):
        clip0, path0, acc0 = _run(lib, pred, gt, i0, q, group, n_groups, root, band=0)
        pd, gd = torch.as_tensor(pred).to(DEV), torch.as_tensor(gt).to(DEV)
        grp = torch.as_tensor(group, dtype=torch.int32).to(DEV)
        prot = torch.zeros(2 * n_groups * p + n_groups, dtype=torch.float64, device=DEV)
        assert lib.r50_op_pose_protocols(pd.data_ptr(), gd.data_ptr(), grp.data_ptr(), b, p, t_gt, i0, j, root, n_groups, prot.data_ptr(),
                                         _stream()) == 0
        prot = prot.cpu().numpy()
        acc0 = acc0.cpu().numpy()
        sums = acc0[:n_groups * 2 * v].reshape(n_groups, 2, v)
        want = prot[:2 * n_groups * p].reshape(n_groups, p, 2).transpose(0, 2, 1)                 # (G, 2, P)
        np.testing.assert_allclose(sums[:, :, 1:1 + p], want, rtol=1e-12, atol=0)
        assert np.all(sums[:, :, 1 + p:] == 0.0)                                                  # every lag exactly 0
        assert np.array_equal(acc0[n_groups * 2 * v:], prot[2 * n_groups * p:])
        clip0 = clip0.cpu().numpy()
        assert np.all(clip0[:, :, 1] == p) and np.all(clip0[:, :, 2 + p:2 + 2 * p] == 1.0) and np.all(clip0[:, :, 2 + 2 * p:] == 0.0)
        diag = path0.cpu().numpy()[:, :, :p]
        assert np.array_equal(diag[..., 0], diag[..., 1]) and np.array_equal(diag[0, 0, :, 0], np.arange(p))
        assert np.all(path0.cpu().numpy()[:, :, p:] == -1)
        free = _run(lib, pred, gt, i0, q, group, n_groups, root, band)[0].cpu().numpy()
        # the band-0 total is the diagonal's sum in the DP's own order: rounding cannot lift the warped total above it
        assert np.all(free[:, :, 0] <= clip0[:, :, 0])
        assert np.all(free[:, :, 0] / free[:, :, 1] <= clip0[:, :, 0] / p)


def test_exact_ties_on_plateaus(lib):
    pred, gt, want_path = dr.plateau_inputs()
    (r1, _), c = dr.dtw_clip(pred[0], gt[0])
    assert r1["path"] == want_path and r1["total"] == 0.0 and (c[0] == 0.0).sum() == len(want_path) and c[0][c[0] > 0].min() > 1e-2
    clip_out, path_out, _ = _run(lib, pred, gt, 0, 6, [0], 1)
    clip_out, path_out = clip_out.cpu().numpy(), path_out.cpu().numpy()
    assert clip_out[0, 0, 0] == 0.0 and clip_out[0, 0, 1] == len(want_path)                       # exactly 0.0
    assert np.array_equal(path_out[0, 0], dr.path_array(r1, 6, 6))
    assert np.array_equal(clip_out[0, 0], dr.record(r1))
    band = _run(lib, pred, gt, 0, 6, [0], 1, band=0)[0].cpu().numpy()
    assert band[0, 0, 0] > 0.0                                                                   # the plain P1 is not 0
    # every cost equal (all poses the same): every choice is a tie, the path is the diagonal
    same = np.tile(gt[:, :1], (1, 6, 1, 1))
    clip_s, path_s, _ = _run(lib, same, same, 0, 6, [0], 1)
    assert np.all(clip_s.cpu().numpy()[0, 0, :2] == [0.0, 6.0])
    assert np.array_equal(path_s.cpu().numpy()[0, 0, :6], np.stack([np.arange(6)] * 2, axis=1))


def test_deterministic_adds_and_null_path(lib):
    case = (6, 25, 25, 40, 15, 17, 15, 0, -1)
    b, p, q, t_gt, i0, j, n_groups, root, band = case
    plain, _, gt, group = _oracle(case)[:4]
    first = _run(lib, plain, gt, i0, q, group, n_groups, root, band)
    second = _run(lib, plain, gt, i0, q, group, n_groups, root, band)
    for a, b_ in zip(first, second):
        assert torch.equal(a, b_)                                        # fixed order: the same bits
    again = _run(lib, plain, gt, i0, q, group, n_groups, root, band, acc=first[2].clone())
    assert torch.equal(again[2], 2 * first[2])                           # it ADDS
    no_path = _run(lib, plain, gt, i0, q, group, n_groups, root, band, paths=False)
    assert no_path[1] is None and torch.equal(no_path[0], first[0]) and torch.equal(no_path[2], first[2])


def test_refusals_launch_nothing(lib):
    from implementation_phd_lab_vision_amd import dtw
    b, t, p, q, j, g = 4, 8, 3, 5, 17, 2
    pred = torch.zeros(b, p, j, 3, device=DEV)
    gt = torch.zeros(b, t, j, 3, device=DEV)
    grp = torch.zeros(b, dtype=torch.int32, device=DEV)
    acc = torch.full((_acc_size(g, p),), 7.0, dtype=torch.float64, device=DEV)
    clip_out = torch.full((b, 2, 2 + 3 * p), 5.0, dtype=torch.float64, device=DEV)
    path_out = torch.full((b, 2, p + q - 1, 2), 5, dtype=torch.int32, device=DEV)
    good = dict(pred=pred.data_ptr(), gt=gt.data_ptr(), group=grp.data_ptr(), b=b, p=p, t_gt=t, i0=1, q=q, joints=j, root=0, band=-1,
                n_groups=g, clip_out=clip_out.data_ptr(), path_out=path_out.data_ptr(), acc=acc.data_ptr())
    assert lib.r50_op_dtw_protocols(*good.values(), _stream()) == 0
    assert lib.r50_op_dtw_protocols(*dict(good, path_out=None).values(), _stream()) == 0          # path_out may be null
    torch.cuda.synchronize()
    kept = acc.clone(), clip_out.clone(), path_out.clone()
    bad = [dict(b=0), dict(p=0), dict(p=65), dict(q=0), dict(q=65), dict(joints=0), dict(joints=65), dict(root=-1), dict(root=j),
           dict(i0=-1), dict(i0=t - q + 1), dict(band=0), dict(band=1), dict(n_groups=0), dict(pred=None), dict(gt=None), dict(group=None),
           dict(clip_out=None), dict(acc=None)]
    for change in bad:
        args = dict(good, **change)
        assert lib.r50_op_dtw_protocols(*args.values(), _stream()) != 0, change
        assert b"r50_op_dtw_protocols" in lib.r50_last_error(None), change
    torch.cuda.synchronize()
    assert torch.equal(acc, kept[0]) and torch.equal(clip_out, kept[1]) and torch.equal(path_out, kept[2])
    assert lib.r50_op_dtw_protocols(*dict(good, band=2).values(), _stream()) == 0                 # band = |p - q| is allowed

    kept = acc.clone()
    with pytest.raises(ValueError, match=r"\[0, 2\)"):                  # the wrapper checks the group values on the host
        dtw.add_dtw_sums(pred, gt, 1, q, torch.tensor([0, 1, 2, 0], dtype=torch.int32, device=DEV), g, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt, 1, q, torch.tensor([0, -1, 0, 0], dtype=torch.int32, device=DEV), g, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(torch.zeros(b, p, 65, 3, device=DEV), torch.zeros(b, t, 65, 3, device=DEV), 1, q, grp, g, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred.double(), gt, 1, q, grp, g, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred[:, :, :, :2], gt, 1, q, grp, g, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt[:3], 1, q, grp, g, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt, 1, q, grp.long(), g, acc)
    with pytest.raises(ValueError):
        dtw.add_dtw_sums(pred, gt, 1, q, grp, g, acc.float())
    with pytest.raises(ValueError, match="band"):
        dtw.add_dtw_sums(pred, gt, 1, q, grp, g, acc, band=1)
    with pytest.raises(ValueError, match="GPU"):
        dtw.add_dtw_sums(pred.cpu(), gt, 1, q, grp, g, acc)
    torch.cuda.synchronize()
    assert torch.equal(acc, kept)
    rec = dtw.add_dtw_sums(pred, gt, 1, q, grp, g, acc)
    assert tuple(rec.shape) == (b, 2, 2 + 3 * p) and not torch.equal(acc, kept)


def test_a_nan_coordinate_stays_in_its_clip(lib):
    """Ordinary data: one NaN coordinate in one predicted frame of one clip.  Every path crosses that frame's row, so the clip's totals
    are NaN; the other clips' records are bit-equal to the run without it, and every loop ends."""
    case = (5, 7, 7, 9, 2, 17, 4, 0, -1)
    b, p, q, t_gt, i0, j, n_groups, root, band = case
    plain, _, gt, group = _oracle(case)[:4]
    clean = _run(lib, plain, gt, i0, q, group, n_groups, root, band)
    dirty_pred = plain.copy()
    dirty_pred[2, 3, 5, 1] = np.nan
    dirty = _run(lib, dirty_pred, gt, i0, q, group, n_groups, root, band)
    rec, ref = dirty[0].cpu().numpy(), clean[0].cpu().numpy()
    assert np.isnan(rec[2, :, 0]).all()
    assert ((rec[2, :, 1] >= p) & (rec[2, :, 1] <= p + q - 1)).all() and (rec[2, :, 2 + p:2 + 2 * p] >= 1).all()
    others = [i for i in range(b) if i != 2]
    assert np.array_equal(rec[others], ref[others]) and torch.equal(dirty[1][others], clean[1][others])
    acc, acc_ref = dirty[2].cpu().numpy(), clean[2].cpu().numpy()
    v = 1 + 2 * p
    sums, sums_ref = acc[:n_groups * 2 * v].reshape(n_groups, 2 * v), acc_ref[:n_groups * 2 * v].reshape(n_groups, 2 * v)
    other_groups = [g for g in range(n_groups) if g != group[2]]
    assert np.isnan(sums[group[2]]).any() and np.array_equal(sums[other_groups], sums_ref[other_groups])


# ------------------------------------------------------------------ evaluation ------------------------------------------------
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp("dtw")
    return rd.make_results_cache(base / "features"), rd.make_preprocessed_tree(base / "videos")


def _head(d, nb, seed):
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    from oracle import lifting_oracle as lo
    sd = lo.synthetic_head_state_dict(d, nb, seed)
    h = PHDFor3DJoints(d, 17, nb)
    h.load_state_dict(sd)
    return h.to(DEV).eval(), sd


def test_evaluate_dtw_against_oracle(lib, trees):
    from implementation_phd_lab_vision_amd import dtw, protocols
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    store = DeviceFeatureStore(str(trees[0]), subjects=[9], test_set=True, device=DEV)
    names, ids = protocols.action_groups(store.item_actions())
    head, _ = _head(1024, 2, 6)
    i_len, p_len, g = 3, 5, len(names)
    res = dtw.evaluate_dtw(head, store, ids, names, i_len, p_len)
    assert res["group_names"] == names and res["clips"].tolist() == np.bincount(ids).tolist() and res["clips"].dtype == np.int64
    for key, shape in (("dtw", (g, 2)), ("dtw_all", (2,)), ("dtw_mean", (2,)), ("dtw_future", (g, p_len, 2)), ("dtw_future_all", (p_len, 2)),
                       ("lag", (g, p_len, 2)), ("lag_all", (p_len, 2)), ("plain_future_all", (p_len, 2)), ("plain_all", (2,))):
        assert res[key].shape == shape and res[key].dtype == np.float64, key
    assert np.allclose(res["dtw_mean"], res["dtw"].mean(axis=0), rtol=1e-15) and res["band"] == -1

    feats, gt = store.get_batch(list(range(len(store))))[:2]
    pred = head.rollout(feats, i_len, p_len)[1]                          # the device's own rollout: one batch of 11
    gt32 = gt.to(torch.float32)
    _, want_clip, want_path, margins = dr.dtw_batch(pred.cpu(), gt32.cpu(), i_len, p_len)
    acc = torch.zeros(dtw.acc_size(g, p_len), dtype=torch.float64, device=DEV)
    path_out = torch.empty((len(store), 2, 2 * p_len - 1, 2), dtype=torch.int32, device=DEV)
    clip_out = dtw.add_dtw_sums(pred, gt32.contiguous(), i_len, p_len, torch.tensor(ids, dtype=torch.int32, device=DEV), g, acc,
                                path_out=path_out)
    torch.cuda.synchronize()
    excluded = _compare(clip_out, path_out, want_clip, want_path, margins, (0, 1), p_len, "evaluate")
    low = np.flatnonzero((margins < MARGIN * want_clip[:, :, 0]).any(axis=1))
    print(f"clips under the margin: {len(low)} of {len(store)} ({excluded} clip-metric pairs)")
    assert len(low) <= 2
    keep = np.setdiff1d(np.arange(len(store)), low)
    want = dr.values_from_sums(dr.dtw_sums(want_clip, ids, g), g, p_len)
    own = dr.values_from_sums(dr.dtw_sums(clip_out.cpu().numpy(), ids, g), g, p_len)         # the pass aggregates its own records
    for key in ("dtw", "dtw_all", "dtw_mean", "dtw_future", "dtw_future_all", "lag", "lag_all"):
        np.testing.assert_allclose(res[key], own[key], rtol=1e-12, atol=1e-15, err_msg=key)
    if len(low) == 0:
        for key in ("dtw", "dtw_all", "dtw_future", "dtw_future_all"):
            np.testing.assert_allclose(res[key], want[key], rtol=1e-9, atol=1e-12, err_msg=key)
        for key in ("lag", "lag_all"):
            np.testing.assert_allclose(res[key], want[key], rtol=1e-9, atol=1e-12, err_msg=key)
    else:                                                                # the path-dependent values on the clips above the margin
        sub = dr.values_from_sums(dr.dtw_sums(want_clip[keep], np.zeros(len(keep), dtype=np.int64), 1), 1, p_len)
        got = dr.values_from_sums(dr.dtw_sums(clip_out.cpu().numpy()[keep], np.zeros(len(keep), dtype=np.int64), 1), 1, p_len)
        for key in ("dtw_all", "dtw_future_all", "lag_all"):
            np.testing.assert_allclose(got[key], sub[key], rtol=1e-9, atol=1e-12, err_msg=key)
    plain = protocols.evaluate_protocols(head, store, ids, names, i_len, p_len)
    assert np.array_equal(res["plain_future_all"], plain["future_all"])                      # the same arithmetic, the same pass
    assert np.all(res["dtw_all"] <= res["plain_all"] * (1.0 + 1e-12))                        # means of per-clip values, each warped <= plain

    for bs in (2, 7, 256):
        other = dtw.evaluate_dtw(head, store, ids, names, i_len, p_len, batch_size=bs)
        assert np.array_equal(other["clips"], res["clips"])
        for key in ("dtw", "dtw_all", "dtw_mean", "dtw_future", "dtw_future_all", "lag", "lag_all", "plain_future_all", "plain_all"):
            np.testing.assert_allclose(other[key], res[key], rtol=1e-12, atol=1e-15, err_msg=f"{bs} {key}")

    padded = dtw.evaluate_dtw(head, store, ids, names + ["zz_empty"], i_len, p_len)          # a group without clips: NaN, out of the mean
    assert np.isnan(padded["dtw"][-1]).all() and np.isnan(padded["lag"][-1]).all() and padded["clips"][-1] == 0
    assert np.array_equal(padded["dtw"][:-1], res["dtw"]) and np.array_equal(padded["dtw_mean"], res["dtw_mean"])
    banded = dtw.evaluate_dtw(head, store, ids, names, i_len, p_len, band=0)
    assert np.all(banded["lag_all"] == 0.0) and banded["band"] == 0
    np.testing.assert_allclose(banded["dtw_future_all"], res["plain_future_all"], rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        dtw.evaluate_dtw(head, store, ids, names, 4, 5)                  # 9 > seq_len 8
    with pytest.raises(ValueError):
        dtw.evaluate_dtw(head, store, ids, names, 3, 0)
    with pytest.raises(ValueError):
        dtw.evaluate_dtw(head, store, ids[:-1], names, i_len, p_len)
    with pytest.raises(ValueError):
        dtw.evaluate_dtw(head, store, [3] * len(store), names, i_len, p_len)


# ------------------------------------------------------------------ CLI -------------------------------------------------------
def _cli(argv, ok=True):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "implementation_phd_lab_vision_amd.results", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, f"results exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


def _same_array(a, b) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != object:
        return np.array_equal(a, b)
    return all(set(x) == set(y) and all(torch.equal(x[k], y[k]) if isinstance(x[k], torch.Tensor) else x[k] == y[k] for k in x)
               for x, y in zip(a, b))


def test_results_cli_dtw(lib, trees, tmp_path):
    from implementation_phd_lab_vision_amd import dtw, protocols, results
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    features, videos = trees
    sd = lo.synthetic_head_state_dict(1024, 2, seed=2)
    ckpt = tmp_path / "model.pt"
    torch.save(sd, ckpt)
    base = ["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(ckpt), "--seq-len", str(rd.SEQ_LEN),
            "--batch-size", "4", "--save-n", "3", "--video-size", "32", "--video-reader", "tests.results_data:read_video"]
    rollout = ["--input-len", "3", "--pred-len", "5"]
    out_off, out_on = tmp_path / "off.npz", tmp_path / "on.npz"
    so_off = _cli(base + rollout + ["--out", str(out_off)]).stdout
    so_on = _cli(base + rollout + ["--out", str(out_on), "--dtw"]).stdout
    refused = _cli(base + ["--out", str(tmp_path / "no.npz"), "--dtw"], ok=False)               # --dtw without --pred-len
    assert refused.returncode != 0 and "--dtw needs --pred-len" in refused.stderr and not (tmp_path / "no.npz").exists()

    store = DeviceFeatureStore(str(features), subjects=[9], test_set=True, device=DEV)
    head = results.build_head(sd, DEV)
    names, ids = protocols.action_groups(store.item_actions())
    res = dtw.evaluate_dtw(head, store, ids, names, 3, 5)
    lines = dtw.dtw_lines(res, 3, 5)
    assert lines[0].startswith("DTW metrics | input 3 | pred 5 | band none | clips 11 | all: p1 (mm) ") and len(lines) == 5
    assert lines[-1].startswith("DTW horizons | p1 (mm) @1: ") and "lag p2 (frames) @1: " in lines[-1]
    on_lines = so_on.replace(str(out_on), str(out_off)).splitlines()
    for line in lines:
        assert line in on_lines, line
    assert not any(l.startswith(("DTW metrics", "DTW horizons")) for l in so_off.splitlines())
    timing = ("Results time",)
    assert [l for l in on_lines if l not in lines and not l.startswith(timing)] == \
           [l for l in so_off.splitlines() if not l.startswith(timing)]                  # the rest of stdout as without the flag

    z_off, z_on = np.load(out_off, allow_pickle=True), np.load(out_on, allow_pickle=True)
    new = {"dtw_actions", "dtw_clips", "dtw", "dtw_all", "dtw_future", "dtw_future_all", "dtw_lag", "dtw_lag_all", "dtw_band"}
    assert set(z_on.files) == set(z_off.files) | new and not new & set(z_off.files)
    for key in z_off.files:
        assert _same_array(z_off[key], z_on[key]), key
    assert z_on["dtw_actions"].dtype.kind == "U" and z_on["dtw_actions"].tolist() == names
    assert z_on["dtw_clips"].dtype == np.int64 and z_on["dtw_clips"].tolist() == res["clips"].tolist()
    assert z_on["dtw_band"].dtype == np.int64 and int(z_on["dtw_band"]) == -1
    for key, want in (("dtw", res["dtw"]), ("dtw_all", res["dtw_all"]), ("dtw_future", res["dtw_future"]),
                      ("dtw_future_all", res["dtw_future_all"]), ("dtw_lag", res["lag"]), ("dtw_lag_all", res["lag_all"])):
        assert z_on[key].dtype == np.float32 and np.array_equal(z_on[key], want.astype(np.float32)), key
