"""Forecast baselines on the MI355X: ``r50_op_nn_search`` against the fp64 oracle on the same 16-bit-rounded
operands under the DERIVED bound of tests/baselines_reference.py (no measured tolerance appears here), its ties, position independence
and work distribution, its refusals; ``r50_op_baseline_forecasts`` bit for bit against the numpy restatement; ``observe``,
``StripDatabase``, ``evaluate_baselines`` and the ``results --baselines`` CLI on a small cache."""
import itertools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import baselines_data as bd
from tests import baselines_reference as br
from tests import protocols_reference as pr
from tests import results_data as rd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
CAPS = (1, 3, 5)


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def _search(q16, x16, k):
    """(idx (NQ, k) int64, dist2 (NQ, k) fp32) numpy, through the module's wrappers."""
    from implementation_phd_lab_vision_amd.baselines import nn_search, row_norm2
    xd = x16.to(DEV)
    idx, dist2 = nn_search(q16.to(DEV), xd, row_norm2(xd), k)
    return idx.cpu().numpy().astype(np.int64), dist2.cpu().numpy()


def _check_values(q16, x16, k, idx, dist2, what=""):
    """Check 1: every query, every rank.  The TRUE score of the returned r-th row within 2 E_q of the oracle's r-th smallest, dist2
    within 2 E_q + u (|q|^2 + |x|^2) of the oracle's; the rows distinct and in range."""
    n = x16.shape[0]
    assert idx.shape == dist2.shape == (q16.shape[0], k) and idx.min() >= 0 and idx.max() < n, what
    assert all(len(set(row)) == k for row in idx.tolist()), f"{what}: a row returned twice"
    s = br.true_scores(q16, x16)
    _, want_s, want_d2 = br.search(q16, x16, k)
    got_s = np.take_along_axis(s, idx, axis=1)
    vb, db = br.value_bound(q16, x16), br.dist2_bound(q16, x16)
    worst_s, worst_d = np.max(np.abs(got_s - want_s) / vb[:, None]), np.max(np.abs(dist2.astype(np.float64) - want_d2) / db[:, None])
    print(f"{what}: largest |true score - oracle| / bound {worst_s:.3e}; dist2 {worst_d:.3e}")
    assert worst_s <= 1.0 and worst_d <= 1.0 and np.all(dist2 >= 0.0), what
    assert np.all(np.diff(dist2, axis=1) >= 0.0), f"{what}: dist2 not ascending"


# ------------------------------------------------------------------ search: values and indices -------------------------------
@pytest.mark.parametrize("d,n,nq,k,precision", [(64, 1000, 48, 4, "fp16"), (256, 3000, 80, 1, "fp16"), (1024, 1000, 80, 4, "fp16"),
                                                (1024, 1000, 80, 8, "bf16"), (2048, 500, 33, 4, "fp16"), (96, 700, 300, 3, "bf16")])
def test_search_values_against_the_oracle(lib, d, n, nq, k, precision):
    x, q = br.rows16((n, d), 0, precision), br.rows16((nq, d), 1, precision)
    idx, dist2 = _search(q, x, k)
    _check_values(q, x, k, idx, dist2, f"d {d} n {n} nq {nq} k {k} {precision}")


@pytest.mark.parametrize("d,n,nq,k", [(64, 1000, 48, 4), (256, 3000, 80, 1)])
def test_search_indices_against_the_oracle(lib, d, n, nq, k):
    """Check 2: the oracle's own list for every query it marks as separated; at most 5 % of the queries may be left out."""
    x, q = br.rows16((n, d), 0), br.rows16((nq, d), 1)
    sure = br.separated(q, x, k)
    assert (~sure).sum() <= 0.05 * nq
    idx, _ = _search(q, x, k)
    assert np.array_equal(idx[sure], br.search(q, x, k)[0][sure])


@pytest.mark.parametrize("d,precision", list(itertools.product((32, 64, 1024), ("fp16", "bf16"))))
def test_search_shapes(lib, d, precision):
    """Check 3: n in {k, 1, 63, 64, 65, 1000} x nq in {1, 15, 17, 80} x k in {1, 4, 8}; the winner of query 0 planted at index 0, at
    n - 1 and inside the ragged last chunk; one row of large norm."""
    for n_name, nq, k in itertools.product(("k", 1, 63, 64, 65, 1000), (1, 15, 17, 80), (1, 4, 8)):
        n = k if n_name == "k" else n_name
        if k > n:
            continue
        for plant in sorted({0, n - 1, max(n - 3, 0)}):
            x, q = br.rows16((n, d), 10 + n, precision), br.rows16((nq, d), 11 + nq, precision)
            if n > 5:
                x[5] = (x[5].float() * 30.0).to(x.dtype)
            x[plant] = q[0]
            idx, dist2 = _search(q, x, k)
            what = f"d {d} {precision} n {n} nq {nq} k {k} plant {plant}"
            assert idx[0, 0] == plant and dist2[0, 0] <= br.dist2_bound(q[:1], x)[0], what
            _check_values(q, x, k, idx, dist2, what)


# ------------------------------------------------------------------ search: ties, position independence ----------------------
def test_ties_go_to_the_smaller_index(lib):
    x, q = br.rows16((1000, 64), 3), br.rows16((17, 64), 4)
    for i in (10, 500, 997):
        x[i] = x[3]
    x[40] = x[41]
    q[0], q[1] = x[3], x[41]
    idx, dist2 = _search(q, x, 8)
    assert idx[0, :4].tolist() == [3, 10, 500, 997] and idx[1, :2].tolist() == [40, 41]
    assert np.all(dist2[0, :4] == dist2[0, 0]) and 0.0 <= dist2[0, 0] <= br.dist2_bound(q[:1], x)[0]
    _check_values(q, x, 8, idx, dist2, "ties")


@pytest.mark.parametrize("d,precision", [(64, "fp16"), (1024, "bf16")])
def test_scores_do_not_depend_on_position_or_batch(lib, d, precision):
    n, nq, k = 1000, 80, 4
    x, q = br.rows16((n, d), 5, precision), br.rows16((nq, d), 6, precision)
    idx, dist2 = _search(q, x, k)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7))
    idx_p, dist2_p = _search(q, x[perm], k)                    # row i of the permuted database is row perm[i]
    assert np.array_equal(dist2_p.view(np.uint32), dist2.view(np.uint32))
    pad = np.pad(dist2, ((0, 0), (1, 1)), constant_values=-1.0)
    untied = (pad[:, 1:-1] != pad[:, :-2]) & (pad[:, 1:-1] != pad[:, 2:])
    assert untied.mean() > 0.9 and np.array_equal(perm.numpy()[idx_p][untied], idx[untied])
    singles = [_search(q[i:i + 1], x, k) for i in range(nq)]
    assert np.array_equal(np.concatenate([s[0] for s in singles]), idx)
    assert np.array_equal(np.concatenate([s[1] for s in singles]).view(np.uint32), dist2.view(np.uint32))
    again = _search(q, x, k)
    assert np.array_equal(again[0], idx) and np.array_equal(again[1].view(np.uint32), dist2.view(np.uint32))


# ------------------------------------------------------------------ search: work distribution -------------------------------
@pytest.fixture(scope="module")
def cap(lib_built):
    """``cap(v)`` sets the process-wide workgroup cap through a small backbone's handle; it is back at 0 when the module is done."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    bb = ResNet50Backbone(seed=0, max_batch=1).to("cuda:0").eval()

    def set_cap(v):
        bb.set_option("cu_cap", int(v))

    set_cap.bb = bb
    try:
        yield set_cap
    finally:
        bb.set_option("cu_cap", 0)
        bb.close()


def _chunks(n, d):
    """The launcher's arithmetic (csrc/r50_abi.hip): chunks of 32 database rows up to d = 1024, 16 above; the grid is
    min(chunks, CU budget)."""
    rows = 32 if d <= 1024 else 16
    return (n + rows - 1) // rows


@pytest.mark.parametrize("d,n,nq,k,precision", [(64, 1000, 80, 4, "fp16"), (1024, 1000, 80, 8, "bf16"), (2048, 300, 17, 4, "fp16"),
                                                (64, 200, 300, 1, "fp16")])
def test_same_bits_under_every_cap(lib, cap, d, n, nq, k, precision):
    x, q = br.rows16((n, d), 8, precision), br.rows16((nq, d), 9, precision)
    try:
        cap(0)
        idx, dist2 = _search(q, x, k)
        reached = 0
        for c in CAPS:
            if _chunks(n, d) <= c:
                continue                                       # the uncapped launch over again
            reached += 1
            assert _chunks(n, d) > c                           # some workgroup walks several chunks
            cap(c)
            idx_c, dist2_c = _search(q, x, k)
            assert np.array_equal(idx_c, idx) and np.array_equal(dist2_c.view(np.uint32), dist2.view(np.uint32)), c
    finally:
        cap(0)
    assert reached >= 2 and cap.bb.get_option("cu_cap") == 0
    _check_values(q, x, k, idx, dist2, f"caps d {d}")


# ------------------------------------------------------------------ search: refusals ------------------------------------------
def test_refusals_touch_nothing(lib):
    from implementation_phd_lab_vision_amd.baselines import row_norm2
    n, nq, d, k = 100, 5, 64, 4
    x, q = br.rows16((n, d), 0).to(DEV), br.rows16((nq, d), 1).to(DEV)
    x48, q48 = br.rows16((n, 48), 0).to(DEV), br.rows16((nq, 48), 1).to(DEV)
    xn = row_norm2(x)
    idx = torch.full((nq, 8), -7, dtype=torch.int32, device=DEV)
    dist2 = torch.full((nq, 8), -7.0, dtype=torch.float32, device=DEV)
    ws_bytes = int(lib.r50_op_nn_search_workspace(nq, n, k))
    assert ws_bytes > 0 and lib.r50_op_nn_search_workspace(nq, n, 0) == 0 and lib.r50_op_nn_search_workspace(nq, n, 9) == 0
    ws = torch.full((int(lib.r50_op_nn_search_workspace(nq, n, 8)),), 0x5A, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()                                  # noqa: E731
    good = [P(q), nq, P(x), n, d, 1, P(xn), k, P(idx), P(dist2), P(ws), ws.numel(), stream]

    def call(**kw):
        a = list(good)
        for name, v in kw.items():
            a[{"q": 0, "nq": 1, "x": 2, "n": 3, "d": 4, "et": 5, "xn": 6, "k": 7, "idx": 8, "dist2": 9, "ws": 10, "ws_bytes": 11}[name]] = v
        return lib.r50_op_nn_search(*a)

    bad = [dict(k=0), dict(k=9), dict(k=5, n=4), dict(d=48, q=P(q48), x=P(x48)), dict(d=0), dict(d=4096), dict(nq=0), dict(et=2),
           dict(q=None), dict(x=None), dict(xn=None), dict(idx=None), dict(dist2=None), dict(ws=None),
           dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"r50_op_nn_search" in lib.r50_last_error(None)
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((dist2 == -7.0).all()) and bool((ws == 0x5A).all())
    assert lib.r50_op_row_norm2(None, n, d, 1, P(xn), stream) == -1 and lib.r50_op_row_norm2(P(x), n, 12, 1, P(xn), stream) == -1
    assert call() == 0                                          # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert bool((idx.view(-1)[: nq * k] >= 0).all()) and bool((idx.view(-1)[nq * k:] == -7).all())      # (nq, k) written, nothing after
    from implementation_phd_lab_vision_amd import baselines
    with pytest.raises(ValueError):
        baselines.nn_search(q, x, xn, 9)
    with pytest.raises(ValueError):
        baselines.nn_search(q.cpu(), x.cpu(), xn.cpu(), 1)      # no CPU fallback
    with pytest.raises(ValueError):
        baselines.nn_search(q48, x, xn, 1)


def test_row_norm2_is_the_rounded_fp64_sum(lib):
    from implementation_phd_lab_vision_amd.baselines import row_norm2
    for precision, d in (("fp16", 1024), ("bf16", 2048), ("fp16", 40)):
        x = br.rows16((131, d), 2, precision)
        want = (br.f64(x) ** 2).sum(axis=1)
        got = row_norm2(x.to(DEV)).cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * want * (1 + 1e-6)), (precision, d)


# ------------------------------------------------------------------ the forecasts op ------------------------------------------
def test_forecasts_equal_the_restatement_bit_for_bit(lib):
    from implementation_phd_lab_vision_amd import baselines
    i_len, t_db, n_db = 3, 30, 9
    names = baselines.BASELINES
    for b, k, j, p in itertools.product((1, 5), (1, 3), (1, 17), (1, 25)):
        a1, a0 = br.grid_poses((b, j, 3), 1 + b), br.grid_poses((b, j, 3), 2 + j)
        dbj = br.grid_poses((n_db, t_db, j, 3), 3 + k)
        nn_row = torch.randint(0, n_db, (b, k), generator=torch.Generator().manual_seed(p + k), dtype=torch.int32)
        root = 0 if j == 1 else 2
        want = br.forecasts(a1, a0, nn_row, dbj, i_len, p, names, root)
        for r in range(1, 4):
            for which in itertools.combinations(names, r):     # every combination of wanted (non-null) outputs
                got = baselines.baseline_forecasts(a1.to(DEV), a0.to(DEV) if "const_vel" in which else None,
                                                   nn_row.to(DEV) if "nn" in which else None, dbj.to(DEV) if "nn" in which else None,
                                                   i_len, p, which, root)
                assert set(got) == set(which)
                for name in which:
                    assert got[name].shape == (b, p, j, 3)
                    assert np.array_equal(got[name].cpu().numpy().view(np.uint32), want[name].view(np.uint32)), (b, k, j, p, which, name)


def test_forecasts_refusals(lib):
    from implementation_phd_lab_vision_amd import baselines
    a = br.grid_poses((2, 17, 3), 1).to(DEV)
    dbj = br.grid_poses((4, 8, 17, 3), 2).to(DEV)
    rows = torch.zeros((2, 1), dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((2, 5, 17, 3), -7.0, device=DEV)
    P = lambda t: t.data_ptr()                                  # noqa: E731
    for args in ((None, P(a), P(rows), P(dbj), 4, 2, 1, 8, 17, 0, 3, 5, P(out), None, None, stream),          # no a1
                 (P(a), None, P(rows), P(dbj), 4, 2, 1, 8, 17, 0, 3, 5, None, P(out), None, stream),          # const_vel without a0
                 (P(a), P(a), None, P(dbj), 4, 2, 1, 8, 17, 0, 3, 5, None, None, P(out), stream),             # nn without rows
                 (P(a), P(a), P(rows), P(dbj), 4, 2, 1, 8, 17, 0, 3, 5, None, None, None, stream),            # no output
                 (P(a), P(a), P(rows), P(dbj), 4, 2, 9, 8, 17, 0, 3, 5, None, None, P(out), stream),          # k = 9
                 (P(a), P(a), P(rows), P(dbj), 4, 2, 1, 8, 17, 0, 4, 5, None, None, P(out), stream),          # 4 + 5 > 8 frames
                 (P(a), P(a), P(rows), P(dbj), 4, 2, 1, 8, 17, 17, 3, 5, P(out), None, None, stream)):        # root = joints
        assert lib.r50_op_baseline_forecasts(*args) == -1
        assert b"r50_op_baseline_forecasts" in lib.r50_last_error(None)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    with pytest.raises(ValueError, match="input_len >= 2"):
        baselines.baseline_forecasts(a, a, None, None, 1, 5, ("const_vel",))
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        baselines.baseline_forecasts(a, None, torch.full((2, 1), 4, dtype=torch.int32, device=DEV), dbj, 3, 5, ("nn",))


# ------------------------------------------------------------------ module ----------------------------------------------------
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp("baselines")
    return bd.make_baselines_cache(base / "features"), rd.make_preprocessed_tree(base / "videos")


@pytest.fixture(scope="module")
def world(lib, trees):
    """(head, state dict, test store, train store, group names, group ids): built once, left unchanged."""
    from implementation_phd_lab_vision_amd import protocols, results
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    sd = lo.synthetic_head_state_dict(1024, 2, seed=2)
    head = results.build_head(sd, DEV)
    test = DeviceFeatureStore(str(trees[0]), subjects=[9], test_set=True, device=DEV)
    train = DeviceFeatureStore(str(trees[0]), subjects=[1, 6, 7, 8], device=DEV)
    assert (len(test), len(train)) == (rd.N_S9, bd.N_S1)
    names, ids = protocols.action_groups(test.item_actions())
    return head, sd, test, train, names, ids


I_LEN, P_LEN = 3, 5


def test_observe_is_the_observed_part_of_the_rollout(world):
    head, _, test, _, _, _ = world
    feats = test.get_batch(list(range(len(test))))[0]
    phi, joints = head.observe(feats, I_LEN)
    assert phi.shape == (len(test), I_LEN, 1024) and phi.dtype == torch.float16 and joints.dtype == torch.float32
    assert torch.equal(joints, head.joints(feats[:, :I_LEN]))
    poisoned = feats.clone()
    poisoned[:, I_LEN:] = float("nan")                          # it never sees the future
    assert torch.equal(head.observe(poisoned, I_LEN)[0], phi)
    seen = []
    inner = head._temporal_net

    def spy(x, b, t, net, nb):
        out = inner(x, b, t, net, nb)
        if net == "f_movie":
            seen.append(out.clone())
        return out

    head._temporal_net = spy
    try:
        head.rollout(feats, I_LEN, P_LEN)
    finally:
        del head._temporal_net
    assert len(seen) == 1 and torch.equal(seen[0].view(len(test), I_LEN, 1024), phi)      # the rows in front of the sequence buffer
    with pytest.raises(ValueError):
        head.observe(feats, 0)
    with pytest.raises(ValueError):
        head.observe(feats, rd.SEQ_LEN + 1)


def test_evaluate_baselines_against_the_references(world):
    from implementation_phd_lab_vision_amd import baselines, forecast, protocols
    head, _, test, train, names, ids = world
    g = len(names)
    db = baselines.StripDatabase.build(head, train, I_LEN)
    assert len(db) == bd.N_S1 and db.keys.shape == (bd.N_S1, 1024) and db.keys.dtype == torch.float16
    assert db.joints.data_ptr() == train.joints3d.data_ptr()   # a view: no copy of the joints
    feats_tr = train.get_batch(list(range(len(train))))[0]
    assert torch.equal(db.keys, head.observe(feats_tr, I_LEN)[0][:, I_LEN - 1])
    assert torch.equal(db.norm2, baselines.row_norm2(db.keys)) and torch.equal(db.rows.long(), train._row)

    feats, gt = test.get_batch(list(range(len(test))))[:2]
    gt = gt.float().contiguous()
    for anchor, k in (("pred", 1), ("gt", 3)):
        res = baselines.evaluate_baselines(head, test, db, ids, names, I_LEN, P_LEN, baselines.BASELINES, nn_k=k, anchor=anchor)
        assert res["names"] == ("model",) + baselines.BASELINES and res["clips"].tolist() == np.bincount(ids).tolist()
        # the retrieval, by check 1's bound: the true distance of the r-th retrieved strip within 2 E_q of the oracle's r-th smallest
        phi, obs = head.observe(feats, I_LEN)
        fb = baselines.forecast_batch(head, db, feats, gt, I_LEN, P_LEN, baselines.BASELINES, k, anchor)
        q16 = phi[:, I_LEN - 1].cpu()
        _check_values(q16, db.keys.cpu(), k, fb["nn_index"].cpu().numpy().astype(np.int64), fb["nn_dist2"].cpu().numpy(), f"strips {anchor}")
        assert abs(res["nn_dist2_mean"] - float(fb["nn_dist2"].double().mean())) <= 1e-12 * res["nn_dist2_mean"]
        # the forecasts: the numpy restatement given the op's own neighbour indices, bit for bit
        src = obs if anchor == "pred" else gt
        rows = db.rows.cpu()[fb["nn_index"].cpu().long()]
        want = br.forecasts(src[:, I_LEN - 1], src[:, I_LEN - 2], rows, train.joints3d, I_LEN, P_LEN, baselines.BASELINES)
        preds = {"model": head.rollout(feats, I_LEN, P_LEN)[1]}
        for name in baselines.BASELINES:
            assert np.array_equal(fb[name].cpu().numpy(), want[name]), (anchor, name)
            preds[name] = torch.from_numpy(want[name])
        # the sums: numpy fp64 on those predictions
        for name in res["names"]:
            hs = br.horizon_sums(preds[name], gt, I_LEN)
            np.testing.assert_allclose(res[name]["mpjpe"], hs[:P_LEN] / (len(test) * 17), rtol=1e-9, atol=0)
            per, all_, _ = pr.values_from_sums(pr.protocol_sums(preds[name].cpu(), gt.cpu(), I_LEN, ids, g), g, P_LEN)
            np.testing.assert_allclose(res[name]["per_action"], per, rtol=1e-9, atol=1e-15)
            np.testing.assert_allclose(res[name]["p1"], all_[:, 0], rtol=1e-9, atol=1e-15)
            np.testing.assert_allclose(res[name]["p2"], all_[:, 1], rtol=1e-9, atol=1e-15)
        # the model's rows: the existing passes' numbers exactly
        roll = forecast.evaluate_rollout(head, test, I_LEN, P_LEN)
        prot = protocols.evaluate_protocols(head, test, ids, names, I_LEN, P_LEN)
        assert res["model"]["mpjpe"].tolist() == roll["mpjpe"]
        assert np.array_equal(res["model"]["p1"], prot["future_all"][:, 0]) and np.array_equal(res["model"]["p2"], prot["future_all"][:, 1])
        assert np.array_equal(res["model"]["per_action"], prot["future"])
    only = baselines.evaluate_baselines(head, test, None, ids, names, 1, P_LEN, ("const_pose",), batch_size=4)
    assert only["names"] == ("model", "const_pose") and np.isnan(only["nn_dist2_mean"])
    with pytest.raises(ValueError, match="input_len >= 2"):
        baselines.evaluate_baselines(head, test, None, ids, names, 1, P_LEN, ("const_vel",))
    with pytest.raises(ValueError):
        baselines.evaluate_baselines(head, test, None, ids, names, I_LEN, P_LEN, ("nn",))
    with pytest.raises(ValueError):
        baselines.evaluate_baselines(head, test, db, ids, names, I_LEN, P_LEN, ("nn",), nn_k=9)


def test_a_database_of_the_test_clips_retrieves_each_clip_itself(world):
    """The stores are passed directly (the CLI would refuse the overlap).  With the ground-truth anchor the retrieved future IS the
    clip's future, re-rooted: out = fl(r + fl(x - r)) with r the clip's own root at frame I - 1, so each coordinate is within
    u (|x - r| + |x|) (1 + u) <= 3 u M of x (M the largest |coordinate|), and P1, a mean of norms of differences of two such joints,
    is at most 2 sqrt(3) * 3 u M."""
    from implementation_phd_lab_vision_amd import baselines
    head, _, test, _, names, ids = world
    db = baselines.StripDatabase.build(head, test, I_LEN)
    feats, gt = test.get_batch(list(range(len(test))))[:2]
    fb = baselines.forecast_batch(head, db, feats, gt.float().contiguous(), I_LEN, P_LEN, ("nn",), 1, "gt")
    assert fb["nn_index"].view(-1).tolist() == list(range(len(test)))
    res = baselines.evaluate_baselines(head, test, db, ids, names, I_LEN, P_LEN, ("nn",), nn_k=1, anchor="gt")
    bound = 2.0 * np.sqrt(3.0) * 3.0 * br.U * float(gt.abs().max())
    print(f"self-retrieval: largest nn P1 {res['nn']['p1'].max():.3e} (bound {bound:.3e})")
    assert np.all(res["nn"]["p1"] <= bound) and np.all(res["nn"]["p1"] >= 0.0)


# ------------------------------------------------------------------ CLI -------------------------------------------------------
def _cli(argv):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "implementation_phd_lab_vision_amd.results", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"results exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def _parse(line):
    """{metric: {'@h' | 'mean': mm}} of one predictor line."""
    out = {}
    for key in ("mpjpe", "p1", "p2"):
        vals = {}
        for tok in line.split(f"{key} (mm) ")[1].split(" | "):
            name, val = tok.split(": ")
            vals[name] = float(val)
            if name == "mean":
                break
        out[key] = vals
    return out


def test_results_cli_baselines(world, trees, tmp_path):
    from implementation_phd_lab_vision_amd import baselines, results
    head, sd, test, train, names, ids = world
    features, videos = trees
    ckpt = tmp_path / "model.pt"
    torch.save(sd, ckpt)
    base = ["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(ckpt), "--seq-len", str(rd.SEQ_LEN),
            "--batch-size", "4", "--save-n", "3", "--video-size", "32", "--video-reader", "tests.results_data:read_video",
            "--input-len", str(I_LEN), "--pred-len", str(P_LEN)]
    out_off, out_on = tmp_path / "off.npz", tmp_path / "on.npz"
    so_off = _cli(base + ["--out", str(out_off)])
    so_on = _cli(base + ["--out", str(out_on), "--baselines", "--nn-k", "2"])

    db = baselines.StripDatabase.build(head, train, I_LEN)
    res = baselines.evaluate_baselines(head, test, db, ids, names, I_LEN, P_LEN, baselines.BASELINES, nn_k=2)
    lines = baselines.baseline_lines(res, I_LEN, P_LEN)
    on_lines = so_on.replace(str(out_on), str(out_off)).splitlines()
    for line in lines:
        assert line in on_lines, line
    assert lines[0].startswith(f"Baselines | input {I_LEN} | pred {P_LEN} | clips {rd.N_S9} | anchor pred | predictors 4 | nn k 2 | ")
    new_lines = [l for l in on_lines if l.startswith("Baselines") or l in lines]
    assert len(new_lines) == len(lines) + 1 and not any(l.startswith("Baselines") for l in so_off.splitlines())
    timing = ("Results time",)
    assert [l for l in on_lines if l not in new_lines and not l.startswith(timing)] == \
           [l for l in so_off.splitlines() if not l.startswith(timing)]                  # the rest of stdout as without the flag

    z_off, z_on = np.load(out_off, allow_pickle=True), np.load(out_on, allow_pickle=True)
    assert set(z_off.files) == {"video", "joints3d", "predicted3djoints", "joints2d", "K", "meta", "test_metrics",
                                "predicted_future3djoints", "future_mpjpe", "rollout_lens"}                  # exactly today's keys
    new = {"baseline_names", "baseline_mpjpe", "baseline_p1", "baseline_p2", "baseline_actions", "baseline_per_action", "baseline_anchor",
           "nn_index", "nn_dist2", "nn_future3djoints"}
    assert set(z_on.files) == set(z_off.files) | new
    for key in z_off.files:
        if z_off[key].dtype != object:
            assert np.array_equal(z_off[key], z_on[key]), key
    assert z_on["baseline_names"].tolist() == ["model", "const_pose", "const_vel", "nn"] and str(z_on["baseline_anchor"]) == "pred"
    assert z_on["baseline_actions"].tolist() == names
    for i, name in enumerate(res["names"]):
        for key in ("mpjpe", "p1", "p2"):
            assert np.array_equal(z_on["baseline_" + key][i], res[name][key].astype(np.float32)), (name, key)
        assert np.array_equal(z_on["baseline_per_action"][i], res[name]["per_action"].astype(np.float32))
        got = _parse(next(l for l in on_lines if l.startswith(f"  {name} | ")))           # the lines parse back to the .npz values
        for key in ("mpjpe", "p1", "p2"):
            row = z_on["baseline_" + key][i].astype(np.float64)
            for h in (1, 5):
                assert abs(got[key][f"@{h}"] - row[h - 1] * 1000.0) <= 0.005 + 1e-4 * row[h - 1] * 1000.0, (name, key, h)
            assert abs(got[key]["mean"] - row.mean() * 1000.0) <= 0.005 + 1e-4 * row.mean() * 1000.0
    _, dump_idx = results.loader_batch_order(len(test), 4, 0)
    feats, gt = test.get_batch(dump_idx)[:2]
    fb = baselines.forecast_batch(head, db, feats[:3], gt[:3].float().contiguous(), I_LEN, P_LEN, ("nn",), 2, "pred")
    assert z_on["nn_index"].shape == (3, 2) and np.array_equal(z_on["nn_index"], fb["nn_index"].cpu().numpy())
    assert np.array_equal(z_on["nn_dist2"], fb["nn_dist2"].cpu().numpy())
    assert z_on["nn_future3djoints"].shape == (3, P_LEN, 17, 3) and np.array_equal(z_on["nn_future3djoints"], fb["nn"].cpu().numpy())
