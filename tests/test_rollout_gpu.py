"""The autoregressive rollout on the MI355X: the time-major GroupNorm kernel against the batch-major one,
the per-horizon metrics kernel against torch, ``PHDFor3DJoints.rollout`` against the reference module's rollouts
(tests/golden/rollout_golden.pt) and against the 16-bit-emulating restatement, ``forecast.evaluate_rollout`` and the results CLI's
``--pred-len``."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import results_data as rd
from tests.helpers import GOLDEN
from tests.rollout_reference import case_feats, horizon_sums, rollout_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]

# Tolerances, relative L2 over clips and channels, checked at EVERY horizon k.  An fp64 emulation of the device's 16-bit storage
# (tests/rollout_reference.py, store16) measured against the exact program on the three golden cases: fp16 0.82e-3 .. 1.7e-3,
# bf16 6.7e-3 .. 1.31e-2 (latents and joints, any horizon; the 25-step case grows from 0.9e-3 to 1.5e-3 in fp16, 7e-3 to 1.3e-2 in
# bf16).  So the head's own tolerances (4e-3 fp16, 3e-2 bf16) leave >= 2.3x headroom at every horizon and are kept.  Against the
# emulation itself the device differs only where fp32 summation order flips a 16-bit rounding: half the head's tolerance, i.e.
# about the emulation's own largest error, bounds that (the MI355X measured at most 1.26e-3 fp16 and 8.9e-3 bf16 from it).
TOL = {"fp16": 4e-3, "bf16": 3e-2}
EMU_TOL = {"fp16": 2e-3, "bf16": 1.5e-2}


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel_per_horizon(got, want):
    """(P,) relative L2 error of horizon k over clips and the remaining dims; got / want (B, P, ...)."""
    g, w = got.double().cpu(), want.double().cpu()
    b, p = w.shape[:2]
    return ((g - w).reshape(b, p, -1).norm(dim=(0, 2)) / w.reshape(b, p, -1).norm(dim=(0, 2)).clamp_min(1e-30))


def _head(d, nb, seed, precision="fp16"):
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    from oracle import lifting_oracle as lo
    sd = lo.synthetic_head_state_dict(d, nb, seed)
    h = PHDFor3DJoints(d, 17, nb, precision=precision)
    h.load_state_dict(sd)
    return h.to(DEV).eval(), sd


# ------------------------------------------------------------------ kernels ---------------------------------------------------
@pytest.mark.parametrize("et", [1, 0])
@pytest.mark.parametrize("t", [1, 2, 3, 40])
def test_gn_tm_matches_batch_major_kernel(lib, et, t):
    dt = torch.float16 if et else torch.bfloat16
    b, c, groups = 3, 256, 32
    g = torch.Generator().manual_seed(10 * t + et)
    x = (torch.randn(b, t, c, generator=g) * 2 + 0.3).to(dt).to(DEV)
    gamma = (1 + 0.1 * torch.randn(c, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(c, generator=g)).to(DEV)
    ref = torch.empty((b * t, 3 * c), dtype=dt, device=DEV)
    assert lib.r50_op_gn_relu_causal3(x.data_ptr(), b, t, c, groups, gamma.data_ptr(), beta.data_ptr(), 1e-5, ref.data_ptr(), et, _stream()) == 0
    ref = ref.view(b, t, 3 * c)
    x_tm = x.transpose(0, 1).contiguous()                                     # (t, b, c)
    for t0 in sorted({0, t - 1, t // 2}):
        rows = (t - t0) * b
        buf = torch.full((rows + 5, 3 * c), 7.0, dtype=dt, device=DEV)        # a guard band behind the output
        assert lib.r50_op_gn_relu_causal3_tm(x_tm.data_ptr(), b, t, t0, c, groups, gamma.data_ptr(), beta.data_ptr(), 1e-5,
                                             buf.data_ptr(), et, _stream()) == 0
        got = buf[:rows].view(t - t0, b, 3 * c).transpose(0, 1)               # back to (b, t - t0, 3c)
        assert torch.equal(got.view(torch.int16), ref[:, t0:].view(torch.int16)), (t, t0)
        assert torch.all(buf[rows:] == 7.0)
    for bad_t0 in (-1, t):
        assert lib.r50_op_gn_relu_causal3_tm(x_tm.data_ptr(), b, t, bad_t0, c, groups, gamma.data_ptr(), beta.data_ptr(), 1e-5,
                                             buf.data_ptr(), et, _stream()) != 0
    assert b"r50_op_gn_relu_causal3_tm" in lib.r50_last_error(None)
    assert lib.r50_op_gn_relu_causal3_tm(x_tm.data_ptr(), b, t, 0, c, 24, gamma.data_ptr(), beta.data_ptr(), 1e-5, buf.data_ptr(), et,
                                         _stream()) != 0


def test_gn_tm_at_the_head_width(lib):
    """D = 1024 (cg = 32), t = 40, b = 32: the rollout's last step."""
    b, t, c = 32, 40, 1024
    g = torch.Generator().manual_seed(5)
    x = torch.randn(b, t, c, generator=g).half().to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).to(DEV), (0.1 * torch.randn(c, generator=g)).to(DEV)
    ref = torch.empty((b * t, 3 * c), dtype=torch.float16, device=DEV)
    assert lib.r50_op_gn_relu_causal3(x.data_ptr(), b, t, c, 32, gamma.data_ptr(), beta.data_ptr(), 1e-5, ref.data_ptr(), 1, _stream()) == 0
    out = torch.empty((b, 3 * c), dtype=torch.float16, device=DEV)
    x_tm = x.transpose(0, 1).contiguous()
    assert lib.r50_op_gn_relu_causal3_tm(x_tm.data_ptr(), b, t, t - 1, c, 32, gamma.data_ptr(), beta.data_ptr(), 1e-5, out.data_ptr(), 1,
                                         _stream()) == 0
    assert torch.equal(out.view(torch.int16), ref.view(b, t, 3 * c)[:, -1].view(torch.int16))


def test_horizon_metrics_kernel(lib):
    b, t, j, i0, p = 5, 12, 17, 3, 7
    g = torch.Generator().manual_seed(1)
    gt = torch.randn(b, t, j, 3, generator=g)
    pred = gt[:, i0:i0 + p] + 0.05 * torch.randn(b, p, j, 3, generator=g) * torch.arange(1, p + 1).view(1, p, 1, 1)
    want = horizon_sums(pred, gt, i0)
    runs = []
    for _ in range(2):
        acc = torch.zeros(2 * p + 1, dtype=torch.float64, device=DEV)
        assert lib.r50_op_horizon_metrics(pred.contiguous().to(DEV).data_ptr(), gt.to(DEV).data_ptr(), b, p, t, i0, j, acc.data_ptr(),
                                          _stream()) == 0
        runs.append(acc.cpu())
    torch.testing.assert_close(runs[0], want, rtol=1e-6, atol=0)
    assert torch.equal(runs[0], runs[1])                                     # fixed summation order: the same bits
    acc = runs[0].to(DEV)                                                    # it ADDS
    pd, gd = pred.contiguous().to(DEV), gt.to(DEV)
    assert lib.r50_op_horizon_metrics(pd.data_ptr(), gd.data_ptr(), b, p, t, i0, j, acc.data_ptr(), _stream()) == 0
    assert torch.equal(acc.cpu(), 2 * runs[0])
    for args in ((b, p, t, t - p + 1, j), (0, p, t, i0, j), (b, 0, t, i0, j), (b, p, t, -1, j), (b, p, t, i0, 0)):
        assert lib.r50_op_horizon_metrics(pd.data_ptr(), gd.data_ptr(), *args, acc.data_ptr(), _stream()) != 0


# ------------------------------------------------------------------ rollout ---------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_rollout_matches_golden_and_emulation(lib, precision):
    for c in torch.load(GOLDEN / "rollout_golden.pt", map_location="cpu", weights_only=True):
        head, sd = _head(c["latent_dim"], c["number_blocks"], c["seed"], precision)
        feats = case_feats(c["seed"], c["b"], c["t"])
        phi, joints = head.rollout(feats.to(DEV), c["input_len"], c["pred_len"])
        assert phi.shape == c["future_phi"].shape and phi.dtype == torch.float32
        assert joints.shape == c["future_joints"].shape and joints.dtype == torch.float32
        emu = rollout_reference(sd, feats, c["input_len"], c["pred_len"], store16=precision)
        for name, got, want, e in (("phi", phi, c["future_phi"], emu[0]), ("joints", joints, c["future_joints"], emu[1])):
            r_gold, r_emu = _rel_per_horizon(got, want), _rel_per_horizon(got, e)
            print(f"{precision} D{c['latent_dim']} I{c['input_len']} P{c['pred_len']} {name}: vs golden max {float(r_gold.max()):.2e} "
                  f"(last {float(r_gold[-1]):.2e}), vs emulation max {float(r_emu.max()):.2e}")
            assert torch.isfinite(got).all()
            assert bool((r_gold < TOL[precision]).all()), (name, r_gold.tolist())
            assert bool((r_emu < EMU_TOL[precision]).all()), (name, r_emu.tolist())


def test_rollout_ignores_future_features_and_is_deterministic(lib):
    head, _ = _head(128, 2, 8)
    feats = case_feats(8, 3, 12).to(DEV)
    a = head.rollout(feats, 5, 6)
    b = head.rollout(feats, 5, 6)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    nan = feats.clone()
    nan[:, 5:] = float("nan")
    c = head.rollout(nan, 5, 6)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, c))
    d = head.rollout(feats[:, :5].contiguous(), 5, 6)                       # T == input_len is enough
    assert all(torch.equal(x, y) for x, y in zip(a, d))
    for i_len, p_len in ((0, 3), (13, 1), (5, 0)):
        with pytest.raises(ValueError):
            head.rollout(feats, i_len, p_len)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_one_step_rollout_is_the_strip_the_shift_drops(lib, precision):
    """rollout(pred_len=1) = f_AR(phi)[:, -1] of the batch-major head (GEMM tiles differ with the row count: close, not bit-equal)."""
    from implementation_phd_lab_vision_amd import _lib
    from implementation_phd_lab_vision_amd.model import _AR_BLOCKS
    head, _ = _head(1024, 2, 9, precision)
    b, i_len = 4, 15
    feats = case_feats(9, b, i_len + 3).to(DEV)
    phi1, j1 = head.rollout(feats, i_len, 1)
    f = feats[:, :i_len].contiguous()
    x0 = torch.empty((b * i_len, 2048), dtype=head._dtype, device=DEV)
    _lib.check(lib.r50_op_cast_rows(f.data_ptr(), b * i_len, 2048, x0.data_ptr(), 2048, head._et, _stream()), None, "cast")
    phi = head._temporal_net(head._gemm(x0, "input_proj", relu=False), b, i_len, "f_movie", head.number_blocks)
    ar = head._temporal_net(phi, b, i_len, "f_AR", _AR_BLOCKS).view(b, i_len, -1)[:, -1:].float()
    r = _rel_per_horizon(phi1, ar)
    print(f"{precision}: one-step rollout vs batch-major f_AR last row: rel {float(r[0]):.2e}")
    assert float(r[0]) < TOL[precision]
    assert j1.shape == (b, 1, 17, 3)


def test_rollout_on_a_trained_ar_head(lib):
    from implementation_phd_lab_vision_amd import train, train_ar
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    from oracle import lifting_oracle as lo
    sd = lo.synthetic_head_state_dict(256, 2, 11)
    h = train_ar.ARTrainableHead(256, 17, 2)
    h.load_state_dict(sd)
    h.to(DEV).train()
    g = torch.Generator().manual_seed(4)
    feats = torch.randn(3, 10, 2048, generator=g).abs().to(DEV)
    gt = (torch.randn(3, 10, 17, 3, generator=g) * 0.5).to(DEV)
    optim = train.AdamW(h, lr=1e-3)
    assert not h.train_step(feats, gt, optim, train.GradScaler(init_scale=1024.0))[2]
    trained = h.state_dict()
    assert not torch.equal(trained["f_AR.blocks.0.conv1.conv.weight"], sd["f_AR.blocks.0.conv1.conv.weight"])
    kept = [t.clone() for t in (h.flat_master, h.flat_w16, h.flat_grad, optim.exp_avg, optim.exp_avg_sq)]
    step = optim.step_count
    got = h.rollout(feats, 6, 4)
    assert h.training is True and optim.step_count == step
    assert all(torch.equal(a, b) for a, b in zip(kept, (h.flat_master, h.flat_w16, h.flat_grad, optim.exp_avg, optim.exp_avg_sq)))
    plain = PHDFor3DJoints(256, 17, 2)
    plain.load_state_dict(trained)
    want = plain.to(DEV).eval().rollout(feats, 6, 4)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # a phase-1 training head inherits it too (f_AR frozen there: the plain head's numbers)
    th = train.TrainableHead(256, 17, 2)
    th.load_state_dict(sd)
    th.to(DEV).train()
    plain0 = PHDFor3DJoints(256, 17, 2)
    plain0.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(th.rollout(feats, 6, 4), plain0.to(DEV).rollout(feats, 6, 4)))
    assert th.training is True


# ------------------------------------------------------------------ evaluation + CLI ------------------------------------------
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp("rollout")
    return rd.make_results_cache(base / "features"), rd.make_preprocessed_tree(base / "videos")


def test_evaluate_rollout_against_restatement(lib, trees):
    from implementation_phd_lab_vision_amd import forecast
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    store = DeviceFeatureStore(str(trees[0]), subjects=[9], test_set=True, device=DEV)
    head, sd = _head(1024, 2, 6)
    i_len, p_len = 3, 5
    res = forecast.evaluate_rollout(head, store, i_len, p_len)
    assert res["clips"] == len(store) == rd.N_S9 and len(res["mpjpe"]) == len(res["l3d"]) == p_len
    feats, gt = store.get_batch(list(range(len(store))))[:2]
    want = forecast.metrics_from_sums(horizon_sums(rollout_reference(sd, feats.cpu(), i_len, p_len)[1], gt.cpu(), i_len).tolist(),
                                      p_len, 17)
    for k in range(p_len):
        assert res["mpjpe"][k] == pytest.approx(want["mpjpe"][k], rel=5e-3), k
        assert res["l3d"][k] == pytest.approx(want["l3d"][k], rel=1e-2), k
    assert res["mpjpe_mean"] == pytest.approx(sum(res["mpjpe"]) / p_len, rel=1e-12)
    for bs in (2, 7):
        other = forecast.evaluate_rollout(head, store, i_len, p_len, batch_size=bs)
        assert other["clips"] == rd.N_S9
        for key in ("mpjpe", "l3d"):
            assert other[key] == pytest.approx(res[key], rel=1e-5), (bs, key)
    with pytest.raises(ValueError):
        forecast.evaluate_rollout(head, store, 4, 5)                         # 9 > seq_len 8


def test_results_cli_with_rollout(lib, trees, tmp_path):
    from implementation_phd_lab_vision_amd import forecast, results
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    features, videos = trees
    sd = lo.synthetic_head_state_dict(1024, 2, seed=2)
    ckpt = tmp_path / "model.pt"
    torch.save(sd, ckpt)
    out = tmp_path / "batch.npz"
    argv = ["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(ckpt), "--out", str(out),
            "--seq-len", str(rd.SEQ_LEN), "--batch-size", "4", "--save-n", "3", "--video-size", "32",
            "--video-reader", "tests.results_data:read_video", "--input-len", "3", "--pred-len", "5"]
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "implementation_phd_lab_vision_amd.results", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"results exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "Rollout metrics | input 3 | pred 5 | clips 11 | mpjpe (mm) @1: " in r.stdout and "@5: " in r.stdout

    store = DeviceFeatureStore(str(features), subjects=[9], test_set=True, device=DEV)
    head = results.build_head(sd, DEV)
    _, dump_idx = results.loader_batch_order(len(store), 4, 0)
    feats = store.get_batch(dump_idx)[0]
    z = np.load(out, allow_pickle=True)
    assert set(z.files) == {"video", "joints3d", "predicted3djoints", "joints2d", "K", "meta", "test_metrics",
                            "predicted_future3djoints", "future_mpjpe", "rollout_lens"}
    assert z["predicted_future3djoints"].shape == (3, 5, 17, 3) and z["predicted_future3djoints"].dtype == np.float32
    assert np.array_equal(z["predicted_future3djoints"], head.rollout(feats[:3], 3, 5)[1].cpu().numpy())
    want = forecast.evaluate_rollout(head, store, 3, 5)["mpjpe"]
    assert z["future_mpjpe"].dtype == np.float32 and np.array_equal(z["future_mpjpe"], np.array(want, dtype=np.float32))
    assert z["rollout_lens"].tolist() == [3, 5]
    assert np.array_equal(z["predicted3djoints"], head.joints(feats)[:3].cpu().numpy())    # the existing keys are as before
