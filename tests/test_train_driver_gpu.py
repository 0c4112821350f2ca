"""The phase-1 training driver on the MI355X (src/train.py:219-465): the pose-metric kernel, ``joints()``, ``evaluate`` against the
CPU oracle, one driver epoch against a hand loop of ``train_step``, the CLI's checkpoints in the reference's format (loaded by
torch.optim.AdamW over the oracle's parameters), checkpoint round trips and early stopping.  CLI runs are fresh child processes
under a time limit."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests.train_driver_data import make_feature_cache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return make_feature_cache(tmp_path_factory.mktemp("cache4"), n_vars=4)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _head(seed=0, cls="train"):
    from implementation_phd_lab_vision_amd import model, train
    from oracle import lifting_oracle as lo
    sd = lo.synthetic_head_state_dict(1024, 2, seed)
    h = (train.TrainableHead if cls == "train" else model.PHDFor3DJoints)(1024, 17, 2)
    h.load_state_dict(sd)
    h.to(DEV)
    return h, sd


def _cli(*argv, timeout=900):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "implementation_phd_lab_vision_amd.train", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"driver exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout, [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


# ------------------------------------------------------------------ kernel ----------------------------------------------------
def test_pose_metrics_kernel(lib):
    from implementation_phd_lab_vision_amd import _lib
    for k, sizes in enumerate((((1, 1), (7, 17), (3, 5)), ((1280, 17), (4999, 17), (11, 3)), ((5880, 17), (1, 17), (2, 1)))):
        runs = []
        for _ in range(2):                              # the same inputs twice: the same bits
            g = torch.Generator().manual_seed(5 + k)
            acc = torch.zeros(3, dtype=torch.float64, device=DEV)
            want = torch.zeros(3, dtype=torch.float64)
            for rows, joints in sizes:
                p = torch.randn(rows, joints, 3, generator=g)
                gt = p + 0.1 * torch.randn(rows, joints, 3, generator=g)
                p_d, gt_d = p.to(DEV), gt.to(DEV)
                _lib.check(lib.r50_op_pose_metrics(p_d.data_ptr(), gt_d.data_ptr(), rows, joints, acc.data_ptr(), _stream()), None,
                           "pose_metrics")
                d = (p - gt).double()
                want += torch.tensor([float(d.pow(2).mean()), float(torch.norm(d, dim=-1).mean()), 1.0], dtype=torch.float64)
            got = acc.cpu()
            assert float(got[2]) == len(sizes)
            torch.testing.assert_close(got[:2], want[:2], rtol=1e-6, atol=0)
            runs.append(got)
        assert torch.equal(runs[0], runs[1])
    x = torch.zeros(4, 17, 3, device=DEV)
    acc = torch.zeros(3, dtype=torch.float64, device=DEV)
    for args in ((None, x.data_ptr(), 4, 17, acc.data_ptr()), (x.data_ptr(), None, 4, 17, acc.data_ptr()),
                 (x.data_ptr(), x.data_ptr(), 4, 17, None), (x.data_ptr(), x.data_ptr(), 0, 17, acc.data_ptr()),
                 (x.data_ptr(), x.data_ptr(), 4, 0, acc.data_ptr()), (x.data_ptr(), x.data_ptr(), -3, 17, acc.data_ptr())):
        assert lib.r50_op_pose_metrics(*args, _stream()) == -1
    assert b"pose_metrics" in lib.r50_last_error(None)
    assert torch.equal(acc.cpu(), torch.zeros(3, dtype=torch.float64))


def test_joints_equal_full_forward(lib):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 9, 2048, generator=g).abs().to(DEV)
    for cls in ("model", "train"):
        h, _ = _head(1, cls)
        assert torch.equal(h.joints(x), h(x)[2])


# ------------------------------------------------------------------ evaluate --------------------------------------------------
def test_evaluate_matches_oracle(lib, cache):
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    store = DeviceFeatureStore(str(cache), subjects=[5], device=DEV)
    assert len(store) == 10                                        # batches of 4: 4, 4, 2
    head, sd = _head(3)
    head.train()
    before = head.flat_master.clone()
    loss, mpjpe, l3d, l2d = train.evaluate(head, store, 4)
    assert head.training and torch.equal(head.flat_master, before) and l2d == 0.0 and loss == l3d
    ls, ms = [], []
    for s in range(0, 10, 4):
        feats, j3d = store.get_batch(list(range(s, min(s + 4, 10))))[:2]
        pred = lo.forward_reference(sd, feats.cpu())[2]
        ls.append(float((pred - j3d.cpu()).pow(2).mean()))
        ms.append(float(torch.norm(pred - j3d.cpu(), dim=-1).mean()))
    want_l, want_m = sum(ls) / 3, sum(ms) / 3
    assert abs(mpjpe - want_m) <= 5e-3 * want_m, (mpjpe, want_m)
    assert abs(loss - want_l) <= 1e-2 * want_l, (loss, want_l)
    head.eval()
    assert train.evaluate(head, store, 4) == (loss, mpjpe, l3d, l2d) and not head.training


# ------------------------------------------------------------------ driver ----------------------------------------------------
def test_driver_epoch_equals_hand_loop(lib, cache, tmp_path):
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from implementation_phd_lab_vision_amd.samplers import MixedShardBatchSampler
    out = tmp_path / "run"
    train.main(["--train", str(cache), "--val", str(cache), "--epochs", "3", "--batch-size", "8", "--seed", "7", "--outdir", str(out),
                "--log-every", "0", "--early-stop-patience", "1", "--lr", "2e-4"])
    ckpt = torch.load(out / "last.pt", weights_only=True)
    best = torch.load(out / "best.pt", weights_only=True)
    first = best if best["epoch"] == 0 else None

    store = DeviceFeatureStore(str(cache), subjects=[1, 6, 7, 8], augment=True, device=DEV)
    sampler = MixedShardBatchSampler(store, batch_size=8, shuffle=True, drop_last=True, seed=0)
    head = train.TrainableHead(1024, 17, 2)
    head.load_state_dict(train.default_state_dict(1024, 17, 2, seed=7))
    head.to(DEV)
    optim, scaler, sched = train.AdamW(head, lr=2e-4), train.GradScaler(), train.CosineLR(2e-4, 3)
    for epoch in range(ckpt["epoch"] + 1):
        sampler.set_epoch(epoch)
        optim.lr = sched.lr
        for it, idx in enumerate(sampler):
            feats, j3d = store.get_batch(idx)[:2]
            masks = head.make_dropout_masks(8, feats.shape[1], generator=train.dropout_generator(7, epoch, it, head._device))
            head.train_step(feats, j3d, optim, scaler, masks=masks)
        sched.step()
        optim.lr = sched.lr
        if epoch == 0 and first is not None:
            _assert_same_as_checkpoint(head, optim, first)
    _assert_same_as_checkpoint(head, optim, ckpt)


def _assert_same_as_checkpoint(head, optim, ckpt):
    from implementation_phd_lab_vision_amd import train
    model = head.state_dict()
    for k in train.trainable_names(2):
        assert torch.equal(ckpt["model"][k], model[k]), k
    mine = optim.state_dict()
    assert mine["param_groups"][0]["lr"] == ckpt["optim"]["param_groups"][0]["lr"]
    for i in range(len(train.trainable_names(2))):
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(mine["state"][i][f], ckpt["optim"]["state"][i][f]), (i, f)


def _oracle_trainable(model_sd, names):
    return [torch.nn.Parameter(model_sd[n].clone()) for n in names]


def test_cli_writes_reference_checkpoints(lib, cache, tmp_path):
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.model import expected_keys
    from oracle import lifting_oracle as lo
    out = tmp_path / "run"
    stdout, epochs = _cli("--train", str(cache), "--val", str(cache), "--epochs", "2", "--batch-size", "8", "--seed", "1",
                          "--outdir", str(out), "--log-every", "0", "--lr", "1e-4")
    assert [e["epoch"] for e in epochs] == [0, 1]
    applied = sum(e["steps"] for e in epochs)
    assert applied > 0
    ref_lr = train.CosineLR(1e-4, 2)
    ref_lr.step(); ref_lr.step()
    sd_keys = lo.synthetic_head_state_dict(1024, 2, 0)
    for name in ("last.pt", "best.pt"):
        ck = torch.load(out / name, weights_only=True)
        assert set(ck) == {"epoch", "best_val", "model", "optim", "args"}
        assert {k: tuple(v.shape) for k, v in ck["model"].items()} == {k: tuple(v.shape) for k, v in sd_keys.items()} \
            == expected_keys(1024, 17, 2)
        lo.forward_reference(ck["model"], torch.rand(1, 3, 2048))       # the oracle runs on it
        params = _oracle_trainable(ck["model"], train.trainable_names(2))
        opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-2)
        opt.load_state_dict(ck["optim"])
        assert opt.state_dict()["param_groups"][0]["initial_lr"] == 1e-4
        assert ck["args"]["seed"] == 1 and ck["args"]["batch_size"] == 8
    last = torch.load(out / "last.pt", weights_only=True)
    assert last["epoch"] == 1
    assert last["optim"]["param_groups"][0]["lr"] == ref_lr.lr
    assert all(float(st["step"]) == applied for st in last["optim"]["state"].values())
    best = torch.load(out / "best.pt", weights_only=True)
    assert best["best_val"] == min(e["val_mpjpe"] for e in epochs)

    # resuming from last.pt at the end of the schedule runs no epoch and keeps the weights
    stdout, ep2 = _cli("--train", str(cache), "--val", str(cache), "--epochs", "2", "--batch-size", "8", "--outdir", str(tmp_path / "r2"),
                       "--resume", str(out / "last.pt"), "--log-every", "0")
    assert ep2 == [] and "Resumed from" in stdout


def test_checkpoint_round_trips(lib, cache, tmp_path):
    from implementation_phd_lab_vision_amd import train
    from oracle import lifting_oracle as lo
    # project -> file -> project
    head, _ = _head(4)
    optim, scaler = train.AdamW(head, lr=3e-4), train.GradScaler(init_scale=1024.0)
    g = torch.Generator(device=DEV).manual_seed(0)
    for s in range(2):
        feats = torch.rand(2, 6, 2048, device=DEV, generator=g)
        gt = torch.randn(2, 6, 17, 3, device=DEV, generator=g) * 0.3
        head.train_step(feats, gt, optim, scaler, masks=head.make_dropout_masks(2, 6, generator=g))
    optim.initial_lr = 5e-4
    train.save_checkpoint(str(tmp_path / "a.pt"), head, optim, 3, 0.25, {"note": "x"})
    h2, _ = _head(9)
    o2 = train.AdamW(h2, lr=1.0)
    ck = train.load_checkpoint(str(tmp_path / "a.pt"), h2, o2)
    assert ck["epoch"] == 3 and ck["best_val"] == 0.25
    assert torch.equal(h2.flat_master, head.flat_master) and torch.equal(h2.flat_w16, head.flat_w16)
    assert torch.equal(o2.exp_avg, optim.exp_avg) and torch.equal(o2.exp_avg_sq, optim.exp_avg_sq)
    assert (o2.step_count, o2.lr, o2.initial_lr) == (optim.step_count, 3e-4, 5e-4) and o2.step_count == 2
    for k in h2._wt:
        assert torch.equal(h2._wt[k], head._wt[k]), k

    # a torch.optim.AdamW checkpoint made on the CPU in the reference's format -> project
    names = train.trainable_names(2)
    sd = lo.synthetic_head_state_dict(1024, 2, 6)
    params = _oracle_trainable(sd, names)
    opt = torch.optim.AdamW(params, lr=2e-3, weight_decay=1e-2)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=5)
    gc = torch.Generator().manual_seed(1)
    for _ in range(3):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gc) * 1e-2
        opt.step()
        sched.step()
    model_sd = dict(sd)
    model_sd.update({n: p.detach().clone() for n, p in zip(names, params)})
    torch.save({"epoch": 2, "best_val": 1.5, "model": model_sd, "optim": opt.state_dict(), "args": {}}, tmp_path / "ref.pt")
    h3, _ = _head(0)
    o3 = train.AdamW(h3)
    train.load_checkpoint(str(tmp_path / "ref.pt"), h3, o3)
    assert o3.step_count == 3 and o3.lr == opt.param_groups[0]["lr"] and o3.initial_lr == 2e-3
    back, want = o3.state_dict(), opt.state_dict()
    model_back = h3.state_dict()
    for i, n in enumerate(names):
        assert torch.equal(model_back[n], model_sd[n]), n
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][f], want["state"][i][f]), (n, f)
    assert {k: v for k, v in back["param_groups"][0].items()} == want["param_groups"][0]
    assert torch.equal(h3.flat_w16, h3.flat_master.to(torch.float16))


def test_early_stopping_with_zero_lr(lib, cache, tmp_path):
    out = tmp_path / "run"
    stdout, epochs = _cli("--train", str(cache), "--val", str(cache), "--epochs", "6", "--batch-size", "8", "--lr", "0",
                          "--early-stop-patience", "1", "--outdir", str(out), "--log-every", "0")
    assert [e["epoch"] for e in epochs] == [0, 1]
    assert epochs[0]["val_mpjpe"] == epochs[1]["val_mpjpe"] and epochs[0]["val_loss"] == epochs[1]["val_loss"]
    assert "Early stopping triggered at epoch 2" in stdout
    best, last = torch.load(out / "best.pt", weights_only=True), torch.load(out / "last.pt", weights_only=True)
    assert best["epoch"] == 0 and last["epoch"] == 1 and best["best_val"] == epochs[0]["val_mpjpe"]
    for k, v in best["model"].items():
        assert torch.equal(v, last["model"][k]), k
