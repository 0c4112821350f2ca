"""The rollout objective (training f_AR on its own multi-step rollouts) on the MI355X: the time-major
GroupNorm backward against the batch-major one and against fp64 autograd, the two rollout loss kernels against torch, the training
forward against ``rollout``, two ``rollout_train_step``s against the reference module (tests/golden/train_rollout_golden.pt), the
dropout sites against the CPU restatement (tests/rollout_train_reference.py), overflow handling, and the driver."""
import json
from pathlib import Path

import pytest
import torch

from tests.golden.make_golden_train_rollout import batches_for
from tests.helpers import GOLDEN
from tests.rollout_train_reference import train_rollout_steps_reference
from tests.train_driver_data import make_feature_cache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]

# Tolerances against the fixture (fp32 reference module), per golden case (keyed by k) and precision.  Each is 2.5x what the fp64
# emulation of the step's 16-bit storage in both directions (tests/rollout_train_reference.py, store16, loss scale 1024) measured
# against the exact program on the same case:
#                      loss     grad norm  64-entry grad slice  update median / lr
#   k 1  (D 256, I 1)  fp16 3.9e-4  3.6e-3   2.2e-2               0.014
#                      bf16 4.3e-3  1.3e-2   8.8e-2               0.013
#   k 3  (D 64,  I 4)  fp16 4.7e-4  6.7e-2   2.3e-1               0.037
#                      bf16 2.2e-3  9.1e-2   3.6e-1               0.095
#   k 25 (D 256, I 15) fp16 1.6e-3  4.3e-3   7.0e-2               0.008
#                      bf16 3.9e-3  1.2e-2   1.0e-1               0.024
# The D 64 case is the ill-conditioned one (GroupNorm groups of 2 channels over 4-6 frames), not the deep one: 25 steps of BPTT keep
# the gradient norms within 0.5 % in fp16.  Slices the emulation puts more than 20 % off are not compared (that is the format, not
# the kernels); AdamW's first steps move every weight by about +-lr whatever the gradient's size, so an update is judged by the
# median error over its slice (the fraction of sign flips), not its maximum.  The emulation keeps the weight-gradient products wide;
# on the device they are 16-bit, and in fp16 at scale 1024 they can saturate, so the step is skipped and the batch retried at the
# halved scale, as GradScaler does in training (fp16's relative precision does not depend on the scale above its subnormals).
EMU = {1: {"fp16": (3.9e-4, 3.6e-3, 2.2e-2, 0.014), "bf16": (4.3e-3, 1.3e-2, 8.8e-2, 0.013)},
       3: {"fp16": (4.7e-4, 6.7e-2, 2.3e-1, 0.037), "bf16": (2.2e-3, 9.1e-2, 3.6e-1, 0.095)},
       25: {"fp16": (1.6e-3, 4.3e-3, 7.0e-2, 0.008), "bf16": (3.9e-3, 1.2e-2, 1.0e-1, 0.024)}}
HEADROOM = 2.5
# The masked step (D 1024, B 4, I 15, k 25, fp16, loss scale 256) against the fp64 restatement: the emulation measured 1.0e-4 on the
# losses and 1.9e-2 on the worst parameter's whole gradient.
DROP_LOSS_TOL, DROP_GRAD_TOL = HEADROOM * 1.0e-4, HEADROOM * 1.9e-2


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return make_feature_cache(tmp_path_factory.mktemp("cache_rollout"), n_vars=2, seq_len=8)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _head(d, nb, seed, precision="fp16", lam=1.0):
    from implementation_phd_lab_vision_amd import train_ar
    from oracle import lifting_oracle as lo
    sd = lo.synthetic_head_state_dict(d, nb, seed)
    h = train_ar.ARTrainableHead(d, 17, nb, precision=precision, lambda_latent=lam)
    h.load_state_dict(sd)
    h.to(DEV)
    return h, sd


# ------------------------------------------------------------------ kernels ---------------------------------------------------
def _tm_bwd(lib, dr, x_tm, b, t, t0, c, gamma, beta, add, et):
    dt = x_tm.dtype
    dx = torch.full((t * b + 3, c), 7.0, dtype=dt, device=DEV)              # a guard band behind the output
    part = torch.empty((2, b, c), device=DEV)
    assert lib.r50_op_gn_relu_causal3_tm_bwd(dr.data_ptr(), x_tm.data_ptr(), b, t, t0, c, 32, gamma.data_ptr(), beta.data_ptr(), 1e-5,
                                             add.data_ptr() if add is not None else None, dx.data_ptr(), part[0].data_ptr(),
                                             part[1].data_ptr(), et, _stream()) == 0
    assert torch.all(dx[t * b:] == 7.0)
    return dx[: t * b], part


@pytest.mark.parametrize("et", [1, 0])
@pytest.mark.parametrize("t", [1, 2, 3, 17])
def test_tm_bwd_t0_zero_is_bit_equal_to_batch_major(lib, et, t):
    dt = torch.float16 if et else torch.bfloat16
    b, c = 3, 256
    g = torch.Generator().manual_seed(30 + t + 100 * et)
    x = (torch.randn(b, t, c, generator=g) * 2 + 0.3).to(dt).to(DEV)
    dr = torch.randn(b, t, 3 * c, generator=g).to(dt).to(DEV)
    add = torch.randn(b, t, c, generator=g).to(dt).to(DEV)
    gamma = (1 + 0.1 * torch.randn(c, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(c, generator=g)).to(DEV)
    for a in (None, add):
        ref = torch.empty((b, t, c), dtype=dt, device=DEV)
        ref_part = torch.empty((2, b, c), device=DEV)
        assert lib.r50_op_gn_relu_causal3_bwd(dr.data_ptr(), x.data_ptr(), b, t, c, 32, gamma.data_ptr(), beta.data_ptr(), 1e-5,
                                              a.data_ptr() if a is not None else None, ref.data_ptr(), ref_part[0].data_ptr(),
                                              ref_part[1].data_ptr(), et, _stream()) == 0
        tm = lambda v: v.transpose(0, 1).contiguous()                         # noqa: E731  (b, t, .) -> (t, b, .)
        dx, part = _tm_bwd(lib, tm(dr), tm(x), b, t, 0, c, gamma, beta, tm(a) if a is not None else None, et)
        assert torch.equal(dx.view(t, b, c).transpose(0, 1).view(torch.int16), ref.view(torch.int16))
        assert torch.equal(part, ref_part)


@pytest.mark.parametrize("et", [1, 0])
def test_tm_bwd_partial_emission_against_autograd(lib, et):
    """t0 = t-1 (the rollout's last block) and a middle t0: fp64 autograd of the forward's emitted rows."""
    import torch.nn.functional as F
    dt = torch.float16 if et else torch.bfloat16
    b, t, c = 4, 19, 256
    g = torch.Generator().manual_seed(40 + et)
    x = (torch.randn(t, b, c, generator=g) * 2 + 0.3).to(dt)
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    add = torch.randn(t, b, c, generator=g).to(dt)
    for t0 in (t - 1, 9, 1):
        dr = torch.randn((t - t0) * b, 3 * c, generator=g).to(dt)
        xd = x.double().permute(1, 2, 0).clone().requires_grad_(True)        # (b, c, t)
        y = F.relu(F.group_norm(xd, 32, gamma.double(), beta.double(), eps=1e-5))
        idx = torch.arange(t)
        rows = torch.cat([y[:, :, (idx - 2).clamp_min(0)], y[:, :, (idx - 1).clamp_min(0)], y], dim=1)   # (b, 3c, t)
        emitted = rows[:, :, t0:].permute(2, 0, 1).reshape((t - t0) * b, 3 * c)
        (emitted * dr.double()).sum().backward()
        want = xd.grad.permute(2, 0, 1).reshape(t * b, c) + add.double().view(t * b, c)
        dx, part = _tm_bwd(lib, dr.to(DEV), x.to(DEV).view(t * b, c), b, t, t0, c, gamma.to(DEV), beta.to(DEV),
                           add.to(DEV).view(t * b, c), et)
        # one rounding of the 16-bit output (half an ulp), and fp32 arithmetic against fp64 around it
        torch.testing.assert_close(dx.cpu().double(), want, rtol=2 ** -10 if et else 2 ** -7, atol=1e-4 * float(want.abs().max()))
        xh = F.group_norm(xd.detach(), 32, eps=1e-5)
        yy = xh * gamma.double().view(1, c, 1) + beta.double().view(1, c, 1)
        yv = yy.clone().requires_grad_(True)
        r = torch.cat([F.relu(yv)[:, :, (idx - 2).clamp_min(0)], F.relu(yv)[:, :, (idx - 1).clamp_min(0)], F.relu(yv)], dim=1)
        (r[:, :, t0:].permute(2, 0, 1).reshape((t - t0) * b, 3 * c) * dr.double()).sum().backward()
        pg = (yv.grad * xh).sum(-1)                                          # dgamma / dbeta parts: sums over t of dy * xh, dy
        torch.testing.assert_close(part[0].cpu().double(), pg, rtol=1e-4, atol=1e-4 * float(pg.abs().max()))
        torch.testing.assert_close(part[1].cpu().double(), yv.grad.sum(-1), rtol=1e-4, atol=1e-4 * float(yv.grad.sum(-1).abs().max()))


def test_rollout_loss_kernels(lib):
    from implementation_phd_lab_vision_amd import _lib
    g = torch.Generator().manual_seed(5)
    for b, k, t, i0, j in ((32, 25, 40, 15, 17), (3, 1, 2, 1, 17), (2, 3, 7, 4, 5)):
        pred, gt = torch.randn(k * b, j, 3, generator=g), torch.randn(b, t, j, 3, generator=g)
        pd, gd = pred.to(DEV), gt.to(DEV)
        runs = []
        for _ in range(2):
            dy = torch.full((k * b, j, 3), 7.0, device=DEV)
            loss2 = torch.empty(2, device=DEV)
            _lib.check(lib.r50_op_rollout_pose_loss_grad(pd.data_ptr(), gd.data_ptr(), b, k, t, i0, j, 64.0, dy.data_ptr(), loss2.data_ptr(),
                                                         _stream()), None, "rollout_pose_loss_grad")
            runs.append((dy.cpu(), loss2.cpu()))
        d = pred.double() - gt[:, i0:i0 + k].transpose(0, 1).reshape(k * b, j, 3).double()
        torch.testing.assert_close(runs[0][1].double(), torch.stack([d.pow(2).mean(), d.norm(dim=-1).mean()]), rtol=1e-6, atol=0)
        torch.testing.assert_close(runs[0][0].double(), 64.0 * 2 * d / d.numel(), rtol=1e-6, atol=0)
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for precision in ("fp16", "bf16"):
        dt, et = (torch.float16, 1) if precision == "fp16" else (torch.bfloat16, 0)
        for b, k, t, i0, d, lam, ls in ((32, 25, 40, 15, 1024, 0.5, 256.0), (3, 1, 2, 1, 64, 1.0, 1.0), (2, 3, 7, 4, 8, 0.0, 4.0)):
            fut, phi = torch.randn(k * b, d, generator=g).to(dt), torch.randn(b, t, d, generator=g).to(dt)
            base = torch.randn(k * b, d, generator=g)
            diff = fut.double() - phi[:, i0:i0 + k].transpose(0, 1).reshape(k * b, d).double()
            want = base.double() + lam * 2 * diff / diff.numel() * ls
            fd, pd_ = fut.to(DEV), phi.to(DEV)
            runs = []
            for _ in range(2):
                dfut = base.to(DEV)
                loss = torch.empty(1, device=DEV)
                part = torch.empty(k * b, device=DEV)
                _lib.check(lib.r50_op_rollout_latent_grad(fd.data_ptr(), pd_.data_ptr(), b, k, t, i0, d, lam, ls, dfut.data_ptr(),
                                                          loss.data_ptr(), part.data_ptr(), et, _stream()), None, "rollout_latent_grad")
                runs.append((dfut.cpu(), loss.cpu()))
            torch.testing.assert_close(runs[0][0].double(), want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
            assert float(runs[0][1]) == pytest.approx(float(diff.pow(2).mean()), rel=1e-6)
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------ the step -------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_training_forward_is_the_rollout(lib, precision):
    m, _ = _head(256, 2, 81, precision)
    m.eval()
    g = torch.Generator().manual_seed(810)
    for b, t, i_len, k in ((3, 40, 15, 25), (2, 2, 1, 1), (5, 9, 4, 3)):
        feats, gt = torch.randn(b, t, 2048, generator=g).abs().to(DEV), (torch.randn(b, t, 17, 3, generator=g) * 0.5).to(DEV)
        joints, losses = m.rollout_forward_backward(feats, gt, i_len, k, loss_scale=1024.0)
        assert joints.shape == (b, k, 17, 3)
        assert torch.equal(joints, m.rollout(feats, i_len, k)[1]), (b, t, i_len, k)
        d = joints.double() - gt[:, i_len:i_len + k].double()
        assert float(losses[0]) == pytest.approx(float(d.pow(2).mean()), rel=1e-5)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_train_steps_equal_reference_module(lib, precision):
    from implementation_phd_lab_vision_amd import train
    gold = torch.load(GOLDEN / "train_rollout_golden.pt", map_location="cpu", weights_only=True)
    for c in gold["cases"]:
        loss_t, gnorm_t, ghead_t, upd_t = (HEADROOM * v for v in EMU[c["k"]][precision])
        m, sd = _head(c["latent_dim"], c["number_blocks"], c["seed"], precision, c["lambda_latent"])
        m.eval()                                                   # the fixture's steps ran with dropout = identity
        optim = train.AdamW(m, lr=c["lr"], weight_decay=1e-2)
        scaler = train.GradScaler(init_scale=1024.0)
        for s, (feats, gt) in enumerate(batches_for(c["seed"], c["b"], c["t"])):
            for _ in range(12):                # a skipped step changes nothing: the batch is retried at the halved scale, as in training
                loss, _, skipped = m.rollout_train_step(feats.to(DEV), gt.to(DEV), c["input_len"], c["k"], optim, scaler)
                if not skipped:
                    break
            assert not skipped and scaler.get_scale() >= 16.0, (c["k"], s, scaler.get_scale())
            got = [loss, m.last_losses["l3d"], m.last_losses["l_lat"]]
            assert got == pytest.approx(c["losses"][s], rel=loss_t), (c["k"], s, got, c["losses"][s])
            if s == 0:
                grads = m.named_gradients()
                for i, n in enumerate(gold["trainable"]):
                    assert float(grads[n].norm()) == pytest.approx(c["grad_norm"][i], rel=gnorm_t), (c["k"], n)
                    if ghead_t / HEADROOM <= 0.2:
                        assert _rel(grads[n].reshape(-1)[:64], c["grad_head"][i]) < ghead_t, (c["k"], n)
        final = m.state_dict()
        for i, n in enumerate(gold["trainable"]):
            delta_want = c["param_head"][i] - sd[n].reshape(-1)[:64]
            delta_got = final[n].reshape(-1)[:64] - sd[n].reshape(-1)[:64]
            assert float((delta_got - delta_want).abs().median()) < max(upd_t, 0.02) * c["lr"], (c["k"], n)
            assert float(final[n].norm()) == pytest.approx(c["param_norm"][i], rel=1e-3), (c["k"], n)
        for n in sd:
            if not n.startswith("f_AR."):
                assert torch.equal(final[n], sd[n]), n
        assert optim.step_count == 2


def test_train_step_with_dropout_masks_against_restatement(lib):
    """train.py's configuration (D 1024, 2 blocks), B 4, I 15, k 25, the keep-masks shared with the fp64 restatement."""
    m, sd = _head(1024, 2, 91, lam=0.5)
    m.train()
    g = torch.Generator().manual_seed(911)
    feats = torch.randn(4, 40, 2048, generator=g).abs()
    gt = torch.randn(4, 40, 17, 3, generator=g) * 0.5
    masks = m.make_rollout_dropout_masks(4, 15, 25, torch.Generator(device=DEV).manual_seed(6))
    assert len(masks) == 25 and sorted(masks[0]) == [f"f_AR.blocks.{i}" for i in range(3)]
    assert [tuple(ms["f_AR.blocks.0"].shape) for ms in masks] == [((15 + j) * 4, 1024) for j in range(25)]
    assert 0.49 < float(masks[7]["f_AR.blocks.2"].float().mean()) < 0.51
    _, losses = m.rollout_forward_backward(feats.to(DEV), gt.to(DEV), 15, 25, loss_scale=256.0, masks=masks)
    want, grads, _ = train_rollout_steps_reference(sd, [(feats, gt)], 15, 25, [[{n: v.cpu() for n, v in ms.items()} for ms in masks]],
                                                   lambda_latent=0.5, dtype=torch.float64)
    l3d, mpjpe, l_lat = losses.tolist()
    assert [l3d, l_lat, mpjpe] == pytest.approx([want[0][1], want[0][2], want[0][3]], rel=DROP_LOSS_TOL)
    got = m.named_gradients()
    for n, gr in grads.items():
        assert _rel(got[n], gr) < DROP_GRAD_TOL, (n, _rel(got[n], gr))


def test_overflow_skips_the_step_and_halves_the_scale(lib):
    from implementation_phd_lab_vision_amd import train
    m, _ = _head(64, 2, 41)
    m.eval()
    optim, scaler = train.AdamW(m, lr=1e-4), train.GradScaler(init_scale=2.0 ** 40)       # far beyond fp16's range
    g = torch.Generator().manual_seed(410)
    feats, gt = torch.randn(2, 7, 2048, generator=g).abs().to(DEV), torch.randn(2, 7, 17, 3, generator=g).to(DEV)
    before = m.flat_master.clone()
    _, _, skipped = m.rollout_train_step(feats, gt, 4, 3, optim, scaler)
    assert skipped and scaler.get_scale() == 2.0 ** 39 and optim.step_count == 0
    assert torch.equal(m.flat_master, before)
    scaler = train.GradScaler(init_scale=256.0)
    _, _, skipped = m.rollout_train_step(feats, gt, 4, 3, optim, scaler)
    assert not skipped and optim.step_count == 1 and not torch.equal(m.flat_master, before)
    assert torch.equal(m.flat_w16, m.flat_master.half())


# ------------------------------------------------------------------ driver ----------------------------------------------------
def _run(argv, capsys):
    from implementation_phd_lab_vision_amd import train_ar
    train_ar.main(argv)
    return [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def test_driver_epoch_equals_hand_loop(lib, cache, tmp_path, capsys):
    from implementation_phd_lab_vision_amd import forecast, train, train_ar
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from implementation_phd_lab_vision_amd.samplers import MixedShardBatchSampler
    from oracle import lifting_oracle as lo
    sd = lo.synthetic_head_state_dict(256, 2, 61)
    torch.save({"epoch": 9, "best_val": 1.0, "model": sd, "optim": {}, "args": {}}, tmp_path / "phase1.pt")
    lines = _run(["--train", str(cache), "--val", str(cache), "--epochs", "1", "--batch-size", "8", "--seed", "7", "--outdir",
                  str(tmp_path / "run"), "--log-every", "0", "--lr", "2e-4", "--lambda-latent", "0.5", "--init", str(tmp_path / "phase1.pt"),
                  "--objective", "rollout", "--input-len", "3", "--pred-len", "4", "--curriculum-steps", "2"], capsys)
    assert len(lines) == 1 and lines[0]["k"] == 1
    assert set(lines[0]) == {"epoch", "lr", "k", "train_loss", "train_l3d", "train_l_lat", "train_mpjpe", "steps", "skipped", "val_mpjpe_1",
                             "val_mpjpe_10", "val_mpjpe_4", "val_mpjpe_mean"}
    store = DeviceFeatureStore(str(cache), subjects=[1, 6, 7, 8], augment=True, device=DEV)
    val = DeviceFeatureStore(str(cache), subjects=[5], device=DEV)
    sampler = MixedShardBatchSampler(store, batch_size=8, shuffle=True, drop_last=True, seed=0)
    head = train_ar.ARTrainableHead(256, 17, 2, lambda_latent=0.5)
    head.load_state_dict(sd)
    head.to(DEV)
    optim, scaler = train.AdamW(head, lr=2e-4), train.GradScaler()
    sampler.set_epoch(0)
    head.train()
    losses = []
    for it, idx in enumerate(sampler):
        feats, j3d = store.get_batch(idx)[:2]
        masks = head.make_rollout_dropout_masks(8, 3, 1, generator=train.dropout_generator(7, 0, it, head._device))
        losses.append(head.rollout_train_step(feats, j3d, 3, 1, optim, scaler, masks=masks)[0])
    assert sum(losses) / len(losses) == lines[0]["train_loss"] and lines[0]["steps"] == len(losses)
    v = forecast.evaluate_rollout(head, val, 3, 4, 8)
    assert [lines[0][k] for k in ("val_mpjpe_1", "val_mpjpe_4", "val_mpjpe_mean")] == [v["mpjpe"][0], v["mpjpe"][3], v["mpjpe_mean"]]
    ck = torch.load(tmp_path / "run" / "last.pt", weights_only=True)
    model = head.state_dict()
    for n in sd:
        assert torch.equal(ck["model"][n], model[n]), n
    assert ck["args"]["objective"] == "rollout" and ck["args"]["curriculum_steps"] == 2


def test_cli_curriculum_best_and_resume(lib, cache, tmp_path, capsys):
    from implementation_phd_lab_vision_amd import results, train_ar
    from oracle import lifting_oracle as lo
    torch.save(lo.synthetic_head_state_dict(256, 2, 71), tmp_path / "init.pt")
    out = tmp_path / "run"
    base = ["--train", str(cache), "--val", str(cache), "--batch-size", "8", "--outdir", str(out), "--log-every", "0", "--lr", "1e-3",
            "--objective", "rollout", "--input-len", "2", "--pred-len", "3", "--curriculum-steps", "3", "--early-stop-patience", "0"]
    lines = _run(base + ["--epochs", "3", "--init", str(tmp_path / "init.pt")], capsys)
    assert [e["k"] for e in lines] == [1, 2, 3] and [e["epoch"] for e in lines] == [0, 1, 2]
    best = torch.load(out / "best.pt", weights_only=True)
    means = [e["val_mpjpe_mean"] for e in lines]
    assert best["best_val"] == min(means) and best["epoch"] == means.index(min(means))
    # resume: the curriculum follows the epoch number
    lines2 = _run(base + ["--epochs", "5", "--resume", str(out / "last.pt")], capsys)
    assert [e["epoch"] for e in lines2] == [3, 4] and [e["k"] for e in lines2] == [3, 3]
    # the checkpoint loads in the results CLI's loader and rolls out 25 frames as the trained head does
    last = torch.load(out / "last.pt", weights_only=True)
    assert last["epoch"] == 4 and last["args"]["objective"] == "rollout"
    head = results.build_head(results.load_head_state(str(out / "last.pt")), DEV)
    trained = train_ar.ARTrainableHead(256, 17, 2)
    trained.load_state_dict(last["model"])
    trained.to(DEV)
    feats = torch.rand(2, 40, 2048, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(head.rollout(feats, 15, 25)[1], trained.rollout(feats, 15, 25)[1])
