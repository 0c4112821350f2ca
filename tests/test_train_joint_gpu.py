"""Joint training (input_proj, f_movie, f_AR and f_3D together; implementation_phd_lab_vision_amd/train_joint.py, INTEGRATION.md
section M) on the MI355X: ``r50_op_joint_pose_loss_grad`` against fp64 torch, two ``JointTrainableHead.train_step``s against the
reference module (tests/golden/train_joint_golden.pt), every dropout site against the CPU restatement (tests/joint_reference.py) with
shared masks, the reductions to phase 1 and phase 2 against their own pinned steps, the validation pass against ``train.evaluate``
and ``train_ar.evaluate_future``, overflow handling, checkpoints in torch.optim.AdamW's layout read by the results CLI, and the
driver (one epoch bit-equal to a hand loop, ``best.pt`` on mpjpe + mpjpe_hat, early stopping)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import results_data as rd
from tests.golden.make_golden_train_ar import batches_for
from tests.helpers import GOLDEN
from tests.joint_reference import train_joint_steps_reference
from tests.train_driver_data import make_feature_cache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]

# Tolerances of the fixture comparison, per precision and fixture case (tests/golden/make_golden_train_joint.py CASES: 0 = (64, 2,
# B 3, T 5), 1 = (128, 2, B 2, T 40), 2 = (256, 2, B 8, T 2) at lambda 0.5, 3 = (64, 2, B 3, T 5) at lambda 0).  They start from
# phase 2's (tests/test_train_ar_gpu.py): tol = GRAD_TOL {"fp16": 1.5e-2, "bf16": 1.5e-1}, doubled at T = 2; losses rel 3 tol,
# gradient norms rel tol, 64-entry gradient slices rel 2 tol; parameter updates with loose = (1 fp16, 3 bf16), doubled at T = 2:
# error median < 0.05 loose lr, relative error < 0.3 loose, error max < 2.5 loose lr.  Then tests/joint_reference.py with
# store16 (fp64, loss scale 1024, eval mode) was run against the fixture on the CPU, and wherever its distance for a quantity
# exceeded half of phase 2's tolerance, that quantity's tolerance became twice the measured distance (the device's roundings and
# the emulation's wide products are not the same model of the step).  Measured distances (max over the 48 parameters / 2 steps):
#
#   precision case | losses  grad norms  grad slices | err median/lr  delta rel  err max/lr
#   fp16      0    | 7.3e-4  5.6e-3      2.09e-2     | 0.052          0.250      2.73
#   fp16      1    | 3.2e-4  3.6e-3      6.67e-2     | 0.016          0.271      2.26
#   fp16      2    | 3.5e-3  7.0e-3      1.11e-1     | 0.075          0.455      3.78
#   fp16      3    | 1.1e-3  4.0e-3      3.48e-2     | 0.028          0.264      2.19
#   bf16      0    | 4.6e-3  9.39e-2     4.70e-1     | 0.140          0.677      3.76
#   bf16      1    | 6.6e-4  7.7e-3      1.66e-1     | 0.074          0.352      2.81
#   bf16      2    | 3.0e-3  1.7e-2      4.75e-1     | 0.137          0.698      3.77
#   bf16      3    | 2.8e-3  9.4e-3      1.17e-1     | 0.048          0.540      3.80
#
# f_movie's and the regressor's gradients now pass the f_AR backward and the stacked regressor too, so the slices and updates of
# the phase-1 parameters sit where phase 2 had only f_AR's.  Unlike phase 2, bf16 is held on the gradient slices as well.
_P2 = {"fp16": 1.5e-2, "bf16": 1.5e-1}


def _phase2_tols(precision, t):
    tol = _P2[precision] * (2 if t == 2 else 1)
    loose = (1.0 if precision == "fp16" else 3.0) * (2 if t == 2 else 1)
    return {"loss": 3 * tol, "grad_norm": tol, "grad_slice": 2 * tol, "p_med": 0.05 * loose, "p_rel": 0.3 * loose, "p_max": 2.5 * loose}


# the emulation's distances above, in the order of _phase2_tols' keys
_EMULATION = {
    "fp16": [(7.3e-4, 5.6e-3, 2.09e-2, 0.052, 0.250, 2.73), (3.2e-4, 3.6e-3, 6.67e-2, 0.016, 0.271, 2.26),
             (3.5e-3, 7.0e-3, 1.11e-1, 0.075, 0.455, 3.78), (1.1e-3, 4.0e-3, 3.48e-2, 0.028, 0.264, 2.19)],
    "bf16": [(4.6e-3, 9.39e-2, 4.70e-1, 0.140, 0.677, 3.76), (6.6e-4, 7.7e-3, 1.66e-1, 0.074, 0.352, 2.81),
             (3.0e-3, 1.7e-2, 4.75e-1, 0.137, 0.698, 3.77), (2.8e-3, 9.4e-3, 1.17e-1, 0.048, 0.540, 3.80)],
}
_T = (5, 40, 2, 5)


def tolerances(precision, case):
    base = _phase2_tols(precision, _T[case])
    return {k: (2 * m if m > base[k] / 2 else base[k]) for (k, m) in zip(base, _EMULATION[precision][case])}


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return make_feature_cache(tmp_path_factory.mktemp("cache_joint"), n_vars=4)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _sd(d, nb, seed):
    from oracle import lifting_oracle as lo
    return lo.synthetic_head_state_dict(d, nb, seed)


def _head(d, nb, seed, precision="fp16", cls=None, **kw):
    from implementation_phd_lab_vision_amd import train_joint
    sd = _sd(d, nb, seed)
    h = (cls or train_joint.JointTrainableHead)(d, 17, nb, precision=precision, **kw)
    h.load_state_dict(sd)
    h.to(DEV)
    return h, sd


# ------------------------------------------------------------------ the kernel --------------------------------------------------
def test_joint_pose_loss_grad_kernel(lib):
    from implementation_phd_lab_vision_amd import _lib
    g = torch.Generator().manual_seed(1)
    for b, t, j in ((1, 2, 17), (3, 5, 17), (32, 40, 17), (2, 3, 64)):
        y, gt = torch.randn(2, b, t, j, 3, generator=g), torch.randn(b, t, j, 3, generator=g)
        y_d, gt_d = y.to(DEV), gt.to(DEV)                      # held: a temporary's memory could be reused before the launch
        d1, d2 = (y[0] - gt).double(), (y[1] - gt).double()[:, 1:]
        for lf in (0.0, 0.5, 1.0):
            for ls in (1.0, 1024.0):
                runs = []
                for _ in range(2):
                    dy = torch.full((2, b, t, j, 3), 7.0, device=DEV)
                    out = torch.full((4,), 7.0, device=DEV)
                    _lib.check(lib.r50_op_joint_pose_loss_grad(y_d.data_ptr(), gt_d.data_ptr(), b, t, j, lf, ls, dy.data_ptr(),
                                                               out.data_ptr(), _stream()), None, "joint_pose_loss_grad")
                    runs.append((dy.cpu(), out.cpu()))
                dy, out = runs[0]
                want = torch.stack([d1.pow(2).mean(), torch.norm(d1, dim=-1).mean(), d2.pow(2).mean(), torch.norm(d2, dim=-1).mean()])
                torch.testing.assert_close(out.double(), want, rtol=1e-6, atol=0)
                torch.testing.assert_close(dy[0].double(), ls * 2 * d1 / d1.numel(), rtol=1e-6, atol=0)
                torch.testing.assert_close(dy[1][:, 1:].double(), ls * lf * 2 * d2 / d2.numel(), rtol=1e-6, atol=0)
                assert torch.equal(dy[1][:, 0], torch.zeros(b, j, 3)) and not dy[1][:, 0].signbit().any()
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
                # the arithmetic of the kernels it stands for: mse_loss_grad on the first half, future_pose_loss_grad on the second
                dy1 = torch.empty(b, t, j, 3, device=DEV)
                l1 = torch.empty(2, device=DEV)
                _lib.check(lib.r50_op_mse_loss_grad(y_d[0].data_ptr(), gt_d.data_ptr(), b * t * j * 3, ls, dy1.data_ptr(), l1.data_ptr(),
                                                    _stream()), None, "mse_loss_grad")
                assert torch.equal(dy[0], dy1.cpu())
                dy2 = torch.empty(b, t, j, 3, device=DEV)
                l2 = torch.empty(2, device=DEV)
                _lib.check(lib.r50_op_future_pose_loss_grad(y_d[1].data_ptr(), gt_d.data_ptr(), b, t, j, ls, dy2.data_ptr(), l2.data_ptr(),
                                                            _stream()), None, "future_pose_loss_grad")
                assert torch.equal(out[2:], l2.cpu())
                if lf == 1.0:
                    assert torch.equal(dy[1], dy2.cpu())
                if lf == 0.0:
                    assert not dy[1].any()


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_colsum_split_equals_colsum(lib, precision):
    """The joint step's bias-gradient column sums: ``r50_op_colsum``'s bits exactly, at the step's shapes (B 256 x T 40 stacked to
    20480 rows; 1024, 64 and latent-dim columns), tiny and ragged ones, with and without accumulation."""
    from implementation_phd_lab_vision_amd import _lib
    dt, et = (torch.float16, 1) if precision == "fp16" else (torch.bfloat16, 0)
    g = torch.Generator().manual_seed(3)
    for rows, cols, ld in ((20480, 1024, 1024), (20480, 64, 64), (10240, 1024, 1024), (320, 1088, 1088), (1, 64, 64), (15, 64, 64),
                           (17, 51, 64), (333, 100, 128), (241, 1, 8)):
        x = (torch.randn(rows, ld, generator=g) * 3).to(dt).to(DEV)
        init = torch.randn(cols, generator=g).to(DEV)
        part = torch.full((16 * cols,), 7.0, device=DEV)
        for scale in (1.0, 1.0 / 256):
            for acc in (0, 1):
                want, got = init.clone(), init.clone()
                _lib.check(lib.r50_op_colsum(x.data_ptr(), rows, cols, ld, scale, want.data_ptr(), acc, et, _stream()), None, "colsum")
                _lib.check(lib.r50_op_colsum_split(x.data_ptr(), rows, cols, ld, scale, part.data_ptr(), got.data_ptr(), acc, et, _stream()),
                           None, "colsum_split")
                assert torch.equal(got, want), (rows, cols, ld, scale, acc, float((got - want).abs().max()))
        torch.testing.assert_close(got.double(), init.double() + x[:, :cols].double().sum(0) / 256, rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------ the step against the reference module ------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_train_steps_equal_reference_module(lib, precision):
    from implementation_phd_lab_vision_amd import train
    gold = torch.load(GOLDEN / "train_joint_golden.pt", map_location="cpu", weights_only=True)
    names = gold["trainable"]
    for ci, c in enumerate(gold["cases"]):
        tol = tolerances(precision, ci)
        m, sd = _head(c["latent_dim"], c["number_blocks"], c["seed"], precision, lambda_future=c["lambda_future"],
                      lambda_latent=c["lambda_latent"])
        m.eval()                                                   # the fixture's steps ran with dropout = identity
        optim = train.AdamW(m, lr=c["lr"], weight_decay=1e-2)
        scaler = train.GradScaler(init_scale=1024.0)
        for s, (feats, gt) in enumerate(batches_for(c["seed"], c["b"], c["t"])):
            loss, mpjpe, skipped = m.train_step(feats.to(DEV), gt.to(DEV), optim, scaler)
            assert not skipped, (ci, s)
            want = c["losses"][s]
            got = [loss, m.last_losses["l3d"], m.last_losses["l3d_hat"], m.last_losses["l_lat"]]
            print(precision, ci, s, "losses", got, want)
            assert got == pytest.approx(want, rel=tol["loss"]), (ci, s, got, want)
            assert mpjpe == m.last_losses["mpjpe"]
            if s == 0:
                grads = m.named_gradients()
                assert list(grads) == names
                for i, k in enumerate(names):
                    n = gold["head_len"][i]
                    if c["grad_norm"][i] == 0.0:                    # f_AR at lambda = 0: zeros, as on the reference module
                        assert k.startswith("f_AR.") and not grads[k].any(), k
                        continue
                    assert float(grads[k].norm()) == pytest.approx(c["grad_norm"][i], rel=tol["grad_norm"]), (ci, k)
                    r = _rel(grads[k].reshape(-1)[:n], c["grad_head"][i][:n])
                    assert r < tol["grad_slice"], (ci, k, r)
        final = m.state_dict()
        for i, k in enumerate(names):
            n = gold["head_len"][i]
            delta_want = c["param_head"][i][:n] - sd[k].reshape(-1)[:n]
            delta_got = final[k].reshape(-1)[:n] - sd[k].reshape(-1)[:n]
            assert float(delta_want.abs().max()) > 0
            err = (delta_got - delta_want).abs()                   # as test_train_ar_gpu.py: bulk tight, whole slice loose
            assert float(err.median()) < tol["p_med"] * c["lr"], (ci, k, float(err.median()))
            assert _rel(delta_got, delta_want) < tol["p_rel"], (ci, k, _rel(delta_got, delta_want))
            assert float(err.max()) < tol["p_max"] * c["lr"], (ci, k, float(err.max()))
        assert torch.equal(final["f_3D.y0"], sd["f_3D.y0"])
        assert optim.step_count == 2


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_train_steps_with_dropout_masks_against_restatement(lib, precision):
    """Fixture case 1's geometry and tolerances ((128, 2, B 2, T 40), lambda 1, 1), in train mode: two steps with explicit masks of
    all four families, shared with the fp64 restatement."""
    from implementation_phd_lab_vision_amd import train
    ci, tol = 1, tolerances(precision, 1)
    m, sd = _head(128, 2, 12, precision)
    m.train()
    g = torch.Generator(device=DEV).manual_seed(6)
    masks = [m.make_dropout_masks(2, 40, g) for _ in range(2)]
    assert sorted(masks[0]) == sorted([f"f_movie.blocks.{i}" for i in range(2)] + [f"f_AR.blocks.{i}" for i in range(3)] +
                                      [f"f_3D.{i}" for i in range(3)] + [f"f_3D_hat.{i}" for i in range(3)])
    assert 0.49 < float(torch.cat([v.float().view(-1) for v in masks[0].values()]).mean()) < 0.51
    assert not torch.equal(masks[0]["f_3D.0"], masks[0]["f_3D_hat.0"])
    batches = batches_for(12, 2, 40)
    optim, scaler = train.AdamW(m, lr=1e-4), train.GradScaler(init_scale=1024.0)
    got_losses, grads = [], None
    for s, (feats, gt) in enumerate(batches):
        _, _, skipped = m.train_step(feats.to(DEV), gt.to(DEV), optim, scaler, masks=masks[s])
        assert not skipped
        got_losses.append([m.last_losses[k] for k in ("loss", "l3d", "mpjpe", "l3d_hat", "mpjpe_hat", "l_lat")])
        if s == 0:
            grads = m.named_gradients()
    want_losses, want_grads, want_final = train_joint_steps_reference(sd, batches, [{k: v.cpu() for k, v in ms.items()} for ms in masks],
                                                                      dtype=torch.float64)
    print(precision, "losses", got_losses, want_losses)
    for s in range(2):
        assert got_losses[s] == pytest.approx(want_losses[s], rel=tol["loss"]), s
    final = m.state_dict()
    for k, gw in want_grads.items():
        assert float(grads[k].norm()) == pytest.approx(float(gw.norm()), rel=tol["grad_norm"]), k
        assert _rel(grads[k].reshape(-1)[:64], gw.reshape(-1)[:64]) < tol["grad_slice"], k
        delta_want = (want_final[k] - sd[k].double()).reshape(-1)[:64]
        delta_got = (final[k] - sd[k]).reshape(-1)[:64]
        err = (delta_got - delta_want).abs()
        assert float(err.median()) < tol["p_med"] * 1e-4 and float(err.max()) < tol["p_max"] * 1e-4, k
        assert _rel(delta_got, delta_want) < tol["p_rel"], k


# ------------------------------------------------------------------ reductions to the pinned phases ----------------------------
def test_reduces_to_phase1(lib):
    """lambda_future = lambda_latent = 0 with phase 1's masks on f_movie and f_3D(phi): the 24 phase-1 gradients are
    ``TrainableHead.forward_backward``'s bit for bit and f_AR's are exactly 0.  At this shape (B*T = 160 stacked to 320 rows) the
    regressor's GEMMs pick the same tile for both row counts (the tile choice depends on the rows), so every product sums in the
    same K order; the stacked weight-gradient products only add exact-zero terms (the second half's gradient is 0)."""
    from implementation_phd_lab_vision_amd import train
    m, sd = _head(1024, 2, 21, lambda_future=0.0, lambda_latent=0.0)
    p1, _ = _head(1024, 2, 21, cls=train.TrainableHead)
    g = torch.Generator().manual_seed(211)
    feats = torch.randn(4, 40, 2048, generator=g).abs().to(DEV)
    gt = (torch.randn(4, 40, 17, 3, generator=g) * 0.5).to(DEV)
    masks = m.make_dropout_masks(4, 40, torch.Generator(device=DEV).manual_seed(7))
    pred1, loss1 = p1.forward_backward(feats, gt, loss_scale=256.0, masks={k: v for k, v in masks.items()
                                                                          if k.startswith("f_movie.") or k.startswith("f_3D.")})
    jp, jh, losses = m.forward_backward(feats, gt, loss_scale=256.0, masks=masks)
    assert torch.equal(jp, pred1)
    assert float(losses[1]) == pytest.approx(float(loss1[1]), rel=1e-6)      # mpjpe: fp64 sums here, fp32 in mse_loss_grad
    want, got = p1.named_gradients(), m.named_gradients()
    assert len(want) == 24
    for k, v in want.items():
        assert torch.equal(got[k], v), (k, float((got[k] - v).abs().max()))
    for k in got:
        if k.startswith("f_AR."):
            assert not got[k].any(), k
    assert not m._found.item() and not p1._found.item()


def test_reduces_to_phase2(lib):
    """Eval mode (no masks), lambda_future = 1: f_AR's gradients are ``ARTrainableHead.forward_backward``'s bit for bit on the same
    weights, lambda_latent and loss scale (the regressor's GEMMs pick the same tile for 160 and 320 rows, see above)."""
    from implementation_phd_lab_vision_amd import train_ar
    m, sd = _head(1024, 2, 22, lambda_future=1.0, lambda_latent=0.7)
    p2, _ = _head(1024, 2, 22, cls=train_ar.ARTrainableHead, lambda_latent=0.7)
    m.eval(); p2.eval()
    g = torch.Generator().manual_seed(221)
    feats = torch.randn(4, 40, 2048, generator=g).abs().to(DEV)
    gt = (torch.randn(4, 40, 17, 3, generator=g) * 0.5).to(DEV)
    jh2, losses2 = p2.forward_backward(feats, gt, loss_scale=512.0)
    jp, jh, losses = m.forward_backward(feats, gt, loss_scale=512.0)
    assert torch.equal(jh, jh2)
    assert torch.equal(losses[2:].cpu(), losses2.cpu())                      # [l3d_hat, mpjpe_hat, l_lat]: the same sums
    want, got = p2.named_gradients(), m.named_gradients()
    assert len(want) == 24
    for k, v in want.items():
        assert torch.equal(got[k], v), (k, float((got[k] - v).abs().max()))


# ------------------------------------------------------------------ evaluation, overflow, checkpoints -------------------------
def test_evaluate_joint_against_phase1_and_phase2_passes(lib, cache):
    from implementation_phd_lab_vision_amd import train, train_ar, train_joint
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    store = DeviceFeatureStore(str(cache), subjects=[5], device=DEV)
    m, sd = _head(128, 2, 31, lambda_future=0.5, lambda_latent=2.0)
    p2, _ = _head(128, 2, 31, cls=train_ar.ARTrainableHead)
    m.train()
    loss, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat = train_joint.evaluate_joint(m, store, 4)
    assert m.training
    want1 = train.evaluate(m, store, 4)                                        # (loss, mpjpe, l3d, 0)
    want2 = train_ar.evaluate_future(p2, store, 4)                             # (l3d_hat, mpjpe_hat, l_lat, mpjpe)
    print("evaluate_joint", (loss, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat), want1, want2)
    assert [l3d, mpjpe] == pytest.approx([want1[2], want1[1]], rel=1e-6)
    assert [l3d_hat, mpjpe_hat, l_lat] == pytest.approx(list(want2[:3]), rel=1e-6)
    assert mpjpe == pytest.approx(want2[3], rel=1e-6)
    assert loss == pytest.approx(l3d + 0.5 * l3d_hat + 2.0 * l_lat, rel=1e-12)
    assert train_joint.evaluate_joint(m, store, 4) == (loss, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat)


def test_overflow_skips_the_step_and_halves_the_scale(lib):
    from implementation_phd_lab_vision_amd import train
    m, _ = _head(64, 2, 41)
    m.eval()
    optim, scaler = train.AdamW(m, lr=1e-4), train.GradScaler(init_scale=2.0 ** 40)       # far beyond fp16's range
    g = torch.Generator().manual_seed(410)
    feats, gt = torch.randn(2, 5, 2048, generator=g).abs().to(DEV), torch.randn(2, 5, 17, 3, generator=g).to(DEV)
    before = m.flat_master.clone()
    _, _, skipped = m.train_step(feats, gt, optim, scaler)
    assert skipped and scaler.get_scale() == 2.0 ** 39 and optim.step_count == 0
    assert torch.equal(m.flat_master, before)
    scaler = train.GradScaler(init_scale=256.0)
    _, _, skipped = m.train_step(feats, gt, optim, scaler)
    assert not skipped and optim.step_count == 1 and not torch.equal(m.flat_master, before)
    assert torch.equal(m.flat_w16, m.flat_master.half())


def _results_cli(argv):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "implementation_phd_lab_vision_amd.results", *argv],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"results exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def test_checkpoints_load_in_torch_adamw_and_results_cli(lib, tmp_path):
    from implementation_phd_lab_vision_amd import results, train, train_joint
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    from oracle import lifting_oracle as lo
    m, sd = _head(128, 2, 51)
    optim, scaler = train.AdamW(m, lr=3e-4), train.GradScaler(init_scale=1024.0)
    g = torch.Generator(device=DEV).manual_seed(4)
    for _ in range(2):
        feats = torch.rand(2, 6, 2048, device=DEV, generator=g)
        gt = torch.randn(2, 6, 17, 3, device=DEV, generator=g) * 0.3
        assert not m.train_step(feats, gt, optim, scaler, masks=m.make_dropout_masks(2, 6, generator=g))[2]
    path = tmp_path / "best.pt"
    train.save_checkpoint(str(path), m, optim, 1, 0.5, {"note": "x"})
    ck = torch.load(path, map_location="cpu", weights_only=True)
    names = train_joint.joint_trainable_names(2)
    assert sorted(ck["model"]) == sorted(names + ["f_3D.y0"])
    PHDFor3DJoints(128, 17, 2).load_state_dict(ck["model"], strict=True)
    # project -> torch.optim.AdamW over the reference-layout parameters, in named_parameters() order -> project
    params = [torch.nn.Parameter(ck["model"][n].clone()) for n in names]
    opt = torch.optim.AdamW(params, lr=1.0, weight_decay=1e-2)
    opt.load_state_dict(ck["optim"])
    assert opt.param_groups[0]["lr"] == 3e-4 and len(opt.state) == 48
    for p, n in zip(params, names):
        assert opt.state[p]["exp_avg"].shape == ck["model"][n].shape, n
        p.grad = torch.full_like(p, 1e-3)
    opt.step()
    model_sd = dict(ck["model"])
    model_sd.update({n: p.detach().clone() for n, p in zip(names, params)})
    torch.save({"epoch": 2, "best_val": 0.4, "model": model_sd, "optim": opt.state_dict(), "args": {}}, tmp_path / "torch.pt")
    h2, _ = _head(128, 2, 0)
    o2 = train.AdamW(h2)
    train.load_checkpoint(str(tmp_path / "torch.pt"), h2, o2)
    assert o2.step_count == 3
    back, want = o2.state_dict(), opt.state_dict()
    for i, n in enumerate(names):
        assert torch.equal(h2.state_dict()[n], model_sd[n]), n
        for f in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][f], want["state"][i][f]), (n, f)
    assert torch.equal(h2.flat_w16, h2.flat_master.half())
    # the results loader takes the joint file unchanged; its future joints are the restatement's
    head = results.build_head(results.load_head_state(str(path)), DEV)
    feats = torch.rand(3, 7, 2048, generator=torch.Generator().manual_seed(5))
    got = head(feats.to(DEV), predict_future=True)[3]
    want_j = lo.forward_reference(ck["model"], feats, predict_future=True, dtype=torch.float64)[3]
    assert _rel(got.cpu(), want_j) < 4e-3                                     # test_head_gpu.py's fp16 forward bar
    assert torch.equal(got, m(feats.to(DEV), predict_future=True)[3])
    # the results CLI with --protocols and the longest rollout the cache's clips allow
    features, videos = rd.make_results_cache(tmp_path / "features"), rd.make_preprocessed_tree(tmp_path / "videos")
    p_len = rd.SEQ_LEN - 1
    out = _results_cli(["--features_root", str(features), "--preprocessed_root", str(videos), "--model_path", str(path), "--seq-len",
                        str(rd.SEQ_LEN), "--batch-size", "4", "--save-n", "3", "--video-size", "32", "--video-reader",
                        "tests.results_data:read_video", "--out", str(tmp_path / "res.npz"), "--input-len", "1", "--pred-len", str(p_len),
                        "--protocols"])
    assert any(l.startswith("Protocol metrics") for l in out.splitlines())
    assert any(l.startswith(f"Rollout protocol metrics | input 1 | pred {p_len}") for l in out.splitlines())
    assert (tmp_path / "res.npz").exists()


# ------------------------------------------------------------------ driver ----------------------------------------------------
def test_driver_epochs_equal_hand_loop_and_best_follows_the_sum(lib, cache, tmp_path, capsys):
    from implementation_phd_lab_vision_amd import results, train, train_joint
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from implementation_phd_lab_vision_amd.samplers import MixedShardBatchSampler
    sd = _sd(1024, 2, 61)
    torch.save({"epoch": 9, "best_val": 1.0, "model": sd, "optim": {}, "args": {}}, tmp_path / "phase2.pt")
    out = tmp_path / "run"
    train_joint.main(["--train", str(cache), "--val", str(cache), "--epochs", "2", "--batch-size", "8", "--seed", "7", "--outdir", str(out),
                      "--log-every", "0", "--lr", "2e-4", "--lambda-future", "0.5", "--lambda-latent", "0.25", "--init", str(tmp_path / "phase2.pt"),
                      "--early-stop-patience", "0"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [e["epoch"] for e in lines] == [0, 1]
    terms = ("loss", "l3d", "mpjpe", "l3d_hat", "mpjpe_hat", "l_lat")
    assert set(lines[0]) == {"epoch", "lr", "steps", "skipped", "val_mpjpe_sum"} | {f"{s}_{k}" for s in ("train", "val") for k in terms}
    last = torch.load(out / "last.pt", weights_only=True)
    best = torch.load(out / "best.pt", weights_only=True)
    sums = [e["val_mpjpe"] + e["val_mpjpe_hat"] for e in lines]
    assert [e["val_mpjpe_sum"] for e in lines] == sums
    assert last["epoch"] == 1 and best["best_val"] == min(sums) and best["epoch"] == sums.index(min(sums))
    assert (last["args"]["lambda_future"], last["args"]["lambda_latent"]) == (0.5, 0.25)
    for name in ("last.pt", "best.pt"):                                      # the results loader takes both unchanged
        assert results.infer_head_dims(results.load_head_state(str(out / name))) == (1024, 17, 2)

    store = DeviceFeatureStore(str(cache), subjects=[1, 6, 7, 8], augment=True, device=DEV)
    val = DeviceFeatureStore(str(cache), subjects=[5], device=DEV)
    sampler = MixedShardBatchSampler(store, batch_size=8, shuffle=True, drop_last=True, seed=0)
    head = train_joint.JointTrainableHead(1024, 17, 2, lambda_future=0.5, lambda_latent=0.25)
    head.load_state_dict(sd)
    head.to(DEV)
    optim, scaler, sched = train.AdamW(head, lr=2e-4), train.GradScaler(), train.CosineLR(2e-4, 2)
    for epoch in range(2):
        sampler.set_epoch(epoch)
        optim.lr = sched.lr
        head.train()
        rows = []
        for it, idx in enumerate(sampler):
            feats, j3d = store.get_batch(idx)[:2]
            masks = head.make_dropout_masks(8, feats.shape[1], generator=train.dropout_generator(7, epoch, it, head._device))
            head.train_step(feats, j3d, optim, scaler, masks=masks)
            rows.append([head.last_losses[k] for k in terms])
        for j, k in enumerate(terms):
            assert sum(r[j] for r in rows) / len(rows) == lines[epoch][f"train_{k}"], (epoch, k)
        v = train_joint.evaluate_joint(head, val, 8)
        assert [lines[epoch][f"val_{k}"] for k in terms] == list(v)
        sched.step()
        optim.lr = sched.lr
        ck = best if best["epoch"] == epoch else (last if epoch == 1 else None)
        if ck is not None:
            model, mine = head.state_dict(), optim.state_dict()
            for k in sd:
                assert torch.equal(ck["model"][k], model[k]), k
            assert mine["param_groups"][0]["lr"] == ck["optim"]["param_groups"][0]["lr"]
            for i in range(48):
                for f in ("step", "exp_avg", "exp_avg_sq"):
                    assert torch.equal(mine["state"][i][f], ck["optim"]["state"][i][f]), (i, f)


def test_cli_early_stopping_with_zero_lr(lib, cache, tmp_path):
    from oracle import lifting_oracle as lo
    torch.save(lo.synthetic_head_state_dict(64, 2, 71), tmp_path / "init.pt")          # a plain state dict
    out = tmp_path / "run"
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "implementation_phd_lab_vision_amd.train_joint", "--train",
                        str(cache), "--val", str(cache), "--epochs", "6", "--batch-size", "8", "--lr", "0", "--early-stop-patience", "1",
                        "--outdir", str(out), "--log-every", "0", "--init", str(tmp_path / "init.pt")],
                       cwd=str(ROOT), env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"driver exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    epochs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [e["epoch"] for e in epochs] == [0, 1]
    for k in ("val_mpjpe", "val_mpjpe_hat", "val_l3d", "val_l3d_hat", "val_l_lat", "val_loss"):
        assert epochs[0][k] == epochs[1][k], k
    assert "Early stopping triggered at epoch 2" in r.stdout and "latent 64" in r.stdout
    best, last = torch.load(out / "best.pt", weights_only=True), torch.load(out / "last.pt", weights_only=True)
    assert best["epoch"] == 0 and last["epoch"] == 1 and best["best_val"] == epochs[0]["val_mpjpe"] + epochs[0]["val_mpjpe_hat"]
    for k, v in best["model"].items():
        assert torch.equal(v, last["model"][k]), k
