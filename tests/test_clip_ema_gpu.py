"""Global-norm gradient clipping and EMA weights on the device: ``r50_op_grad_norm`` against numpy's fp64
sum, ``r50_op_adamw_clip_ema`` bit for bit against ``r50_op_adamw`` and fp32 torch ops, two steps of every step kind against the
composition of existing pieces and against tests/clip_ema_reference.py, the launches of ``_finish_step`` with the features off and
on, the skipped step, ``swapped_weights`` and the driver.  PHD(64, 17, 1) heads at B 2, T 4 (rollout: I 2, k 2), fp16, the sizes of
tests/test_trainable_gpu.py, unless stated."""
import json
import shutil

import numpy as np
import pytest
import torch

from tests.clip_ema_reference import ClipAdamWEMA
from tests.train_driver_data import make_feature_cache
from tests.kernel_cases import _lerp_fp32, _ulps  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS, B, T, INPUT_LEN, K_STEPS = (64, 17, 1), 2, 4, 2, 2
STEP_KINDS = ("phase1", "phase2_teacher", "phase2_rollout", "joint")
RTOL, ATOL = 1e-5, 1e-6            # the bar of test_adamw_kernel_equals_torch_adamw
POISON = -7.25

# r50_op_grad_norm's schedule (include/r50.h), restated: W = min(ceil(n / 4096), 2048) workgroups, each a slice of ceil(n / W)
# elements rounded up to a multiple of 4, read in rounds of 1024 elements
GRANULE, ROUND, MAX_WG = 4096, 1024, 2048


def schedule(n):
    w = min(-(-n // GRANULE), MAX_WG)
    return w, -(-(-(-n // w)) // 4) * 4


def every_workgroup_ragged_multi_round(n):
    w, sl = schedule(n)
    lens = [min(sl, n - i * sl) for i in range(w)]
    return all(ln > ROUND and ln % ROUND != 0 for ln in lens)


SMALLEST_RAGGED = next(n for n in range(1, 3 * GRANULE) if every_workgroup_ragged_multi_round(n))
TWO_WG_RAGGED = next(n for n in range(GRANULE + 1, 3 * GRANULE) if every_workgroup_ragged_multi_round(n))
NORM_SIZES = (64, 192, GRANULE + 64, SMALLEST_RAGGED, TWO_WG_RAGGED)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def test_schedule_restatement():
    assert SMALLEST_RAGGED == ROUND + 1 and schedule(SMALLEST_RAGGED) == (1, ROUND + 4)
    assert TWO_WG_RAGGED == GRANULE + 1 and schedule(TWO_WG_RAGGED) == (2, 2052)
    assert schedule(GRANULE + 64) == (2, 2080) and schedule(64) == (1, 64) and schedule(10 ** 8)[0] == MAX_WG


# ------------------------------------------------------------------ the norm op ------------------------------------------------
class NormBuffers:
    def __init__(self, n, guard=8):
        self.w = schedule(n)[0]
        self.part = torch.full((self.w + guard,), POISON, dtype=torch.float64, device=DEV)
        self.found = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.clip2 = torch.full((2,), POISON, dtype=torch.float32, device=DEV)
        self.stats4 = torch.zeros(4, dtype=torch.float64, device=DEV)

    def run(self, lib, g, max_norm, n_part=None):
        from implementation_phd_lab_vision_amd import _lib
        _lib.check(lib.r50_op_grad_norm(g.data_ptr(), g.numel(), max_norm, self.part.data_ptr(), self.w if n_part is None else n_part,
                                        self.found.data_ptr(), self.clip2.data_ptr(), self.stats4.data_ptr(), _stream()), None, "r50_op_grad_norm")
        torch.cuda.synchronize()
        assert torch.all(self.part[self.w:] == POISON), "the guard behind part was written"
        return self.clip2.cpu().numpy().copy()


@pytest.mark.parametrize("n", NORM_SIZES)
@pytest.mark.parametrize("scale", (1.0, 1e18, 1e-30))
def test_grad_norm_equals_fp64_sum(lib, n, scale):
    """norm within 1 fp32 ulp of float32(sqrt(fp64 sum)), coef within 1 ulp of the fp64 rule: the products are exact in fp64 and both
    sums are fp64 trees over at most ~1e4 terms (relative error ~1e-15), so only the final rounding to fp32 can differ, by one ulp at a
    rounding boundary.  At 1e18 the squares overflow fp32: an fp32 accumulator fails here."""
    x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * scale).to(torch.float32)
    assert torch.isfinite(x).all()
    x64 = x.numpy().astype(np.float64)
    norm64 = np.sqrt(np.sum(x64 * x64))
    max_norm = 1.0
    coef64 = min(1.0, max_norm / (norm64 + 1e-6))
    g = x.to(DEV)
    bufs = NormBuffers(n)
    first = bufs.run(lib, g, max_norm)
    part_first = bufs.part.clone()
    print(f"n {n} scale {scale}: norm {first[1]!r} (fp64 {norm64!r}, {_ulps(first[1], np.float32(norm64)):.2f} ulp), "
          f"coef {first[0]!r} (fp64 {coef64!r}, {_ulps(first[0], np.float32(coef64)):.2f} ulp)")
    assert _ulps(first[1], np.float32(norm64)) <= 1.0
    assert _ulps(first[0], np.float32(coef64)) <= 1.0
    assert int(bufs.found.item()) == 0
    np.testing.assert_allclose(bufs.part[:bufs.w].sum().item(), norm64 * norm64, rtol=1e-13)
    st = bufs.stats4.tolist()
    assert st[0] == 1.0 and st[1] == float(coef64 < 1.0) and st[2] == st[3] and _ulps(st[2], np.float32(norm64)) <= 1.0
    second = bufs.run(lib, g, max_norm)                          # the same bits on every run
    assert first.tobytes() == second.tobytes() and torch.equal(bufs.part, part_first)
    assert bufs.stats4[0].item() == 2.0 and bufs.stats4[3].item() == st[3] and bufs.stats4[2].item() == 2 * st[2]
    assert bufs.stats4[1].item() == 2.0 * float(coef64 < 1.0)
    off = bufs.run(lib, g, 0.0)                                  # max_norm <= 0: norm and flag only
    assert off[0] == 1.0 and off.tobytes()[4:] == first.tobytes()[4:]
    assert torch.equal(g.cpu(), x)                               # the gradient is read, never written


def test_grad_norm_flag_and_stats(lib):
    n = GRANULE + 64
    x = torch.randn(n, generator=torch.Generator().manual_seed(3))
    for idx, bad in ((0, float("inf")), (n - 1, float("-inf")), (n // 2 + 1, float("inf")), (1027, float("nan"))):
        g = x.clone()
        g[idx] = bad
        bufs = NormBuffers(n)
        bufs.run(lib, g.to(DEV), 1.0)
        assert int(bufs.found.item()) == 1, (idx, bad)
        assert torch.equal(bufs.stats4.cpu(), torch.zeros(4, dtype=torch.float64)), (idx, bad)     # a found step is not counted
        assert bufs.clip2[0].item() == 1.0 and not np.isfinite(bufs.clip2[1].item())
    bufs = NormBuffers(n)
    bufs.run(lib, x.to(DEV), 1.0)
    assert int(bufs.found.item()) == 0 and bufs.stats4[0].item() == 1.0                            # finite data leaves the flag down
    bufs.found.fill_(1)                                                                              # e.g. the arena's overflow check
    before = bufs.stats4.clone()
    bufs.run(lib, x.to(DEV), 1.0)
    assert int(bufs.found.item()) == 1 and torch.equal(bufs.stats4, before)                        # a raised flag stays; stats stand still


def test_grad_norm_refusals(lib):
    n = GRANULE + 64
    g = torch.ones(n + 4, device=DEV)
    b = NormBuffers(n)
    args = [g.data_ptr(), n, 1.0, b.part.data_ptr(), b.w, b.found.data_ptr(), b.clip2.data_ptr(), b.stats4.data_ptr(), _stream()]
    for i in (0, 3, 5, 6, 7):
        bad = list(args)
        bad[i] = None
        assert lib.r50_op_grad_norm(*bad) == -1 and b"null" in lib.r50_last_error(None), i
    for i, v, word in ((1, 0, b"n"), (4, b.w - 1, b"part"), (0, g.data_ptr() + 4, b"aligned")):
        bad = list(args)
        bad[i] = v
        assert lib.r50_op_grad_norm(*bad) == -1 and word in lib.r50_last_error(None), (i, lib.r50_last_error(None))
    torch.cuda.synchronize()
    assert torch.all(b.part == POISON) and torch.all(b.clip2 == POISON)                            # nothing was launched


# ------------------------------------------------------------------ the update op ----------------------------------------------
GUARD = 64
HYPER = (1e-3, 0.9, 0.999, 1e-8, 1e-2)


class UpdateBuffers:
    """p, m, v, p16 and ema of ``n`` elements, each followed by a poisoned guard; g likewise (read only)."""

    def __init__(self, n, dtype, seed):
        gen = torch.Generator().manual_seed(seed)
        self.n = n

        def guarded(t, dt=torch.float32):
            out = torch.full((n + GUARD,), POISON, dtype=dt, device=DEV)
            out[:n] = t.to(DEV).to(dt)
            return out
        p0 = torch.randn(n, generator=gen)
        self.p, self.m, self.v = guarded(p0), guarded(torch.zeros(n)), guarded(torch.zeros(n))
        self.p16 = guarded(p0, dtype)
        self.ema = guarded(p0 + 0.1 * torch.randn(n, generator=gen))
        self.grads = [guarded(torch.randn(n, generator=gen)) for _ in range(2)]

    def clone(self):
        other = object.__new__(UpdateBuffers)
        other.n = self.n
        for k in ("p", "m", "v", "p16", "ema"):
            setattr(other, k, getattr(self, k).clone())
        other.grads = self.grads
        return other

    def tensors(self):
        return {k: getattr(self, k) for k in ("p", "m", "v", "p16", "ema")}

    def assert_guards(self):
        for k, t in self.tensors().items():
            assert torch.all(t[self.n:] == POISON), f"the guard behind {k} was written"


def _adamw(lib, b, g, step, found, et):
    from implementation_phd_lab_vision_amd import _lib
    _lib.check(lib.r50_op_adamw(b.p.data_ptr(), b.m.data_ptr(), b.v.data_ptr(), g.data_ptr(), b.p16.data_ptr(), b.n, *HYPER, step,
                                found.data_ptr(), et, _stream()), None, "r50_op_adamw")


def _adamw_clip_ema(lib, b, g, step, found, et, clip=None, ema=False, w=0.0):
    from implementation_phd_lab_vision_amd import _lib
    _lib.check(lib.r50_op_adamw_clip_ema(b.p.data_ptr(), b.m.data_ptr(), b.v.data_ptr(), g.data_ptr(), b.p16.data_ptr(), b.n, *HYPER, step,
                                         found.data_ptr(), clip.data_ptr() if clip is not None else None,
                                         b.ema.data_ptr() if ema else None, w, et, _stream()), None, "r50_op_adamw_clip_ema")


@pytest.mark.parametrize("n", (64, 320, 256 * 8192 + 192))                 # the last: a second grid-stride round
@pytest.mark.parametrize("precision", ("fp16", "bf16"))
def test_adamw_clip_ema_bits(lib, n, precision):
    dtype, et = (torch.float16, 1) if precision == "fp16" else (torch.bfloat16, 0)
    base = UpdateBuffers(n, dtype, seed=n)
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    clip = torch.tensor([0.37, 123.0], dtype=torch.float32, device=DEV)
    w = 0.1
    want, plain, clipped, averaged = base.clone(), base.clone(), base.clone(), base.clone()
    want_clipped = base.clone()
    for step, g in enumerate(base.grads, 1):
        g_before = g.clone()
        _adamw(lib, want, g, step, found, et)
        _adamw_clip_ema(lib, plain, g, step, found, et)                                             # (a)
        _adamw(lib, want_clipped, g * clip[0], step, found, et)                                     # the product in fp32 on the device
        _adamw_clip_ema(lib, clipped, g, step, found, et, clip=clip)                                # (b)
        e_before = averaged.ema[:n].clone()
        _adamw_clip_ema(lib, averaged, g, step, found, et, ema=True, w=w)                           # (c)
        torch.cuda.synchronize()
        assert torch.equal(g, g_before)                                                             # the gradient is not written back
        for k in ("p", "m", "v", "p16"):
            assert torch.equal(getattr(plain, k), getattr(want, k)), (step, k)
            assert torch.equal(getattr(clipped, k), getattr(want_clipped, k)), (step, k)
            assert torch.equal(getattr(averaged, k), getattr(want, k)), (step, k)
        assert torch.equal(plain.ema, base.ema) and torch.equal(clipped.ema, base.ema)
        assert torch.equal(averaged.ema[:n], _lerp_fp32(e_before, averaged.p[:n], w)), step
        assert not torch.equal(clipped.p, want.p) and not torch.equal(averaged.ema[:n], e_before)
    for b in (plain, clipped, averaged):
        b.assert_guards()
    found.fill_(1)                                                                                  # (d)
    frozen = averaged.clone()
    _adamw_clip_ema(lib, averaged, base.grads[0], 3, found, et, clip=clip, ema=True, w=w)
    torch.cuda.synchronize()
    for k, t in averaged.tensors().items():
        assert torch.equal(t, getattr(frozen, k)), k


# ------------------------------------------------------------------ steps ------------------------------------------------------
def head_class(kind):
    from implementation_phd_lab_vision_amd import train, train_ar, train_joint
    return {"phase1": train.TrainableHead, "phase2": train_ar.ARTrainableHead, "joint": train_joint.JointTrainableHead}[kind]


def make_head(kind, dims=DIMS):
    from oracle import lifting_oracle as lo
    d, j, nb = dims
    h = head_class(kind)(d, j, nb, precision="fp16")
    h.load_state_dict(lo.synthetic_head_state_dict(d, nb, 3))
    return h.to(DEV).train(False)                                            # dropout off: a step is a function of its inputs


def batches(count=2):
    g = torch.Generator().manual_seed(11)
    out = []
    for _ in range(count):
        feats = torch.randn(B, T, 2048, generator=g).abs()
        gt = torch.randn(B, T, 17, 3, generator=g) * 0.3
        out.append((feats.to(DEV), gt.to(DEV)))
    return out


def forward_backward(head, step_kind, feats, gt, scale):
    if step_kind == "phase2_rollout":
        head.rollout_forward_backward(feats, gt, INPUT_LEN, K_STEPS, scale)
    else:
        head.forward_backward(feats, gt, scale)


def train_step(head, step_kind, feats, gt, optim, scaler):
    if step_kind == "phase2_rollout":
        return head.rollout_train_step(feats, gt, INPUT_LEN, K_STEPS, optim, scaler)[2]
    return head.train_step(feats, gt, optim, scaler)[2]


SCALE = 1024.0


def first_step_norm(step_kind):
    head = make_head(step_kind.split("_")[0])
    forward_backward(head, step_kind, *batches(1)[0], SCALE)
    return float(head.flat_grad.double().norm())


@pytest.mark.parametrize("step_kind", STEP_KINDS)
def test_two_steps_equal_the_composition_and_the_reference(lib, step_kind):
    from implementation_phd_lab_vision_amd import _lib, train
    from implementation_phd_lab_vision_amd.trainable import WeightEMA
    max_norm = 0.5 * first_step_norm(step_kind)
    assert max_norm > 0
    head = make_head(step_kind.split("_")[0])
    optim, scaler = train.AdamW(head, lr=1e-3), train.GradScaler(init_scale=SCALE)
    optim.max_grad_norm, optim.ema = max_norm, WeightEMA(head, 0.9)
    n = head.flat_master.numel()
    # the composition of existing pieces, on clones
    p, m, v = head.flat_master.clone(), optim.exp_avg.clone(), optim.exp_avg_sq.clone()
    p16, e = head.flat_w16.clone(), optim.ema.flat.clone()
    found0 = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref = ClipAdamWEMA([head.flat_master.cpu()], 1e-3, max_norm=max_norm)
    coefs = []
    for step, (feats, gt) in enumerate(batches(2), 1):
        w = optim.ema.weight()
        assert not train_step(head, step_kind, feats, gt, optim, scaler)
        g = head.flat_grad.clone()                                               # the UNCLIPPED gradient
        coef, norm = head._clip2.tolist()
        coefs.append(coef)
        assert norm == pytest.approx(float(g.double().norm()), rel=1e-6)
        g_clipped = g * head._clip2[0]                                           # one fp32 product per element, as the op forms it
        _lib.check(lib.r50_op_adamw(p.data_ptr(), m.data_ptr(), v.data_ptr(), g_clipped.data_ptr(), p16.data_ptr(), n, optim.lr,
                                    0.9, 0.999, optim.eps, optim.weight_decay, step, found0.data_ptr(), 1, _stream()), None, "r50_op_adamw")
        e = _lerp_fp32(e, p, w)
        torch.cuda.synchronize()
        assert torch.equal(head.flat_master, p) and torch.equal(head.flat_w16, p16), step
        assert torch.equal(optim.exp_avg, m) and torch.equal(optim.exp_avg_sq, v), step
        assert torch.equal(optim.ema.flat, e), step
        ref.step([g.cpu()], w=w)
        assert ref.coefs[-1] == pytest.approx(coef, rel=1e-6)
        torch.testing.assert_close(head.flat_master.cpu().double(), ref.p[0], rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(optim.ema.flat.cpu().double(), ref.ema[0], rtol=RTOL, atol=ATOL)
        assert optim.ema.updates == step == optim.step_count
    assert coefs[0] < 1.0, coefs                                                 # step 1 was clipped: max_norm is half its norm
    st = head.clip_stats()
    assert st["steps"] == 2 and st["clipped_frac"] == sum(c < 1.0 for c in coefs) / 2 and st["grad_norm_max"] >= st["grad_norm_mean"] > 0
    assert head.clip_stats()["steps"] == 0                                       # reset


# ------------------------------------------------------------------ the off path, the skip, the swap -----------------------------
def record_finish(head, optim, scaler, monkeypatch):
    from implementation_phd_lab_vision_amd import _lib
    calls = []
    real = _lib.check

    def check(rc, handle=None, what=""):
        calls.append(what)
        return real(rc, handle, what)

    forward_backward(head, "phase1", *batches(1)[0], scaler.get_scale())
    monkeypatch.setattr(_lib, "check", check)
    try:
        assert not head._finish_step(optim, scaler, None)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_lib, "check", real)
    return calls


def test_launches_of_the_step_tail(lib, monkeypatch):
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.trainable import WeightEMA
    new = {"r50_op_grad_norm", "r50_op_adamw_clip_ema"}
    head = make_head("phase1")
    optim, scaler = train.AdamW(head, lr=1e-3), train.GradScaler(init_scale=SCALE)
    assert optim.max_grad_norm is None and optim.ema is None
    off = record_finish(head, optim, scaler, monkeypatch)
    assert not new & set(off), off
    assert off[:2] == ["r50_op_check_finite", "r50_op_adamw"] and set(off[2:]) == {"r50_op_transpose16"}, off
    optim.max_grad_norm = 1.0
    clip = record_finish(head, optim, scaler, monkeypatch)
    assert clip[:2] == ["r50_op_grad_norm", "r50_op_adamw_clip_ema"] and clip[2:] == off[2:], clip
    assert "r50_op_check_finite" not in clip and "r50_op_adamw" not in clip
    optim.max_grad_norm, optim.ema = None, WeightEMA(head, 0.9)
    ema = record_finish(head, optim, scaler, monkeypatch)
    assert ema[:2] == ["r50_op_check_finite", "r50_op_adamw_clip_ema"] and ema[2:] == off[2:], ema


@pytest.mark.parametrize("step_kind", ("phase1", "phase2_rollout"))
def test_overflow_skips_ema_and_stats(lib, step_kind):
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.trainable import WeightEMA
    head = make_head(step_kind.split("_")[0])
    optim, scaler = train.AdamW(head, lr=1e-4), train.GradScaler(init_scale=2.0 ** 40)           # far beyond fp16's range
    optim.max_grad_norm, optim.ema = 1.0, WeightEMA(head, 0.9)
    optim.ema.flat.add_(0.125)                                                                     # not the master's bits
    before_p, before_e = head.flat_master.clone(), optim.ema.flat.clone()
    feats, gt = batches(1)[0]
    assert train_step(head, step_kind, feats, gt * 1000.0, optim, scaler)
    assert scaler.get_scale() == 2.0 ** 39 and optim.step_count == 0 and optim.ema.updates == 0
    assert torch.equal(head.flat_master, before_p) and torch.equal(optim.ema.flat, before_e)
    assert head._stats4[0].item() == 0.0 and head.clip_stats()["steps"] == 0


def test_swapped_weights(lib):
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    from implementation_phd_lab_vision_amd.trainable import WeightEMA
    head = make_head("phase1")
    optim, scaler = train.AdamW(head, lr=1e-3), train.GradScaler(init_scale=SCALE)      # the steps test's rate: no step overflows
    optim.ema = WeightEMA(head, 0.9)
    for feats, gt in batches(2):
        assert not head.train_step(feats, gt, optim, scaler)[2]
    assert not torch.equal(optim.ema.flat, head.flat_master)
    feats = batches(1)[0][0]
    ema_sd = optim.ema.state_dict()
    assert set(ema_sd) == {"decay", "warmup", "updates", "model"} and ema_sd["updates"] == 2 and sorted(ema_sd["model"]) == sorted(head.state_dict())
    plain = PHDFor3DJoints(*DIMS, precision="fp16")
    plain.load_state_dict(ema_sd["model"], strict=True)
    want = plain.to(DEV).eval().joints(feats)
    raw_joints = head.joints(feats).clone()
    before = {"master": head.flat_master.clone(), "w16": head.flat_w16.clone(), "ema": optim.ema.flat.clone(),
              **{f"wt.{k}": v.clone() for k, v in head._wt.items()}}
    with head.swapped_weights(optim.ema.flat):
        assert torch.equal(head.flat_master, before["ema"]) and torch.equal(optim.ema.flat, before["master"])
        got = head.joints(feats).clone()
    assert torch.equal(got, want) and not torch.equal(got, raw_joints)
    assert torch.equal(head.flat_master, before["master"]) and torch.equal(head.flat_w16, before["w16"])
    assert torch.equal(optim.ema.flat, before["ema"])
    for k, v in head._wt.items():
        assert torch.equal(v, before[f"wt.{k}"]), k
    assert torch.equal(head.joints(feats), raw_joints)
    # the round trip of the EMA's state
    other = WeightEMA(head, 0.5, warmup=False)
    other.load_state_dict(ema_sd)
    assert (other.decay, other.warmup, other.updates) == (0.9, True, 2) and torch.equal(other.flat, optim.ema.flat)
    with pytest.raises(ValueError):
        with head.swapped_weights(optim.ema.flat[:-64]):
            pass


# ------------------------------------------------------------------ the driver -------------------------------------------------
@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return make_feature_cache(tmp_path_factory.mktemp("cache4"), n_vars=4)


def _run(argv, capsys):
    from implementation_phd_lab_vision_amd import train
    capsys.readouterr()
    train.main(argv)
    return [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def test_driver_clip_ema_resume_and_checkpoints(lib, cache, tmp_path, capsys, monkeypatch):
    from implementation_phd_lab_vision_amd import results, train
    common = ["--train", str(cache), "--val", str(cache), "--batch-size", "8", "--seed", "7", "--log-every", "0", "--lr", "2e-4"]
    flags = ["--clip-grad-norm", "50", "--ema-decay", "0.9"]
    real_save = train.save_checkpoint

    def save_and_keep_each_epoch(path, head, optim, epoch, best_val, args):
        real_save(path, head, optim, epoch, best_val, args)
        if path.endswith("last.pt"):
            shutil.copy(path, path[:-len("last.pt")] + f"epoch{epoch}.pt")

    monkeypatch.setattr(train, "save_checkpoint", save_and_keep_each_epoch)
    # Checkpoints do not hold the GradScaler (as the reference's do not), so a resumed run equals the uninterrupted one only if no step
    # overflowed before the cut.  The cache's joints are in mm: at the default scale of 65536 the first steps overflow and back the
    # scale off.  Every run here starts at a scale no step overflows at, and asserts that none was skipped.
    real_scaler = train.GradScaler
    monkeypatch.setattr(train, "GradScaler", lambda *a, **k: real_scaler(*a, **{"init_scale": 16.0, **k}))
    full = tmp_path / "full"
    lines = _run(common + flags + ["--epochs", "2", "--outdir", str(full)], capsys)
    monkeypatch.setattr(train, "save_checkpoint", real_save)
    assert [l["epoch"] for l in lines] == [0, 1]
    print("skipped per epoch:", [l["skipped"] for l in lines], "clipped_frac:", [l["clipped_frac"] for l in lines])
    assert all(l["skipped"] == 0 for l in lines)
    for l in lines:
        assert {"grad_norm_mean", "grad_norm_max", "clipped_frac", "val_loss", "val_mpjpe", "val_loss_raw", "val_mpjpe_raw"} <= set(l)
        assert l["grad_norm_max"] >= l["grad_norm_mean"] > 0 and 0.0 <= l["clipped_frac"] <= 1.0
        assert l["val_mpjpe"] != l["val_mpjpe_raw"]
    last = torch.load(full / "last.pt", map_location="cpu", weights_only=True)
    assert set(last) == {"epoch", "best_val", "model", "optim", "args", "ema"}
    assert set(last["ema"]) == {"decay", "warmup", "updates", "model"} and last["ema"]["decay"] == 0.9 and last["ema"]["warmup"] is True
    assert last["ema"]["updates"] == sum(l["steps"] for l in lines) > 0
    assert last["args"]["clip_grad_norm"] == 50.0 and last["args"]["ema_decay"] == 0.9 and "ema_no_warmup" not in last["args"]
    best = torch.load(full / "best.pt", map_location="cpu", weights_only=True)
    assert best["best_val"] == min(l["val_mpjpe"] for l in lines)                      # the EMA weights' score selects best.pt

    # epoch 0's checkpoint + --resume for the second epoch: the same raw and EMA weights as the uninterrupted run
    resumed = tmp_path / "resumed"
    lines2 = _run(common + flags + ["--epochs", "2", "--outdir", str(resumed), "--resume", str(full / "epoch0.pt")], capsys)
    assert [l["epoch"] for l in lines2] == [1] and lines2[0]["skipped"] == 0
    again = torch.load(resumed / "last.pt", map_location="cpu", weights_only=True)
    for k in last["model"]:
        assert torch.equal(again["model"][k], last["model"][k]), k
        assert torch.equal(again["ema"]["model"][k], last["ema"]["model"][k]), k
    assert again["ema"]["updates"] == last["ema"]["updates"]

    # the readers
    auto, raw, ema = (results.load_head_state(str(full / "best.pt"), which) for which in ("auto", "model", "ema"))
    trainable = train.trainable_names(2)
    for k in best["model"]:
        assert torch.equal(auto[k], best["ema"]["model"][k]) and torch.equal(ema[k], auto[k]) and torch.equal(raw[k], best["model"][k]), k
    assert any(not torch.equal(auto[k], raw[k]) for k in trainable)
    assert all(torch.equal(auto[k], raw[k]) for k in best["model"] if k not in trainable)          # frozen entries are shared

    # a run without the flags writes what it always wrote
    plain = tmp_path / "plain"
    lines3 = _run(common + ["--epochs", "1", "--outdir", str(plain)], capsys)
    assert set(lines3[0]) == {"epoch", "lr", "train_loss", "train_mpjpe", "steps", "skipped", "val_loss", "val_mpjpe"}
    for name in ("last.pt", "best.pt"):
        ck = torch.load(plain / name, map_location="cpu", weights_only=True)
        assert set(ck) == {"epoch", "best_val", "model", "optim", "args"}
        assert not {"clip_grad_norm", "ema_decay", "ema_no_warmup"} & set(ck["args"])
    with pytest.raises(ValueError):
        results.load_head_state(str(plain / "best.pt"), "ema")
