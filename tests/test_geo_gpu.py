"""The geometric pose losses (2D reprojection, velocity, bone length) on the MI355X:
``r50_op_geo_pose_loss_grad`` against the fp64 restatement (tests/geo_reference.py, pinned to the reference's own functions by
tests/golden/geo_golden.pt), its bit-level ties to ``r50_op_mse_loss_grad`` / ``r50_op_future_pose_loss_grad``, the phase-1 and joint
steps with ``geo`` against the reference module's steps, and the ``train_geo`` driver and ``results --geo-metrics``.

Bars.  The op: tests/test_head_kernels_gpu.py's bar for kernels whose arithmetic is the reference's own, 4 x torch's fp32 CPU deviation
from fp64 on the same input, floored at 2^-20 of the result's scale (the case's largest |dy|, resp. the value itself); n_clamped exact.
The steps: section M's rule (tests/test_train_joint_gpu.py).  They start from tests/test_head_train_gpu.py's bounds for phase 1 (tol =
{fp16 1.5e-2, bf16 8e-2}: losses rel 3 tol, gradient norms rel tol, 64-entry gradient slices rel 2 tol; parameter updates with loose
= (1 fp16, 3 bf16): error median < 0.05 loose lr, relative error < 0.3 loose, error max < 2.5 loose lr) and from
tests/test_train_joint_gpu.py's for the joint step (tol = {fp16 1.5e-2, bf16 1.5e-1}).  Then tests/geo_reference.py with store16 (fp64,
loss scale 1024, eval mode) was run against the fixture on the CPU (scripts/geo_emulation_distances.py), and wherever its distance
for a quantity exceeded half the starting tolerance, that quantity's tolerance became twice the measured distance.  Measured
distances (max over the parameters / 2 steps), cases 0 = (64, 2, B 3, T 5), 1 = (128, 2, B 2, T 40):

    precision stage  case | losses   grad norms  grad slices | err median/lr  delta rel  err max/lr
    fp16      phase1 0    | 8.875e-4 8.572e-3    5.681e-2    | 7.960e-3       0.3146     2.340
    fp16      phase1 1    | 7.841e-4 1.957e-3    3.294e-2    | 7.115e-3       0.3669     2.011
    bf16      phase1 0    | 4.941e-3 2.008e-2    1.281e-1    | 3.393e-2       0.3727     3.350
    bf16      phase1 1    | 1.092e-3 5.105e-3    3.749e-2    | 2.553e-2       0.4056     3.888
    fp16      joint  0    | 8.336e-4 7.761e-3    6.043e-2    | 1.898e-2       0.3082     3.339
    fp16      joint  1    | 7.414e-4 6.068e-3    1.071e-1    | 1.967e-2       0.3074     2.272
    bf16      joint  0    | 8.359e-3 5.717e-2    1.995e-1    | 7.063e-2       0.5059     3.471
    bf16      joint  1    | 2.545e-3 8.287e-3    2.238e-1    | 6.537e-2       0.4456     3.913
"""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from tests import geo_reference as gr
from tests import head_kernels_reference as R
from tests import results_data as rd
from tests.geo_driver_data import make_geo_feature_cache
from tests.golden.make_golden_geo import LAMBDAS, geo_batches_for, geo_state_dict, intrinsics, project64
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_KEYS = ("loss", "grad_norm", "grad_slice", "p_med", "p_rel", "p_max")
_BASE_TOL = {"phase1": {"fp16": 1.5e-2, "bf16": 8e-2}, "joint": {"fp16": 1.5e-2, "bf16": 1.5e-1}}
_EMULATION = {     # as scripts/geo_emulation_distances.py prints them, to four digits
    ("fp16", "phase1"): [(8.875e-4, 8.572e-3, 5.681e-2, 7.960e-3, 0.3146, 2.340), (7.841e-4, 1.957e-3, 3.294e-2, 7.115e-3, 0.3669, 2.011)],
    ("bf16", "phase1"): [(4.941e-3, 2.008e-2, 1.281e-1, 3.393e-2, 0.3727, 3.350), (1.092e-3, 5.105e-3, 3.749e-2, 2.553e-2, 0.4056, 3.888)],
    ("fp16", "joint"): [(8.336e-4, 7.761e-3, 6.043e-2, 1.898e-2, 0.3082, 3.339), (7.414e-4, 6.068e-3, 1.071e-1, 1.967e-2, 0.3074, 2.272)],
    ("bf16", "joint"): [(8.359e-3, 5.717e-2, 1.995e-1, 7.063e-2, 0.5059, 3.471), (2.545e-3, 8.287e-3, 2.238e-1, 6.537e-2, 0.4456, 3.913)],
}


def tolerances(precision, stage, case):
    tol = _BASE_TOL[stage][precision]
    loose = 1.0 if precision == "fp16" else 3.0
    base = dict(zip(_KEYS, (3 * tol, tol, 2 * tol, 0.05 * loose, 0.3 * loose, 2.5 * loose)))
    return {k: (2 * m if m > base[k] / 2 else base[k]) for k, m in zip(_KEYS, _EMULATION[(precision, stage)][case])}


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLDEN / "geo_golden.pt", map_location="cpu", weights_only=True)


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return make_geo_feature_cache(tmp_path_factory.mktemp("cache_geo"), clips_per_subject=8)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _edges_c(edges):
    flat = [v for e in edges for v in e]
    return (C.c_int * max(len(flat), 1))(*flat)


def _op(lib, inp, edges, lam, s0=0, term_scale=1.0, loss_scale=1.0, with_dy=True, eps=1e-6):
    """One call on device copies of ``inp`` = (pred, g3d, g2d, K).  Returns (rc, dy (B,T,J,3) cpu or None, out8 cpu, guard ok)."""
    pred, g3d, g2d, k = (v.to(DEV).contiguous() for v in inp)
    b, t, j, _ = pred.shape
    buf = torch.full((b * t * j * 3 + 64,), 7.0, dtype=torch.float32, device=DEV)            # guard band behind dy
    part = torch.empty(8 * b, dtype=torch.float64, device=DEV)
    out8 = torch.full((8,), -1.0, dtype=torch.float32, device=DEV)
    rc = lib.r50_op_geo_pose_loss_grad(pred.data_ptr(), g3d.data_ptr(), g2d.data_ptr(), k.data_ptr(), b, t, s0, j, _edges_c(edges), len(edges),
                                       lam[0], lam[1], lam[2], eps, term_scale, loss_scale, buf.data_ptr() if with_dy else None,
                                       part.data_ptr(), out8.data_ptr(), _stream())
    torch.cuda.synchronize()
    n = b * t * j * 3
    guard = bool((buf[n:] == 7.0).all()) and (with_dy or bool((buf == 7.0).all()))
    return rc, (buf[:n].view(b, t, j, 3).cpu() if with_dy else None), out8.cpu(), guard


def _big_case(b, t, seed):
    """(pred, g3d, g2d, K) at a driver's size: poses at 4-5 m whose limbs are 0.2-0.5 m long (the skeleton grown along H36M_EDGES), so
    that among millions of bones none comes out shorter than 1e-2 by chance; predictions 5 cm off, joints2d one pixel off."""
    from implementation_phd_lab_vision_amd.train import H36M_EDGES
    g = torch.Generator().manual_seed(seed)
    root = torch.cat([torch.rand(b, 1, 2, generator=g) - 0.5, 4.0 + torch.rand(b, 1, 1, generator=g)], dim=-1)
    body = torch.zeros(b, 17, 3)
    for a, c in H36M_EDGES:
        d = torch.randn(b, 3, generator=g)
        body[:, c] = body[:, a] + d / d.norm(dim=-1, keepdim=True) * (0.2 + 0.3 * torch.rand(b, 1, generator=g))
    gt = (root[:, None] + 0.01 * torch.randn(b, t, 1, 3, generator=g).cumsum(dim=1) + body[:, None] + 0.01 * torch.randn(b, t, 17, 3, generator=g))
    gt[..., 2].clamp_(min=2.0)
    k = intrinsics(b, g)
    pred = gt + 0.05 * torch.randn(b, t, 17, 3, generator=g)
    return pred, gt, (project64(gt, k) + torch.randn(b, t, 17, 2, generator=g).double()).float(), k


def _op_cases(gold):
    """(name, inputs, [lambda sets]): every fixture case, then the drivers' sizes."""
    out = [(c["name"], (c["pred"], c["joints3d"], c["joints2d"], c["K"]), [tuple(s["lambdas"]) for s in c["sets"]]) for c in gold["op"]]
    out += [(f"b{b}", _big_case(b, 40, 40 + b), [LAMBDAS]) for b in (256, 32)]
    out.append(("t256", _big_case(3, 256, 92), [LAMBDAS]))                     # T 256 at J 17: the largest clip the op must stage
    return out


# ------------------------------------------------------------------ 1. the op against fp64 ------------------------------------------
def test_op_against_fp64_reference(lib, gold):
    edges = [tuple(e) for e in gold["edges"]]
    worst = {}
    for name, inp, sets in _op_cases(gold):
        t = inp[0].shape[1]
        z = torch.einsum("bij,btnj->btni", inp[3].double(), inp[0].double())[..., 2]
        bl = gr.bone_lengths(inp[0].double(), edges)
        # no element has to be left out: none near the clamp, no bone between 0 and 1e-2 (the mask from the fp64 values is empty)
        assert int((((z > -0.1) & (z < 1.0)).sum() + ((bl > 0) & (bl < 1e-2)).sum())) == 0, name
        for lam in sets:
            for s0, ts, ls in ((0, 1.0, 1.0), (1, 0.5, 4.0)):
                if t - s0 < 1 or (lam[1] != 0 and t - s0 < 2):
                    continue                                   # the op refuses these by contract (test_refusals)
                ref8, ref_g = gr.geo_loss_grad(*inp, edges, lam, s0=s0, scale=ts * ls)
                t8, t_g = gr.geo_loss_grad(*inp, edges, lam, s0=s0, scale=ts * ls, dtype=torch.float32)
                rc, dy, out8, guard = _op(lib, inp, edges, lam, s0, ts, ls)
                assert rc == 0, (name, lam, s0, lib.r50_last_error(None))
                assert guard, "wrote past the end of dy"
                assert bool(torch.isfinite(dy).all()) and bool(torch.isfinite(out8).all()), (name, lam, s0)
                bar = R.bar_from(t_g, ref_g)
                err = float((dy.double() - ref_g).abs().max())
                ratio = err / bar
                print(f"{name} lam {lam} s0 {s0}: dy err {err:.3g} bar {bar:.3g} (max |dy| {float(ref_g.abs().max()):.3g})")
                assert err <= bar, (name, lam, s0, err, bar)
                if s0 == 1:
                    assert not bool(dy[:, 0].any()) and not bool(torch.signbit(dy[:, 0]).any()), "frame-0 rows must be exact +0"
                for i, key in enumerate(gr.OUT8):
                    if key == "n_clamped":
                        assert float(out8[i]) == float(ref8[i]), (name, lam, s0)
                        continue
                    kbar = R.bar_from(t8[i], ref8[i])
                    kerr = abs(float(out8[i]) - float(ref8[i]))
                    print(f"    {key}: {float(out8[i])!r} fp64 {float(ref8[i])!r} err {kerr:.3g} bar {kbar:.3g}")
                    assert kerr <= kbar, (name, lam, s0, key, float(out8[i]), float(ref8[i]), kbar)
                    ratio = max(ratio, kerr / kbar if kbar > 0 else 0.0)
                worst[name] = max(worst.get(name, 0.0), ratio)
                rc, none, out8_eval, guard = _op(lib, inp, edges, lam, s0, ts, ls, with_dy=False)
                assert rc == 0 and none is None and guard, "dy = NULL must store no gradient"
                assert torch.equal(out8_eval, out8), (name, lam, s0)
    print("worst error / bar per case:", {k: round(v, 3) for k, v in worst.items()})


# ------------------------------------------------------------------ 2. ties to the existing kernels ----------------------------------
def test_zero_lambdas_give_the_existing_kernels_bits(lib, gold):
    from implementation_phd_lab_vision_amd import _lib
    edges = [tuple(e) for e in gold["edges"]]
    for inp in [(c["pred"], c["joints3d"], c["joints2d"], c["K"]) for c in gold["op"] if c["t"] > 1] + [_big_case(32, 40, 72)]:
        b, t, j, _ = inp[0].shape
        y, gt = inp[0].to(DEV).contiguous(), inp[1].to(DEV).contiguous()
        for ls in (1.0, 1024.0):
            want, l2 = torch.empty_like(y), torch.empty(2, device=DEV)
            _lib.check(lib.r50_op_mse_loss_grad(y.data_ptr(), gt.data_ptr(), y.numel(), ls, want.data_ptr(), l2.data_ptr(), _stream()), None, "mse")
            rc, dy, out8, _ = _op(lib, inp, edges, (0.0, 0.0, 0.0), 0, 1.0, ls)
            assert rc == 0 and torch.equal(dy.view(torch.int32), want.cpu().view(torch.int32)), "s0 = 0: r50_op_mse_loss_grad's bits"
            assert out8[:3].tolist() == pytest.approx([float(l2[0]), float(l2[0]), float(l2[1])], rel=1e-5)
            _lib.check(lib.r50_op_future_pose_loss_grad(y.data_ptr(), gt.data_ptr(), b, t, j, ls, want.data_ptr(), l2.data_ptr(), _stream()),
                       None, "future")
            rc, dy, out8, _ = _op(lib, inp, edges, (0.0, 0.0, 0.0), 1, 1.0, ls)
            assert rc == 0 and torch.equal(dy.view(torch.int32), want.cpu().view(torch.int32)), "s0 = 1: r50_op_future_pose_loss_grad's bits"
            assert not bool(dy[:, 0].view(torch.int32).any())                                  # exact +0
            assert out8[:3].tolist() == pytest.approx([float(l2[0]), float(l2[0]), float(l2[1])], rel=1e-6)


def test_a_term_at_lambda_zero_contributes_nothing(lib, gold):
    edges = [tuple(e) for e in gold["edges"]]
    c = gold["op"][1]
    inp = (c["pred"], c["joints3d"], c["joints2d"], c["K"])
    _, dy, out8, _ = _op(lib, inp, edges, (0.0, 0.7, 1.3))
    other = (inp[0], inp[1], inp[2] * 3.0 + 50.0, inp[3].flip(0) * 1.5)
    _, dy2, out8b, _ = _op(lib, other, edges, (0.0, 0.7, 1.3))
    assert torch.equal(dy.view(torch.int32), dy2.view(torch.int32)) and float(out8b[3]) != float(out8[3])      # still reported
    assert float(out8b[0]) == float(out8[0])
    _, dy, out8, _ = _op(lib, inp, edges, (1e-4, 0.7, 0.0))
    _, dy2, out8b, _ = _op(lib, inp, [(0, 16), (3, 9)], (1e-4, 0.7, 0.0))
    assert torch.equal(dy.view(torch.int32), dy2.view(torch.int32)) and float(out8b[6]) != float(out8[6])
    _, dy2, out8b, _ = _op(lib, inp, [], (1e-4, 0.7, 0.0))
    assert torch.equal(dy.view(torch.int32), dy2.view(torch.int32)) and float(out8b[6]) == 0.0
    one = gold["op"][3]                                                                            # one frame: l_vel reported as 0
    _, _, out8, _ = _op(lib, (one["pred"], one["joints3d"], one["joints2d"], one["K"]), edges, (1e-4, 0.0, 1.3))
    assert float(out8[5]) == 0.0


# ------------------------------------------------------------------ 3. the same bits on every run ------------------------------------
def test_two_launches_same_bits(lib, gold):
    edges = [tuple(e) for e in gold["edges"]]
    for inp in (_big_case(256, 40, 91), _big_case(3, 256, 92)):                 # T 256 at J 17: the largest clip the op stages
        for s0 in (0, 1):
            a = _op(lib, inp, edges, LAMBDAS, s0, 1.0, 512.0)
            b = _op(lib, inp, edges, LAMBDAS, s0, 1.0, 512.0)
            assert a[0] == 0 and b[0] == 0 and a[3] and b[3]
            assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


# ------------------------------------------------------------------ 4. refusals -----------------------------------------------------
def test_refusals_leave_dy_untouched(lib, gold):
    edges = [tuple(e) for e in gold["edges"]]
    c = gold["op"][0]
    inp = (c["pred"], c["joints3d"], c["joints2d"], c["K"])
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(lam=(-1.0, 0, 0)), b"lambdas"), (dict(lam=(0, nan, 0)), b"lambdas"), (dict(lam=(0, 0, inf)), b"lambdas"),
                     (dict(s0=2), b"s0"), (dict(s0=-1), b"s0"), (dict(eps=0.0), b"eps"), (dict(eps=-1e-6), b"eps"),
                     (dict(edges=[(0, 17)]), b"edge index"), (dict(edges=[(-1, 0)]), b"edge index"),
                     (dict(edges=[(0, 1)] * 65), b"n_edges")):
        args = dict(edges=edges, lam=LAMBDAS, s0=0, eps=1e-6)
        args.update(kw)
        rc, dy, out8, guard = _op(lib, inp, args["edges"], args["lam"], args["s0"], eps=args["eps"])
        assert rc == -1 and word in lib.r50_last_error(None), (kw, lib.r50_last_error(None))
        assert bool((dy == 7.0).all()) and guard and bool((out8 == -1.0).all()), kw
    one = gold["op"][3]
    one_inp = (one["pred"], one["joints3d"], one["joints2d"], one["K"])
    for lam, s0, word in ((LAMBDAS, 0, b"t - s0 >= 2"), ((0.0, 0.0, 0.0), 1, b"t - s0 >= 1")):
        rc, dy, _, _ = _op(lib, one_inp, edges, lam, s0)
        assert rc == -1 and word in lib.r50_last_error(None) and bool((dy == 7.0).all())
    rc, dy, _, _ = _op(lib, _big_case(1, 272, 5), edges, LAMBDAS)                 # 272 * 17 > 4608
    assert rc == -1 and b"4608" in lib.r50_last_error(None) and bool((dy == 7.0).all())


# ------------------------------------------------------------------ 5. the steps against the reference module ------------------------
def _check_step_case(c, tol, m, sd, names, step_losses, grads):
    for s in range(2):
        print("losses", s, step_losses[s], c["losses"][s])
        assert step_losses[s] == pytest.approx(c["losses"][s], rel=tol["loss"]), (s, step_losses[s], c["losses"][s])
    assert sorted(grads) == sorted(names)
    for i, k in enumerate(names):
        n = c["head_len"][i]
        assert float(grads[k].norm()) == pytest.approx(c["grad_norm"][i], rel=tol["grad_norm"]), k
        r = _rel(grads[k].reshape(-1)[:n], c["grad_head"][i][:n])
        assert r < tol["grad_slice"], (k, r)
    final = m.state_dict()
    for i, k in enumerate(names):
        n = c["head_len"][i]
        delta_want = c["param_head"][i][:n] - sd[k].reshape(-1)[:n]
        delta_got = final[k].reshape(-1)[:n] - sd[k].reshape(-1)[:n]
        assert float(delta_want.abs().max()) > 0
        err = (delta_got - delta_want).abs()
        assert float(err.median()) < tol["p_med"] * c["lr"], (k, float(err.median()))
        assert _rel(delta_got, delta_want) < tol["p_rel"], (k, _rel(delta_got, delta_want))
        assert float(err.max()) < tol["p_max"] * c["lr"], (k, float(err.max()))
    assert torch.equal(final["f_3D.y0"], sd["f_3D.y0"])


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_phase1_steps_equal_reference_module(lib, gold, precision):
    from implementation_phd_lab_vision_amd import train
    geo = train.GeoWeights(*LAMBDAS)
    for ci, c in enumerate(gold["steps"]):
        sd = geo_state_dict(c["latent_dim"], c["number_blocks"], c["seed"])
        m = train.TrainableHead(c["latent_dim"], 17, c["number_blocks"], precision=precision)
        m.load_state_dict(sd); m.to(DEV)
        m.eval()                                                   # the fixture's steps ran with dropout = identity
        optim, scaler = train.AdamW(m, lr=c["lr"], weight_decay=1e-2), train.GradScaler(init_scale=1024.0)
        step_losses, grads = [], None
        for s, batch in enumerate(geo_batches_for(c["seed"], c["b"], c["t"])):
            feats, gt, j2d, k = (v.to(DEV) for v in batch)
            loss, mpjpe, skipped = m.train_step(feats, gt, optim, scaler, joints2d=j2d, K=k, geo=geo)
            assert not skipped and loss == m.last_losses["loss"] and mpjpe == m.last_losses["mpjpe"]
            assert m.last_losses["n_clamped"] == 0.0 and set(m.last_losses) == set(train.GEO_KEYS)
            step_losses.append([loss] + [m.last_losses[n] for n in ("l3d", "l2d", "l_vel", "l_bone")])
            if s == 0:
                grads = m.named_gradients()
        _check_step_case(c, tolerances(precision, "phase1", ci), m, sd, c["trainable"], step_losses, grads)
        assert optim.step_count == 2


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_joint_steps_equal_reference_module(lib, gold, precision):
    from implementation_phd_lab_vision_amd import train, train_joint
    geo = train.GeoWeights(*LAMBDAS)
    for ci, c in enumerate(gold["joint_steps"]):
        sd = geo_state_dict(c["latent_dim"], c["number_blocks"], c["seed"])
        m = train_joint.JointTrainableHead(c["latent_dim"], 17, c["number_blocks"], precision=precision, lambda_future=c["lambda_future"],
                                           lambda_latent=c["lambda_latent"])
        m.load_state_dict(sd); m.to(DEV)
        m.eval()
        optim, scaler = train.AdamW(m, lr=c["lr"], weight_decay=1e-2), train.GradScaler(init_scale=1024.0)
        step_losses, grads = [], None
        for s, batch in enumerate(geo_batches_for(c["seed"], c["b"], c["t"])):
            feats, gt, j2d, k = (v.to(DEV) for v in batch)
            loss, mpjpe, skipped = m.train_step(feats, gt, optim, scaler, joints2d=j2d, K=k, geo=geo)
            ll = m.last_losses
            assert not skipped and loss == ll["loss"] and ll["n_clamped"] == 0.0 and ll["n_clamped_hat"] == 0.0
            step_losses.append([loss] + [ll[n] for n in ("l3d", "l2d", "l_vel", "l_bone", "l3d_hat", "l2d_hat", "l_vel_hat", "l_bone_hat", "l_lat")])
            if s == 0:
                grads = m.named_gradients()
        _check_step_case(c, tolerances(precision, "joint", ci), m, sd, c["trainable"], step_losses, grads)


# ------------------------------------------------------------------ 6. degenerate weights, graphs -------------------------------------
def _batch(b, t, seed):
    feats, gt, j2d, k = geo_batches_for(seed, b, t)[0]
    return feats.to(DEV), gt.to(DEV), j2d.to(DEV), k.to(DEV)


def test_zero_weights_equal_no_geo_bit_for_bit(lib):
    from implementation_phd_lab_vision_amd import train, train_joint
    zero = train.GeoWeights(0.0, 0.0, 0.0)
    feats, gt, j2d, k = _batch(4, 10, 3)
    sd = geo_state_dict(128, 2, 77)
    for cls, kw in ((train.TrainableHead, {}), (train_joint.JointTrainableHead, dict(lambda_future=0.5, lambda_latent=0.25))):
        got = []
        for geo in (None, zero):
            m = cls(128, 17, 2, **kw)
            m.load_state_dict(sd); m.to(DEV)
            m.eval()
            out = m.forward_backward(feats, gt, 256.0, None, *((j2d, k, geo) if geo is not None else ()))
            torch.cuda.synchronize()
            got.append((m.flat_grad.clone(), out[-1].clone()))
        assert torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32)), cls.__name__
        assert bool(got[0][0].any())
        if cls is train.TrainableHead:                 # loss2 = [l3d, mpjpe]: the op's sums are fp64, mse_loss_grad's fp32
            assert got[1][1].tolist() == pytest.approx(got[0][1].tolist(), rel=1e-5)
        else:                                          # [l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat]: fp64 sums on both sides
            assert got[1][1].tolist() == pytest.approx(got[0][1].tolist(), rel=1e-6)
    with pytest.raises(ValueError):
        m.forward_backward(feats, gt, 256.0, None, None, None, zero)                     # geo needs joints2d and K
    with pytest.raises(ValueError, match="per-frame"):
        m.forward_backward(feats, gt, 256.0, None, j2d, k[:, None].expand(4, 10, 3, 3), zero)


def test_graphed_geo_step_equals_eager(lib):
    from implementation_phd_lab_vision_amd import train
    geo = train.GeoWeights(*LAMBDAS)
    batches = [_batch(4, 10, s) for s in (5, 6, 7)]
    finals = []
    for graphed in (False, True):
        m = train.TrainableHead(128, 17, 2)
        m.load_state_dict(geo_state_dict(128, 2, 51)); m.to(DEV)
        m.eval().enable_graphs(graphed)
        optim, scaler = train.AdamW(m, lr=1e-5), train.GradScaler(init_scale=512.0)     # small steps: the poses stay in front of the camera
        rows = []
        for f, y, j2d, k in batches:
            loss, _, skipped = m.train_step(f, y, optim, scaler, joints2d=j2d, K=k, geo=geo)
            assert not skipped
            rows.append((loss, dict(m.last_losses)))
        finals.append((rows, m.flat_grad.clone(), m.flat_master.clone()))
        if graphed:
            assert len(m._graphs) == 1
            m.train_step(*batches[0][:2], optim, scaler)                        # without geo: a graph of its own
            m.train_step(*batches[0][:2], optim, scaler, joints2d=batches[0][2], K=batches[0][3], geo=train.GeoWeights(0.0, 0.7, 1.3))
            assert len(m._graphs) == 3
    assert finals[0][0] == finals[1][0]
    assert torch.equal(finals[0][1], finals[1][1]) and torch.equal(finals[0][2], finals[1][2])


# ------------------------------------------------------------------ 7. the driver and results --------------------------------------
_GEO = ("l2d", "reproj_px", "l_vel", "l_bone", "n_clamped")


def _lines(capsys):
    return [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def _same_model(a, b):
    return all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"]) and set(a["model"]) == set(b["model"])


def test_driver_phase1_and_results(lib, cache, tmp_path, capsys):
    from implementation_phd_lab_vision_amd import results, train, train_geo
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    common = ["--train", str(cache), "--val", str(cache), "--batch-size", "8", "--seed", "3", "--log-every", "0", "--early-stop-patience", "0",
              "--lambda-vel", "0.5", "--lambda-bone", "2.0"]
    train_geo.main([*common, "--epochs", "2", "--lambda-2d", "1e-6", "--warmup-2d-epochs", "1", "--outdir", str(tmp_path / "a")])
    a = _lines(capsys)
    train_geo.main([*common, "--epochs", "1", "--lambda-2d", "1e-6", "--warmup-2d-epochs", "1", "--outdir", str(tmp_path / "a1")])
    a1 = _lines(capsys)
    train_geo.main([*common, "--epochs", "1", "--lambda-2d", "0", "--outdir", str(tmp_path / "b")])
    b = _lines(capsys)
    assert [e["epoch"] for e in a] == [0, 1] and len(a1) == 1 and len(b) == 1
    want = {"epoch", "lr", "train_loss", "train_mpjpe", "steps", "skipped", "val_loss", "val_mpjpe", "lambda_2d_active"} | \
           {f"{s}_{k}" for s in ("train", "val") for k in _GEO}
    for e in a:
        assert set(e) == want and all(math.isfinite(float(v)) for v in e.values()), e
    assert a[0]["lambda_2d_active"] == 0.0 and a[1]["lambda_2d_active"] == 1e-6 and a[0]["train_l2d"] > 0 and a[0]["steps"] > 0
    assert a[0] == a1[0]                                                    # epoch 0 does not depend on --epochs
    # the warm-up epoch is the --lambda-2d 0 run, bit for bit
    la1, lb = torch.load(tmp_path / "a1" / "last.pt", weights_only=True), torch.load(tmp_path / "b" / "last.pt", weights_only=True)
    assert _same_model(la1, lb) and {k: v for k, v in a1[0].items()} == {k: v for k, v in b[0].items()}
    last = torch.load(tmp_path / "a" / "last.pt", weights_only=True)
    assert last["epoch"] == 1 and (last["args"]["lambda_vel"], last["args"]["lambda_bone"], last["args"]["stage"]) == (0.5, 2.0, "phase1")
    best = torch.load(tmp_path / "a" / "best.pt", weights_only=True)
    assert best["best_val"] == min(e["val_mpjpe"] for e in a)                # best.pt follows val MPJPE, whatever the weights

    # results: best.pt loads, --geo-metrics prints the five numbers = evaluate(..., geo=...)'s over the same batches
    videos = rd.make_preprocessed_tree(tmp_path / "videos")
    out = tmp_path / "res" / "batch.npz"
    argv = ["--features_root", str(cache), "--preprocessed_root", str(videos), "--model_path", str(tmp_path / "a" / "best.pt"), "--out", str(out),
            "--seq-len", str(rd.SEQ_LEN), "--batch-size", "4", "--save-n", "2", "--video-size", "32", "--seed", "0", "--video-reader",
            "tests.results_data:read_video"]
    results.main(argv)
    plain = capsys.readouterr().out
    assert "Geo metrics" not in plain and "geo_metrics" not in np.load(out, allow_pickle=True).files
    results.main([*argv, "--geo-metrics"])
    text = capsys.readouterr().out
    line = next(l for l in text.splitlines() if l.startswith("Geo metrics | "))
    assert text.index("Test metrics") < text.index("Geo metrics")
    store = DeviceFeatureStore(str(cache), subjects=[9], test_set=True, device=DEV)
    head = results.build_head(results.load_head_state(str(tmp_path / "a" / "best.pt")), DEV)
    order, _ = results.loader_batch_order(len(store), 4, 0)
    geo = train.GeoWeights()
    loss, mpjpe, l3d, l2d = train.evaluate(head, store, 4, test_set=True, batches=order, geo=geo)
    g = head.last_eval_geo
    assert (loss, mpjpe, l3d, l2d) == (g["loss"], g["mpjpe"], g["l3d"], g["l2d"]) and l2d > 0
    assert line == "Geo metrics | " + " | ".join(f"{k}: {g[k]:.6f}" for k in _GEO)
    npz = np.load(out, allow_pickle=True)
    assert list(npz["geo_metric_names"]) == list(_GEO) and npz["geo_metrics"].tolist() == [g[k] for k in _GEO]
    plain_eval = train.evaluate(head, store, 4, test_set=True, batches=order)
    assert plain_eval[3] == 0.0 and plain_eval[1] == pytest.approx(mpjpe, rel=1e-6) and plain_eval[2] == pytest.approx(l3d, rel=1e-6)


def test_driver_joint(lib, cache, tmp_path, capsys):
    from implementation_phd_lab_vision_amd import results, train_geo
    from implementation_phd_lab_vision_amd.train import default_state_dict
    torch.save(default_state_dict(1024, 17, 2, seed=5), tmp_path / "init.pt")
    common = ["--stage", "joint", "--init", str(tmp_path / "init.pt"), "--train", str(cache), "--val", str(cache), "--batch-size", "8", "--seed", "3",
              "--log-every", "0", "--early-stop-patience", "0", "--lambda-future", "0.5", "--lambda-latent", "0.25"]
    train_geo.main([*common, "--epochs", "2", "--lambda-2d", "1e-6", "--warmup-2d-epochs", "1", "--outdir", str(tmp_path / "a")])
    a = _lines(capsys)
    train_geo.main([*common, "--epochs", "1", "--lambda-2d", "1e-6", "--warmup-2d-epochs", "1", "--outdir", str(tmp_path / "a1")])
    a1 = _lines(capsys)
    train_geo.main([*common, "--epochs", "1", "--lambda-2d", "0", "--outdir", str(tmp_path / "b")])
    b = _lines(capsys)
    terms = ("loss", "l3d", "mpjpe", "l3d_hat", "mpjpe_hat", "l_lat") + _GEO + tuple(k + "_hat" for k in _GEO)
    want = {"epoch", "lr", "steps", "skipped", "val_mpjpe_sum", "lambda_2d_active"} | {f"{s}_{k}" for s in ("train", "val") for k in terms}
    assert [e["epoch"] for e in a] == [0, 1]
    for e in a:
        assert set(e) == want and all(math.isfinite(float(v)) for v in e.values()), e
    assert a[0]["lambda_2d_active"] == 0.0 and a[1]["lambda_2d_active"] == 1e-6 and a[0]["train_l2d_hat"] > 0 and a[0]["steps"] > 0
    assert a[0] == a1[0] and a1[0] == b[0]
    assert _same_model(torch.load(tmp_path / "a1" / "last.pt", weights_only=True), torch.load(tmp_path / "b" / "last.pt", weights_only=True))
    best = torch.load(tmp_path / "a" / "best.pt", weights_only=True)
    assert best["best_val"] == min(e["val_mpjpe_sum"] for e in a) and best["args"]["stage"] == "joint"
    assert results.infer_head_dims(results.load_head_state(str(tmp_path / "a" / "best.pt"))) == (1024, 17, 2)
