"""Global-norm gradient clipping and EMA weights without a GPU: the tests' fp64 restatement against
torch's own ``clip_grad_norm_`` / ``AdamW`` / ``AveragedModel``, the EMA's warm-up weights, the four drivers' parsers with and
without the new flags, ``results.load_head_state``'s three modes, and the argument checks of the two new C-ABI entries."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from tests.clip_ema_reference import ClipAdamWEMA, clip_coef, ema_weight, global_norm

from implementation_phd_lab_vision_amd import predict, results, train, train_ar, train_geo, train_joint
from implementation_phd_lab_vision_amd.trainable import WeightEMA

RTOL, ATOL = 1e-5, 1e-6            # the bar of test_adamw_kernel_equals_torch_adamw


class _Params(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])


def test_restatement_equals_torch_clip_adamw_ema():
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    g = torch.Generator().manual_seed(21)
    shapes = [(7, 5), (33,), (4, 3, 3)]
    init = [torch.randn(s, generator=g) for s in shapes]
    max_norm, decay, lr = 2.0, 0.9, 1e-3
    # step 1's gradient has norm ~ 30 (clipped), step 2's ~ 3 (clipped), step 3's ~ 0.3 (not clipped)
    grads = [[torch.randn(s, generator=g) * scale for s in shapes] for scale in (3.0, 0.3, 0.03)]
    model = _Params(init)
    opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=1e-2)
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    avg.update_parameters(model)                         # n_averaged 0 -> 1: the average starts AT the initial weights, as WeightEMA's
    ref = ClipAdamWEMA(init, lr, max_norm=max_norm)
    for step_grads in grads:
        for p, gr in zip(model.ps, step_grads):
            p.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        opt.step()
        avg.update_parameters(model)
        ref.step(step_grads, w=1.0 - decay)
        assert float(total) == pytest.approx(ref.norms[-1], rel=1e-6)
        for i, (p, gr) in enumerate(zip(model.ps, step_grads)):
            torch.testing.assert_close(p.grad.double(), gr.double() * ref.coefs[-1], rtol=RTOL, atol=ATOL)     # the clipped gradient
            torch.testing.assert_close(p.detach().double(), ref.p[i], rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(avg.module.ps[i].detach().double(), ref.ema[i], rtol=RTOL, atol=ATOL)
    assert ref.coefs[0] < 1.0 and ref.coefs[-1] == 1.0, ref.coefs          # the run had both a clipped and an unclipped step
    assert ref.norms[0] > max_norm > ref.norms[-1]
    assert clip_coef(global_norm(grads[0]), None) == 1.0 and clip_coef(5.0, 0.0) == 1.0


def test_ema_weight_with_and_without_warmup():
    head = SimpleNamespace(flat_master=torch.arange(8, dtype=torch.float32))
    for decay in (0.9, 0.999):
        warm, cold = WeightEMA(head, decay), WeightEMA(head, decay, warmup=False)
        assert torch.equal(warm.flat, head.flat_master) and warm.flat.data_ptr() != head.flat_master.data_ptr() and warm.updates == 0
        for u in (0, 1, 9, 10 ** 6):
            warm.updates = cold.updates = u
            assert warm.weight() == 1.0 - min(decay, (1.0 + u) / (10.0 + u)) == ema_weight(decay, u, True)
            assert cold.weight() == 1.0 - decay == ema_weight(decay, u, False)
    w = WeightEMA(head, 0.999)
    assert w.weight() == pytest.approx(0.9)                # update 0: decay 1/10
    w.updates = 9
    assert w.weight() == pytest.approx(1.0 - 10.0 / 19.0)
    w.updates = 10 ** 6
    assert w.weight() == pytest.approx(1e-3)               # the warm-up has run out: the decay itself
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            WeightEMA(head, bad)


FLAGS = ["--clip-grad-norm", "1.5", "--ema-decay", "0.99", "--ema-no-warmup"]
NEW_KEYS = {"clip_grad_norm", "ema_decay", "ema_no_warmup"}


def _parsers():
    """(name, parse function, the arguments the stage needs anyway)."""
    return (("train", lambda argv: train.validate_clip_ema(train.build_parser(), train.build_parser().parse_args(argv)), []),
            ("train_ar", train_ar.parse_args, ["--init", "phase1.pt"]),
            ("train_joint", train_joint.parse_args, ["--init", "phase2.pt"]),
            ("train_geo", train_geo.parse_args, []),
            ("train_geo joint", train_geo.parse_args, ["--stage", "joint", "--init", "phase2.pt"]))


def test_parsers_without_the_flags_are_what_they_were(gold_parser_defaults):
    # tests/test_train_driver_cpu.py::test_parser_defaults_equal_reference
    args = vars(train.build_parser().parse_args([]))
    ref = gold_parser_defaults
    assert {k: args[k] for k in ref} == ref
    assert set(args) - set(ref) == {"precision", "seed", "train_subjects", "val_subjects"}
    # tests/test_train_ar_cpu.py::test_parser_defaults_and_init_rule
    ar = vars(train_ar.parse_args(["--init", "phase1.pt"]))
    assert set(ar) == set(args) | {"init", "lambda_latent"}
    assert {k: v for k, v in ar.items() if k not in ("outdir", "init", "lambda_latent")} == {k: v for k, v in args.items() if k != "outdir"}
    # tests/test_train_joint_cpu.py::test_parser_defaults_and_rules
    jo = vars(train_joint.parse_args(["--init", "phase2.pt"]))
    assert set(jo) == set(args) | {"init", "lambda_future", "lambda_latent"}
    assert {k: v for k, v in jo.items() if k not in ("outdir", "init", "lambda_future", "lambda_latent")} == \
        {k: v for k, v in args.items() if k != "outdir"}
    for name, parse, need in _parsers():
        ns = parse(need)
        assert not NEW_KEYS & set(vars(ns)) and not hasattr(ns, "weights_from"), name
        assert train.clip_ema_options(ns) == (None, None, True), name


@pytest.fixture(scope="module")
def gold_parser_defaults():
    from tests.helpers import GOLDEN
    return torch.load(GOLDEN / "sampler_golden.pt", weights_only=True)["parser_defaults"]


def test_parsers_with_the_flags():
    for name, parse, need in _parsers():
        without, ns = vars(parse(need)), parse(need + FLAGS)
        assert (ns.clip_grad_norm, ns.ema_decay, ns.ema_no_warmup) == (1.5, 0.99, True), name
        assert train.clip_ema_options(ns) == (1.5, 0.99, False), name
        assert {k: v for k, v in vars(ns).items() if k not in NEW_KEYS} == without, name
        assert train.clip_ema_options(parse(need + ["--ema-decay", "0.5"])) == (None, 0.5, True), name
        for bad in (["--clip-grad-norm", "0"], ["--clip-grad-norm", "-1"], ["--clip-grad-norm", "nan"], ["--clip-grad-norm", "inf"],
                    ["--ema-decay", "0"], ["--ema-decay", "1"], ["--ema-decay", "nan"], ["--ema-no-warmup"],
                    ["--ema-no-warmup", "--clip-grad-norm", "1"]):
            with pytest.raises(SystemExit):
                parse(need + bad)
    assert train_ar.parse_args(["--init", "a.pt", "--weights-from", "model"]).weights_from == "model"
    assert train_geo.parse_args(["--stage", "joint", "--init", "a.pt", "--weights-from", "ema"]).weights_from == "ema"
    with pytest.raises(SystemExit):
        train_joint.parse_args(["--init", "a.pt", "--weights-from", "best"])
    r = results.build_parser().parse_args(["--features_root", "F", "--preprocessed_root", "P", "--model_path", "M"])
    p = predict.build_parser().parse_args(["--frames", "a.npy", "--model_path", "m.pt", "--out", "o"])
    assert r.weights_from == p.weights_from == "auto"
    assert results.build_parser().parse_args(["--features_root", "F", "--preprocessed_root", "P", "--model_path", "M", "--weights-from",
                                              "ema"]).weights_from == "ema"
    assert predict.build_parser().parse_args(["--frames", "a.npy", "--model_path", "m.pt", "--out", "o", "--weights-from",
                                              "model"]).weights_from == "model"


def test_load_head_state_modes(tmp_path):
    raw = {"input_proj.weight": torch.zeros(4, 2048), "f_3D.y0": torch.arange(51.0)}
    avg = {k: v + 1.0 for k, v in raw.items()}
    with_ema, without, plain = tmp_path / "ema.pt", tmp_path / "raw.pt", tmp_path / "plain.pt"
    torch.save({"epoch": 1, "best_val": 0.5, "model": raw, "optim": {}, "args": {},
                "ema": {"decay": 0.9, "warmup": True, "updates": 3, "model": avg}}, with_ema)
    torch.save({"epoch": 1, "best_val": 0.5, "model": raw, "optim": {}, "args": {}}, without)
    torch.save(raw, plain)

    def same(a, b):
        return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)

    assert same(results.load_head_state(str(with_ema)), avg) and same(results.load_head_state(str(with_ema), "auto"), avg)
    assert same(results.load_head_state(str(with_ema), "ema"), avg) and same(results.load_head_state(str(with_ema), "model"), raw)
    for path in (without, plain):                                  # files from before the feature load as they did
        assert same(results.load_head_state(str(path)), raw) and same(results.load_head_state(str(path), "model"), raw)
        with pytest.raises(ValueError, match="no EMA weights"):
            results.load_head_state(str(path), "ema")
    with pytest.raises(ValueError):
        results.load_head_state(str(with_ema), "best")


def test_new_ops_refuse_bad_arguments_without_a_gpu(lib_built):
    """The refusals come before any launch, so they need no device: null pointers, n < 1, a ``part`` smaller than the workgroup
    count, a misaligned gradient."""
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    for args, word in (((None, 64, 1.0, a, 1, a, a, a, None), b"null"), ((a, 64, 1.0, None, 1, a, a, a, None), b"null"),
                       ((a, 64, 1.0, a, 1, None, a, a, None), b"null"), ((a, 64, 1.0, a, 1, a, None, a, None), b"null"),
                       ((a, 64, 1.0, a, 1, a, a, None, None), b"null"), ((a, 0, 1.0, a, 1, a, a, a, None), b"n"),
                       ((a, 4096 + 64, 1.0, a, 1, a, a, a, None), b"part"), ((a, 64, 1.0, a, 0, a, a, a, None), b"part"),
                       ((a + 4, 64, 1.0, a, 1, a, a, a, None), b"aligned"), ((a, 64, float("nan"), a, 1, a, a, a, None), b"nan")):
        assert lib_built.r50_op_grad_norm(*args) == -1, args
        assert word in lib_built.r50_last_error(None), (args, lib_built.r50_last_error(None))
    ok = (a, a, a, a, a, 64, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, a, a, a, 0.1, 1, None)
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (11, 0), (16, 2)):
        bad = list(ok)
        bad[i] = v
        assert lib_built.r50_op_adamw_clip_ema(*bad) == -1, i
        assert b"r50_op_adamw_clip_ema" in lib_built.r50_last_error(None)
