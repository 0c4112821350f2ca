"""The exact tier of tests/test_exact_lattice_gpu.py can fail, and its preconditions hold -- shown without a GPU.

* every case and regime of the GPU file: all terms on the lattice, B = sum of the absolute terms < 2^24 units (fp32 exact in any
  order), fp16 unsaturated; small regime: nothing rounded; wide regime: >= 1 % ties of each parity wherever there are 1000 outputs;
* mutants of the reference (one product removed, two K channels of the last K slice swapped, one halo tap taken from the neighbouring
  image) change at least one element in the small regime; a double rounding changes the wide regime;
* torch's CPU conversions to bf16 / fp16 / e4m3, which the references round with, send the constructed ties to even -- on the
  subnormal grids of fp16 and e4m3 too (every multiple of 2^-27 up to 2^-14, of 2^-12 up to 2^-6), and fp16 saturates at the clamp;
* the low and high regimes (the ends of fp16 and e4m3) meet ``assert_edge_precondition`` in every case, both operand sides carry the
  subnormal values somewhere in every case list, and six mutants of the reference -- subnormal activations / weights / outputs flushed
  to zero, subnormal outputs truncated, the conversion without its clamp, the clamp at 65520 -- change every case.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.resnet50_oracle import conv_bias_act_emulated, conv_cat_emulated, elem_round
from tests import exact_lattice as L
from tests import pair_reference as P
from tests.test_head_kernels_gpu import HEAD_GEMMS, _gemm_id
from tests.test_kernels_gpu import CAT_CASES, CONV_CASES, FP8_CASES

_REG = pytest.mark.parametrize("regime", L.REGIMES)


def _hold(stages, regime, tie_floor=True, both_types=True):
    stages = stages if isinstance(stages, list) else [stages]
    if both_types:
        stages = stages + [s.as_fmt("fp16") for s in stages]
    for s in stages:
        print(regime, s.report())
    L.assert_exact_precondition(stages, regime, tie_floor=tie_floor)


@_REG
@pytest.mark.parametrize("case", CONV_CASES + [(1, 4, 4, 64, 64, 1, 1, 0, True, False)], ids=P.case_id)
def test_conv_cases_meet_the_preconditions(case, regime):
    _, st = L.conv_case(case, "bf16", regime)
    _hold(st, regime, tie_floor=st.pre.numel() >= 1000)
    if regime == "wide":
        assert float(st.pre.abs().max()) / st.unit > 2000, "the wide regime must reach values that round"


@_REG
@pytest.mark.parametrize("case", CAT_CASES, ids=str)
def test_cat_cases_meet_the_preconditions(case, regime):
    _hold(L.cat_case(case, "bf16", regime)[1], regime)


@_REG
@pytest.mark.parametrize("case", FP8_CASES, ids=str)
def test_fp8_cases_meet_the_preconditions(case, regime):
    tensors, st = L.fp8_case(case, regime)
    _hold(st, regime, both_types=False)
    sx, sw, sr, sy = tensors[4]
    assert all(math.frexp(s)[0] == 0.5 for s in (sx, sw, sr, sy)), "fp8 scales must be powers of two"
    if regime == "wide":
        sat = float((st.pre.abs() >= 448.0).float().mean())
        assert 0.0 < sat < 0.5, f"saturating share {sat}"
        dn, up = st.ties()
        assert dn > 0.0 and up > 0.0


@_REG
@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_pair_cases_meet_the_preconditions(case, regime):
    _, st = L.w2_case(case, regime)
    _hold(st, regime, tie_floor=st.pre.numel() >= 1000, both_types=False)
    sp = L.split_case(case, regime)[1]
    _hold(sp, regime, tie_floor=False, both_types=False)
    if regime == "wide" and sp.pre.numel() >= 1000:      # past 2^17 units (the head's 8 bits + 9 of the remainder) the tail plane rounds
        assert float((sp.ref.double() != sp.pre.double()).double().mean()) > 0.001


@_REG
@pytest.mark.parametrize("name", list(L.CHAIN_CASES))
def test_chain_cases_meet_the_preconditions_at_every_stage(name, regime):
    tensors, stages = L.CHAIN_CASES[name][2](regime)
    assert len(stages) >= 1 and {s.name for s in stages} <= {"t2", "identity", "out", "y1n"}
    _hold(stages, regime, both_types=False)


@_REG
@pytest.mark.parametrize("n", L.STEM_N)
def test_stem_cases_meet_the_preconditions(n, regime):
    _hold(L.stem_case(n, regime)[1], regime, both_types=False)


@_REG
@pytest.mark.parametrize("shape", HEAD_GEMMS, ids=_gemm_id)
def test_gemm_cases_meet_the_preconditions(shape, regime):
    (x, w, bias, res), st = L.gemm_case(shape, "bf16", regime)
    _hold(st, regime)
    if shape[5] == "dw":
        assert not bool(x[:, shape[6]:].any()) and not bool(w[:, shape[6]:].any()), "the dW rows keep their zero padding"
    if shape[5] != "fwd":
        assert not bool(bias.any())


@pytest.mark.parametrize("shape", L.AVGPOOL_SHAPES)
def test_avgpool_reference_is_the_exact_sum_times_the_fp32_reciprocal(shape):
    x, ref = L.avgpool_case(shape)
    n, h, w, c = shape
    s = torch.zeros((n, c), dtype=torch.float32)
    for r in range(h * w):                                   # the kernel's order: rows added one by one in fp32
        s += x.view(n, h * w, c)[:, r].float()
    assert torch.equal(s * torch.tensor(1.0 / (h * w), dtype=torch.float32), ref)


# ---- the ends of fp16 and e4m3: conditions, and mutants of the reference that every case must tell from it
_EDGE = pytest.mark.parametrize("regime", L.EDGE_REGIMES)
SIDES = ("x", "w")


def side_of(i: int) -> str:
    """The operand that carries the subnormal values of a list's i-th low case: the sides rotate over every case list."""
    return SIDES[i % 2]


def _flush(t, fmt):
    return torch.where(t.abs() < L.FORMATS[fmt].min_normal, torch.zeros_like(t), t)


def _output_mutants(st, regime):
    """What a wrong epilogue would store, from the exact value: (name, tensor)."""
    f = L.FORMATS[st.fmt]
    if regime == "low":
        sub = st.pre.abs() < f.min_normal
        trunc = torch.where(sub, torch.trunc(st.pre.double() / f.sub_step).float() * f.sub_step, st.ref)
        return [("subnormal outputs flushed to zero", _flush(st.ref, st.fmt)), ("subnormal outputs truncated toward zero", trunc)]
    return [("conversion without the clamp", st.pre.to(torch.float16).float()),
            ("clamp at 65520", st.pre.clamp(-65520.0, 65520.0).to(torch.float16).float())]


def _hold_edge(stages, regime):
    """The regime's conditions, and its two output mutants change the stage that meets them."""
    stages = stages if isinstance(stages, list) else [stages]
    for s in stages:
        print(regime, s.report())
        print(regime, s.edge_report())
    L.assert_edge_precondition(stages, regime)
    hit = [s for s in stages if regime == "high" or L.low_output_condition(s)]
    for s in hit:
        for name, mut in _output_mutants(s, regime):
            assert int((mut != s.ref).sum()) >= 1, f"{s.name}: {name} went unnoticed"
        if regime == "high":
            assert bool(torch.isinf(_output_mutants(s, regime)[0][1]).any()) and bool(torch.isinf(_output_mutants(s, regime)[1][1]).any())
    assert hit


@_EDGE
@pytest.mark.parametrize("i", range(len(CONV_CASES) + 1))
def test_conv_cases_meet_the_edge_conditions(i, regime):
    case = (CONV_CASES + [(1, 4, 4, 64, 64, 1, 1, 0, True, False)])[i]
    (x, wt, bias, res), st = L.conv_case(case, "fp16", regime, side_of(i))
    _hold_edge(st, regime)
    assert L.representable(x, "fp16") and L.representable(wt, "fp16") and (res is None or L.representable(res, "fp16"))
    if regime == "low":       # the operands are the wide regime's integers at other units
        (xw, ww, _, _), _ = L.conv_case(case, "fp16", "wide")
        un = L.units_of("low", "fp16", side_of(i))
        assert torch.equal(x / un.ux, xw / L.UX) and torch.equal(wt / un.uw, ww / L.UW)


@_EDGE
@pytest.mark.parametrize("i", range(len(CAT_CASES)))
def test_cat_cases_meet_the_edge_conditions(i, regime):
    _hold_edge(L.cat_case(CAT_CASES[i], "fp16", regime, side_of(i))[1], regime)


@pytest.mark.parametrize("case", FP8_CASES, ids=str)
def test_fp8_cases_meet_the_low_conditions(case):
    tensors, st = L.fp8_case(case, "low")
    _hold_edge(st, "low")
    xq, wq, bias, rq, (sx, sw, sr, sy) = tensors
    assert all(math.frexp(s)[0] == 0.5 for s in (sx, sw, sr, sy)), "fp8 scales must be powers of two"
    for t in (xq, wq) + (() if rq is None else (rq,)):       # nonzero values on both sides of 2^-6, all on 2^-9
        a = t.float().abs()
        assert bool(((a > 0) & (a < 2.0 ** -6)).any()) and bool((a >= 2.0 ** -6).any()) and bool((a * 512 == (a * 512).round()).all())
    a = st.pre.abs()
    assert bool(((a > 0) & (a < 2.0 ** -6)).any()) and bool((a >= 2.0 ** -6).any()) and float(st.ref.abs().max()) > 1.0


@_EDGE
@pytest.mark.parametrize("i", range(len(HEAD_GEMMS)))
def test_gemm_cases_meet_the_edge_conditions(i, regime):
    _hold_edge(L.gemm_case(HEAD_GEMMS[i], "fp16", regime, side=side_of(i))[1], regime)


@pytest.mark.parametrize("name", L.LOW_CHAINS)
def test_chain_cases_meet_the_low_conditions(name):
    """fp16: the chain's inputs are normal, every stored intermediate is subnormal and meets the output condition, and the stage that
    re-reads it names it as the operand that carries the subnormal values."""
    tensors, stages = L.CHAIN_CASES[name][2]("low", "fp16")
    _hold_edge(stages, "low")
    for t in tensors:
        if t is not None and t.dtype == torch.float16:
            a = t.float().abs()
            assert bool(torch.isfinite(a).all())
    first = stages[0]
    assert not first.operands or first.name == "out"          # a first stage's only subnormal operand is a stored identity
    assert all(L.low_output_condition(s) for s in stages), [s.edge_report() for s in stages]
    assert set(L.LOW_CHAINS) <= set(L.CHAIN_CASES)
    assert {L.CHAIN_CASES[n][0] for n in L.LOW_CHAINS} == {L.CHAIN_CASES[n][0] for n in L.CHAIN_CASES}, "a fused kernel has no low case"


@pytest.mark.parametrize("regime,side", [("low", "x"), ("low", "w"), ("high", "x")])
def test_stem_case_meets_the_edge_conditions(regime, side):
    _hold_edge(L.stem_case(1, regime, "fp16", side)[1], regime)


@pytest.mark.parametrize("shape", L.AVGPOOL_SHAPES)
def test_avgpool_low_reference_is_the_exact_sum_of_subnormal_addends(shape):
    x, ref = L.avgpool_case(shape, "fp16", 2.0 ** -24)
    n, h, w, c = shape
    a = x.float().abs()
    assert x.dtype == torch.float16 and bool((a[a > 0] < 2.0 ** -14).all()) and float((a > 0).float().mean()) > 0.9
    s = torch.zeros((n, c), dtype=torch.float32)
    for r in range(h * w):                                   # the kernel's order: rows added one by one in fp32
        s += x.view(n, h * w, c)[:, r].float()
    assert torch.equal(s * torch.tensor(1.0 / (h * w), dtype=torch.float32), ref)


def test_both_operand_sides_carry_the_subnormal_values_in_every_case_list():
    for cases in (CONV_CASES, CAT_CASES, HEAD_GEMMS):
        assert {side_of(i) for i in range(len(cases))} == set(SIDES)


def test_no_edge_regime_for_bf16():
    for regime in L.EDGE_REGIMES:
        with pytest.raises(ValueError):
            L.conv_case(CONV_CASES[0], "bf16", regime)


def _conv_ref(x, w, bias, res, case, fmt="fp16"):
    n, h, wd, cin, cout, k, stride, pad, relu, has_res = case
    return conv_bias_act_emulated(x, w, bias, stride, pad, relu, residual_bf=res, fmt=fmt)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("case", CONV_CASES, ids=P.case_id)
def test_mutant_subnormal_operands_flushed_before_the_product(case, side):
    """Activations (side x) or weights (side w) below 2^-14 read as zero, what an MFMA that flushes its f16 inputs would do."""
    (x, wt, bias, res), st = L.conv_case(case, "fp16", "low", side)
    mut = _conv_ref(_flush(x, "fp16"), wt, bias, res, case) if side == "x" else _conv_ref(x, _flush(wt, "fp16"), bias, res, case)
    assert int((mut != st.ref).sum()) >= 1, f"flushed subnormal {side} operands went unnoticed"


@pytest.mark.parametrize("which", ["x", "w"])
@pytest.mark.parametrize("case", FP8_CASES, ids=str)
def test_mutant_subnormal_fp8_operands_flushed_before_the_product(case, which):
    from tests.kernel_cases import fp8_reference
    n, h, w, cin, cout, k, stride, pad, relu, has_res, _tile = case
    (xq, wq, bias, rq, scales), st = L.fp8_case(case, "low")
    xq, wq = xq.float(), wq.float()
    xq, wq = (_flush(xq, "e4m3"), wq) if which == "x" else (xq, _flush(wq, "e4m3"))
    mut = L.fp8_round(fp8_reference(xq, wq, bias, rq, scales, stride, pad, bool(relu)))
    assert int((mut != st.ref).sum()) >= 1, f"flushed subnormal fp8 {which} operands went unnoticed"


# ---- the references are the oracle's own functions
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("idx", [1, 3, 4, 13])
def test_rounding_the_unrounded_value_is_the_oracles_fused_op(idx, fmt):
    case = CONV_CASES[idx]
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    (x, wt, bias, res), st = L.conv_case(case, fmt, "wide")
    assert torch.equal(st.ref, conv_bias_act_emulated(x, wt, bias, stride, pad, relu, residual_bf=res, fmt=fmt))


@pytest.mark.parametrize("idx", [0, 4])
def test_cat_reference_is_conv_cat_emulated(idx):
    case = CAT_CASES[idx]
    n, h, c1, h2, c2, s2, cout, relu, _tile = case
    (x1, x2, wcat, bias), st = L.cat_case(case, "bf16", "wide")
    nchw = lambda t: t.float().permute(0, 3, 1, 2)         # noqa: E731
    w = wcat.float()
    ref = conv_cat_emulated(nchw(x1), w[:, :c1].reshape(cout, c1, 1, 1), bias, nchw(x2), w[:, c1:].reshape(cout, c2, 1, 1),
                            torch.zeros(cout), s2)
    assert torch.equal(st.ref, ref)


# ---- mutants: what a kernel with one defect would compute
def _mutant_inputs(which):
    """(x, w, bias, res, stride, pad, relu) of a small-regime case as one conv: CONV_CASES rows, or a two-source row over its
    concatenated K = [x1 | x2 at stride2]."""
    if which[0] == "cat":
        case = CAT_CASES[which[1]]
        n, h, c1, h2, c2, s2, cout, relu, _tile = case
        (x1, x2, wcat, bias), _ = L.cat_case(case, "bf16", "small")
        x = torch.cat([x1.float().permute(0, 3, 1, 2), x2.float().permute(0, 3, 1, 2)[:, :, ::s2, ::s2]], 1)
        return x, wcat.float().view(cout, c1 + c2, 1, 1), bias, None, 1, 0, bool(relu)
    case = CONV_CASES[which[1]]
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    (x, wt, bias, res), _ = L.conv_case(case, "bf16", "small")
    return x, wt, bias, res, stride, pad, relu


MUTANT_CASES = [("conv", 3), ("conv", 4), ("conv", 1), ("conv", 10), ("cat", 0), ("cat", 4)]    # 3x3 padded; 3x3 stride 2; residual; two sources


def _true(x, w, bias, res, stride, pad, relu):
    return conv_bias_act_emulated(x, w, bias, stride, pad, relu, residual_bf=res)


@pytest.mark.parametrize("which", MUTANT_CASES, ids=str)
def test_mutant_one_product_removed(which):
    x, w, bias, res, stride, pad, relu = _mutant_inputs(which)
    ref = _true(x, w, bias, res, stride, pad, relu)
    lin = conv_bias_act_emulated(x, w, bias, stride, pad, False, residual_bf=res, fmt="fp32")
    n0, co, oy, ox = (int(v) for v in (lin == lin.max()).nonzero()[0])
    assert float(lin[n0, co, oy, ox]) > 0
    k = w.shape[2]
    prod = None
    for ky in range(k):
        for kx in range(k):
            iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
            if 0 <= iy < x.shape[2] and 0 <= ix < x.shape[3]:
                p = x[n0, :, iy, ix].double() * w[co, :, ky, kx].double()
                if bool(p.any()) and prod is None:
                    prod = float(p[p != 0][0])
    assert prod is not None
    mut = lin.clone()
    mut[n0, co, oy, ox] -= prod
    mut = elem_round(F.relu(mut) if relu else mut, "bf16")
    assert int((mut != ref).sum()) >= 1, "a missing non-zero product went unnoticed"


@pytest.mark.parametrize("which", MUTANT_CASES, ids=str)
def test_mutant_two_k_channels_of_the_last_slice_swapped(which):
    x, w, bias, res, stride, pad, relu = _mutant_inputs(which)
    ref = _true(x, w, bias, res, stride, pad, relu)
    cin, k = w.shape[1], w.shape[2]
    wm = w.clone()
    wm[:, [cin - 1, cin - 2], k - 1, k - 1] = w[:, [cin - 2, cin - 1], k - 1, k - 1]
    assert int((_true(x, wm, bias, res, stride, pad, relu) != ref).sum()) >= 1, "a swap of two K slots went unnoticed"


@pytest.mark.parametrize("which", [m for m in MUTANT_CASES if m[0] == "conv" and CONV_CASES[m[1]][5] == 3], ids=str)
def test_mutant_one_halo_tap_from_the_neighbouring_image(which):
    x, w, bias, res, stride, pad, relu = _mutant_inputs(which)
    ref = _true(x, w, bias, res, stride, pad, relu)
    assert x.shape[0] >= 2 and pad == 1
    xp = F.pad(x, (1, 1, 1, 1))
    xp[1, :, 0, 1] = x[0, :, -1, 0]                          # the top-left halo pixel of image 1 read from image 0's last row
    mut = _true(xp, w, bias, res, stride, 0, relu)
    assert mut.shape == ref.shape and int((mut != ref).sum()) >= 1, "a halo tap from the wrong image went unnoticed"


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("idx", [1, 5, 10])
def test_double_rounding_differs_in_the_wide_regime(idx, fmt):
    case = CONV_CASES[idx]
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    assert has_res
    (x, wt, bias, res), st = L.conv_case(case, fmt, "wide")
    acc16 = conv_bias_act_emulated(x, wt, bias, stride, pad, False, fmt=fmt)          # the accumulator rounded before the residual add
    twice = elem_round(F.relu(acc16.double() + res.double()).float(), fmt)
    assert int((twice != st.ref).sum()) >= 1, "a double rounding went unnoticed"


# ---- torch's conversions round the constructed ties to even
@pytest.mark.parametrize("fmt", ["bf16", "fp16", "e4m3"])
def test_cpu_conversions_round_ties_to_even(fmt):
    st = L.fp8_case(FP8_CASES[2], "wide")[1] if fmt == "e4m3" else L.conv_case(CONV_CASES[2], fmt, "wide")[1]      # no ReLU: both signs
    f = L.FORMATS[fmt]
    a = st.pre.abs()
    ok = (a >= f.min_normal) & (a < f.max_finite)
    pre = st.pre[ok]
    dn, up = L.tie_shares(pre, fmt)
    assert dn > 0.005 and up > 0.005, (dn, up)
    got = pre.to(f.dtype).to(torch.float32)
    want = L.rne_by_integer_arithmetic(pre, fmt)
    assert torch.equal(got, want)
    assert torch.equal(L.round_to(pre, fmt), want)
    bits = pre.contiguous().view(torch.int32) & 0x7FFFFFFF
    tie = (bits & ((1 << f.drop) - 1)) == (1 << (f.drop - 1))
    kept = got.view(torch.int32)[tie]
    assert int(tie.sum()) > 0 and not bool(((kept >> f.drop) & 1).any()), "a tie went to an odd neighbour"
    assert bool((pre[tie] < 0).any()) and bool((pre[tie] > 0).any())
    if fmt != "bf16":                    # the bottom of the format: the whole subnormal grid; fp16: the clamp at the top
        _conversions_round_the_subnormal_grid_to_even(fmt, {"fp16": 2.0 ** -27, "e4m3": 2.0 ** -12}[fmt])
    if fmt == "fp16":
        _conversion_to_fp16_saturates_at_the_clamp()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _conversions_round_the_subnormal_grid_to_even(fmt, fine):
    """Every multiple of 2^-27 up to 2^-14 (fp16) / of 2^-12 up to 2^-6 (e4m3), both signs, and values below half the smallest
    subnormal: torch's conversion and ``round_to`` agree with the integer arithmetic on the bit pattern, sign of zero included, and
    with plain integer rounding of the quotient by the grid step; the ties go to the even multiple."""
    f = L.FORMATS[fmt]
    k = torch.arange(0, int(f.min_normal / fine) + 1, dtype=torch.float64)
    mag = torch.cat([k * fine, torch.tensor([f.sub_step / 2, f.sub_step / 2 * (1 - 2.0 ** -20), f.sub_step / 2 * (1 + 2.0 ** -20), f.sub_step * 2.0 ** -40,
                                             f.min_normal * (1 - 2.0 ** -20), f.min_normal * (1 + 2.0 ** -20)], dtype=torch.float64)])
    pre = torch.cat([mag, -mag]).to(torch.float32)
    assert bool((pre.double() == torch.cat([mag, -mag])).all())
    want = L.rne_by_integer_arithmetic(pre, fmt)
    got = pre.to(f.dtype).to(torch.float32)
    assert _same_bits(got, want), L.describe_mismatch(got, L.Exact("grid", pre, want, 0.0, fine, fmt))
    assert _same_bits(L.round_to(pre, fmt), want)
    q = pre[: k.numel()].double() / f.sub_step                       # the plain statement of the same rounding, on the enumerated part
    fl = q.floor()
    rne = torch.where(q - fl > 0.5, fl + 1, torch.where(q - fl < 0.5, fl, fl + fl.remainder(2.0)))
    assert torch.equal(want[: k.numel()].double(), rne * f.sub_step)
    dn, up = L.tie_shares(pre, fmt, "subnormal")
    assert dn > 0.05 and up > 0.05 and L.tie_shares(pre[pre.abs() < f.min_normal], fmt) == (0.0, 0.0)
    tie = (q - fl == 0.5)
    assert int(tie.sum()) == (1024 if fmt == "fp16" else 8) and bool((want[: k.numel()][tie].double() / f.sub_step).remainder(2.0).eq(0).all())


def _conversion_to_fp16_saturates_at_the_clamp():
    """``round_to`` (clamp, then convert) and the integer arithmetic give +-65504 from 65504 upward, infinity included; the values
    the high regime plants are among them; the unclamped conversion makes an infinity from 65520 on."""
    mag = torch.tensor([65472.0, 65488.0, 65503.99, 65504.0, 65504.01, 65512.0, 65519.996, 65520.0, 65528.0, 65536.0, 1e5, 3e38, float("inf")])
    pre = torch.cat([mag, -mag])
    want = L.rne_by_integer_arithmetic(pre, "fp16")
    assert _same_bits(L.round_to(pre, "fp16"), want)
    assert torch.equal(want[:3], torch.tensor([65472.0, 65472.0, 65504.0])) and bool((want[3:13] == 65504.0).all()) and bool((want[16:] == -65504.0).all())
    raw = pre.to(torch.float16).float()
    assert bool(torch.isfinite(raw[:7]).all()) and bool(torch.isinf(raw[7:13]).all())
    for v in L.HIGH_PLANTS:
        assert v in mag.tolist()
    w8 = L.rne_by_integer_arithmetic(torch.tensor([447.0, 448.0, 463.9, 464.0, 480.0, 1e4, -464.0]), "e4m3")
    assert torch.equal(w8, torch.tensor([448.0, 448.0, 448.0, 448.0, 448.0, 448.0, -448.0]))
    assert torch.equal(L.round_to(torch.tensor([447.0, 464.0, -464.0, 1e4]), "e4m3"), torch.tensor([448.0, 448.0, -448.0, 448.0]))
