"""The exact tier of tests/test_exact_lattice_gpu.py can fail, and its preconditions hold -- shown without a GPU.

* every case and regime of the GPU file: all terms on the lattice, B = sum of the absolute terms < 2^24 units (fp32 exact in any
  order), fp16 unsaturated; small regime: nothing rounded; wide regime: >= 1 % ties of each parity wherever there are 1000 outputs;
* mutants of the reference (one product removed, two K channels of the last K slice swapped, one halo tap taken from the neighbouring
  image) change at least one element in the small regime; a double rounding changes the wide regime;
* torch's CPU conversions to bf16 / fp16 / e4m3, which the references round with, send the constructed ties to even.
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
