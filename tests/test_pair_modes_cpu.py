"""The bars of tests/test_pair_modes_gpu.py can fail: every one-term defect of the fp32x / bf16w2 convolution arithmetic, restated on the
CPU in fp64 (tests/pair_reference.py), lies far outside them on the very cases the device is held to.  No device needed."""
import functools

import pytest
import torch

from tests import pair_reference as P


@functools.lru_cache(maxsize=None)
def _fp32x_case(case):
    """Split inputs of one case and the true oracle, computed once and shared (read-only)."""
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    x, wt, bias, res = P.pair_case_inputs(case)
    xp, wp = P.split_pair(x), P.split_pair(wt)
    rp = P.split_pair(res) if has_res else None
    return xp, wp, bias, rp, P.fp32x_conv(xp, wp, bias, stride, pad, relu, rp)


def test_the_bar_is_below_its_ceiling():
    assert 0.0 < P.FP32X_REL_L2_BAR <= P.FP32X_REL_L2_CEILING == 2.4e-4


@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_correct_fp32x_arithmetic_is_far_inside_the_bar(case):
    """Three products + pair store, summed exactly: what remains is the dropped tail.tail product and the 16-bit store, 3e-6 to 5e-6 --
    which is also all the device shows (its fp32 accumulation adds nothing visible at these K)."""
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xp, wp, bias, rp, true = _fp32x_case(case)
    r = P.rel_l2(P.fp32x_conv(xp, wp, bias, stride, pad, relu, rp, mutation="device"), true)
    assert r < 1e-5, r
    assert r < P.FP32X_REL_L2_BAR


_DEFECTS = [(c, m) for c in P.PAIR_CASES for m in P.MUTATIONS if m != "residual_tail" or c[9]]


@pytest.mark.parametrize("case,mutation", _DEFECTS, ids=lambda v: v if isinstance(v, str) else P.case_id(v))
def test_every_one_term_defect_of_fp32x_is_four_bars_away(case, mutation):
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xp, wp, bias, rp, true = _fp32x_case(case)
    r = P.rel_l2(P.fp32x_conv(xp, wp, bias, stride, pad, relu, rp, mutation=mutation), true)
    assert r >= 4.0 * P.FP32X_REL_L2_BAR, f"{mutation}: rel-L2 {r:.3e} is within 4 x the bar {P.FP32X_REL_L2_BAR:.1e}"


@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_bf16w2_without_the_weight_tail_fails_the_per_kernel_bar(case):
    """x . w_head alone (the bf16 conv) against the weight_terms = 2 oracle: about a fifth of the bf16 outputs move, and `_check_bf16`
    (at most 1 % may differ) must say so; the oracle against itself passes."""
    from oracle.resnet50_oracle import bf16_round, conv_bias_act_emulated
    from tests.test_kernels_gpu import _check_bf16
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    x, wt, bias, res = P.pair_case_inputs(case)
    x = bf16_round(x)
    res = bf16_round(res) if has_res else None
    true = conv_bias_act_emulated(x, wt, bias, stride, pad, relu, residual_bf=res, weight_terms=2)
    dropped = conv_bias_act_emulated(x, wt, bias, stride, pad, relu, residual_bf=res, weight_terms=1)
    _check_bf16(true.permute(0, 2, 3, 1), true, "oracle against itself")
    with pytest.raises(AssertionError):
        _check_bf16(dropped.permute(0, 2, 3, 1), true, "weight tail dropped")
    if cout * n * h * w >= 4096:       # enough elements for a stable fraction
        assert float((dropped != true).float().mean()) > 0.05


def test_split_pair_recombines_exactly_in_fp32():
    """head + tail is an fp32 number: the fp32 sum `head.float() + tail.float()` -- what the kernels' epilogues and pools, and
    `ResNet50Backbone.layer`, form -- loses nothing against the fp64 sum.  It is the fp32 value itself whenever that value has at most
    16 significand bits, and within 2^-17 of it otherwise.  Normal values across the exponent range; zero as well."""
    g = torch.Generator().manual_seed(5)
    mant = torch.randn(200000, generator=g)
    expo = torch.randint(-60, 61, (200000,), generator=g).to(torch.float32)
    v = torch.cat([mant * torch.exp2(expo), torch.tensor([0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 255.5, 3.0e38, -3.0e38, 2.0 ** -100])])
    hd, tl = P.split_pair(v)
    s32 = hd.float() + tl.float()
    assert torch.equal(s32.double(), P.pair_value(hd, tl))
    assert bool(((s32.double() - v.double()).abs() <= 2.0 ** -17 * v.double().abs()).all())
    v16 = s32                               # values that carry no more than a pair can hold
    hd2, tl2 = P.split_pair(v16)
    assert torch.equal(hd2.float() + tl2.float(), v16)


def test_pack_layouts():
    """The two packed row layouts against a direct index restatement."""
    g = torch.Generator().manual_seed(9)
    w = torch.randn((4, 6, 3, 3), generator=g)
    hd, tl = P.split_pair(w)
    p2, p3 = P.pack_ohwi_w2(w), P.pack_ohwi_split(w)
    assert tuple(p2.shape) == (4, 3, 3, 12) and tuple(p3.shape) == (4, 3, 3, 18)
    for o, c, i, j in ((0, 0, 0, 0), (3, 5, 2, 1), (2, 4, 1, 2)):
        assert p2[o, i, j, c] == hd[o, c, i, j] and p2[o, i, j, 6 + c] == tl[o, c, i, j]
        assert p3[o, i, j, c] == hd[o, c, i, j] and p3[o, i, j, 6 + c] == hd[o, c, i, j] and p3[o, i, j, 12 + c] == tl[o, c, i, j]
    assert float(tl.float().abs().max()) > 0.0
