"""Reference arithmetic of the two (head, tail) pair precisions, plain torch on the CPU in fp64 -- test infrastructure only.

fp32x:  every value v travels as head = bf16(v), tail = bf16(v - head); a conv runs the three bf16 products x_head.w_head +
        x_tail.w_head + x_head.w_tail with fp32 accumulation (the x_tail.w_tail product, < 2^-17 relative, is dropped) and stores the
        pair of the fp32 result.
bf16w2: bf16 activations, weights as pairs: x.w_head + x.w_tail in one fp32 accumulator, one bf16 rounding
        (oracle: ``conv_bias_act_emulated(..., weight_terms=2)``).

The true fp32x oracle is the exact conv of the pair VALUES; ``fp32x_conv`` can also leave out single terms, which is how
tests/test_pair_modes_cpu.py shows that the bars of tests/test_pair_modes_gpu.py can fail.
"""
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

# Rel-L2 bar of one fp32x conv launch against the fp64 oracle: 4 x the worst distance measured with the correct kernels on an MI355X over
# the op-level cases and the network's 53 launches (tests/test_pair_modes_gpu.py, profiles/pair_modes_accuracy.txt).
FP32X_WORST_MEASURED = 4.481e-6
FP32X_REL_L2_BAR = 4.0 * FP32X_WORST_MEASURED
# A quarter of the smallest distance of a one-term mutation (9.6e-4, the residual's tail): the bar may never exceed this.
FP32X_REL_L2_CEILING = 2.4e-4

# The CONV_CASES rows of tests/test_kernels_gpu.py the pair modes are held to at op level:
# n, h, w, cin, cout, k, stride, pad, relu, residual
PAIR_CASES = [
    (3, 5, 5, 64, 256, 1, 1, 0, True, True),       # M = 75: ragged pixel tail, residual epilogue
    (1, 1, 1, 64, 64, 3, 1, 1, True, False),       # single pixel: every tap but the centre is padding; 64-cout tile
    (2, 9, 9, 128, 128, 3, 2, 1, True, False),     # 3x3 stride 2, odd size
    (3, 5, 9, 128, 256, 3, 1, 1, True, True),      # non-square, halo rows cross image borders, residual
    (2, 7, 7, 512, 512, 3, 1, 1, True, False),     # K = 4608 (x2 / x3 in the pair modes)
    (2, 7, 7, 2048, 512, 1, 1, 0, True, False),    # K = 2048
    (2, 8, 8, 256, 512, 1, 2, 0, False, False),    # strided 1x1, no ReLU (negative outputs)
]

MUTATIONS = ("x_tail_w_head", "x_head_w_tail", "residual_tail", "output_tail")


def case_id(c) -> str:
    return "n%d_%dx%d_c%d-%d_k%ds%dp%d_r%d_res%d" % tuple(int(v) for v in c)


def split_pair(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 values -> (head, tail) bf16: head = bf16(t), tail = bf16(fp32(t) - head), both round-to-nearest-even.  The subtraction
    is exact in fp32 (head keeps the leading 8 bits of t)."""
    t = t.to(torch.float32)
    head = t.to(torch.bfloat16)
    tail = (t - head.to(torch.float32)).to(torch.bfloat16)
    return head, tail


def pair_value(head: torch.Tensor, tail: torch.Tensor) -> torch.Tensor:
    """The value a pair stands for, in fp64."""
    return head.to(torch.float64) + tail.to(torch.float64)


def nhwc_pair(head_nchw: torch.Tensor, tail_nchw: torch.Tensor) -> torch.Tensor:
    """Two NCHW planes -> the device's activation layout (N,H,W,[head(C) | tail(C)])."""
    return torch.cat([head_nchw.permute(0, 2, 3, 1), tail_nchw.permute(0, 2, 3, 1)], dim=3).contiguous()


def unpair_nhwc(t_nhwc: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The device's (N,H,W,2C) pair tensor -> (head, tail) NCHW planes."""
    c = t_nhwc.shape[3] // 2
    return t_nhwc[..., :c].permute(0, 3, 1, 2).contiguous(), t_nhwc[..., c:].permute(0, 3, 1, 2).contiguous()


def pack_ohwi_w2(w_oihw_f32: torch.Tensor) -> torch.Tensor:
    """(cout,cin,k,k) fp32 -> (cout,k,k,[w_head(cin) | w_tail(cin)]) bf16: the packed rows of bf16w2 mode."""
    hd, tl = split_pair(w_oihw_f32)
    return torch.cat([hd.permute(0, 2, 3, 1), tl.permute(0, 2, 3, 1)], dim=3).contiguous()


def pack_ohwi_split(w_oihw_f32: torch.Tensor) -> torch.Tensor:
    """(cout,cin,k,k) fp32 -> (cout,k,k,[w_head | w_head | w_tail]) bf16: the packed rows of fp32x mode (pairs with
    X = [x_head | x_tail | x_head])."""
    hd, tl = split_pair(w_oihw_f32)
    hd, tl = hd.permute(0, 2, 3, 1), tl.permute(0, 2, 3, 1)
    return torch.cat([hd, hd, tl], dim=3).contiguous()


def fp32x_conv(x_pair, w_pair, bias_f32: torch.Tensor, stride: int, pad: int, relu: bool, res_pair=None,
               mutation: Optional[str] = None) -> torch.Tensor:
    """``y = act(conv(x_head + x_tail, w_head + w_tail) + bias [+ r_head + r_tail])`` in fp64 (NCHW in, NCHW fp64 out): the exact conv of
    the pair values, the oracle of one fp32x launch.  x_pair / w_pair / res_pair: (head, tail) tensors of bf16-representable values.

    ``mutation="device"``: the device's arithmetic summed exactly -- three products (no x_tail.w_tail), the result rounded to fp32 and
    stored as a pair.  Any of MUTATIONS: what a kernel with ONE defect would compute instead of that -- "x_tail_w_head" /
    "x_head_w_tail": that product missing; "residual_tail": the residual read as its head only; "output_tail": only the head of the
    result stored."""
    if mutation is not None and mutation != "device" and mutation not in MUTATIONS:
        raise ValueError(mutation)
    f64 = torch.float64
    xh, xt = (t.to(f64) for t in x_pair)
    wh, wt = (t.to(f64) for t in w_pair)

    def conv(a, b):
        return F.conv2d(a, b, stride=stride, padding=pad)

    if mutation is None:
        y = conv(xh + xt, wh + wt)
    else:
        y = conv(xh, wh)
        if mutation != "x_tail_w_head":
            y = y + conv(xt, wh)
        if mutation != "x_head_w_tail":
            y = y + conv(xh, wt)
    y = y + bias_f32.to(f64).view(1, -1, 1, 1)
    if res_pair is not None:
        y = y + res_pair[0].to(f64)
        if mutation != "residual_tail":
            y = y + res_pair[1].to(f64)
    if relu:
        y = F.relu(y)
    if mutation is not None:
        hd, tl = split_pair(y.to(torch.float32))
        y = hd.to(f64) if mutation == "output_tail" else pair_value(hd, tl)
    return y


def pair_case_inputs(case):
    """Seeded fp32 inputs of one PAIR_CASES row, NCHW / OIHW on the CPU, drawn exactly as ``_conv_inputs`` of tests/test_kernels_gpu.py
    draws them (same seed, order and scales) but kept in fp32, so that every tail plane is populated: (x, w, bias, residual or None)."""
    n, h, w, cin, cout, k, stride, pad, _relu, has_res = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn((n, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    ho = (h + 2 * pad - k) // stride + 1
    wo = (w + 2 * pad - k) // stride + 1
    res = torch.randn((n, cout, ho, wo), generator=g) if has_res else None
    return x, wt, bias, res


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
