"""Plain fp64 references and error bars for the lifting head's kernels (tests/test_head_kernels_gpu.py).  CPU only: everything here takes
and returns CPU tensors, computes in fp64 on the 16-bit values the device reads, and rounds to 16 bits once where the device stores.

et: 0 = bf16, 1 = fp16 (IEEE half), the element codes of the C ABI."""
from __future__ import annotations

import torch
import torch.nn.functional as F

DTYPE = {0: torch.bfloat16, 1: torch.float16}
MANT = {0: 7, 1: 10}                    # explicit significand bits
MIN_EXP = {0: -126, 1: -14}             # exponent of the smallest normal
FP16_MAX = 65504.0
U32 = 2.0 ** -24                        # unit roundoff of fp32


def round16(x: torch.Tensor, et: int) -> torch.Tensor:
    """Round to nearest even into the 16-bit type, as the device stores: fp16 saturates at +-65504 (the conversion of this library never
    makes an infinity out of a finite value), bf16 keeps IEEE behaviour.  NaN stays NaN here; what the device makes of NaN is tested apart."""
    x = x.double()
    if et == 1:
        x = torch.where(torch.isnan(x), x, x.clamp(-FP16_MAX, FP16_MAX))
    return x.to(DTYPE[et])


def ulp16(x: torch.Tensor, et: int) -> torch.Tensor:
    """Spacing of the 16-bit type at |x| (fp64): 2^(e - mantissa bits) for 2^e <= |x| < 2^(e+1), the subnormal spacing below."""
    a = x.double().abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** MIN_EXP[et]))).clamp_min(MIN_EXP[et])
    return torch.pow(2.0, e - MANT[et])


def causal3_rows(y: torch.Tensor) -> torch.Tensor:
    """y (b, t, c) -> the causal conv's input rows (b, t, 3c): row t = [y(t-2) | y(t-1) | y(t)], indices clamped at 0."""
    t = y.shape[1]
    idx = (torch.arange(t).view(t, 1) + torch.arange(-2, 1).view(1, 3)).clamp_min(0)      # (t, 3)
    return y[:, idx, :].reshape(y.shape[0], t, 3 * y.shape[2])


def gn_relu(x: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """ReLU(GroupNorm) over x (b, t, c) in x's own dtype: statistics per (sample, group) over the (c/groups x t) slab."""
    return F.relu(F.group_norm(x.permute(0, 2, 1), groups, gamma.to(x.dtype), beta.to(x.dtype), eps)).permute(0, 2, 1)


def gn_forward_bar(x16: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """fp64 rows (b, t, 3c) of ReLU(GroupNorm(x16)) and the absolute term of the bar: 4 x the largest deviation of torch's own fp32
    F.group_norm from fp64 on the same input, floored at 2^-20 max|ref| -- no worse than the reference's own arithmetic."""
    ref = causal3_rows(gn_relu(x16.double(), groups, gamma, beta, eps))
    t32 = causal3_rows(gn_relu(x16.float(), groups, gamma, beta, eps)).double()
    return ref, max(4.0 * float((t32 - ref).abs().max()), 2.0 ** -20 * float(ref.abs().max()))


def assert_within_rounding(got16: torch.Tensor, ref: torch.Tensor, et: int, abs_term: float, what: str) -> None:
    """|got - ref| <= half a 16-bit ulp (at the larger of the two magnitudes: one rounding of a value that may sit on the other side of a
    binade edge) + abs_term, element-wise; got is the device's 16-bit result, ref fp64."""
    got = got16.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    diff = (got - ref).abs()
    bar = 0.5 * ulp16(torch.maximum(got.abs(), ref.abs()), et) + abs_term
    bad = diff > bar
    if bool(bad.any()):
        i = int(torch.argmax((diff - bar).flatten()))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond one rounding + {abs_term:.3g}; worst at flat "
                             f"index {i}: got {float(got.flatten()[i])!r}, fp64 {float(ref.flatten()[i])!r}")


def gn_relu_ambiguous(x16: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, margin: float) -> torch.Tensor:
    """(b, t, c) bool: elements whose fp64 pre-activation lies within `margin` of 0, where an fp32 ReLU mask may differ from fp64's."""
    pre = F.group_norm(x16.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    return pre.abs() < margin


def causal3_sources(t: int):
    """For each row r and tap k of the causal rows, the frame it reads: max(r - 2 + k, 0).  (t, 3) long."""
    return (torch.arange(t).view(t, 1) + torch.arange(-2, 1).view(1, 3)).clamp_min(0)


def zero_taps_of(dr: torch.Tensor, frames_mask: torch.Tensor) -> torch.Tensor:
    """dr (b, t, 3c) with every (row, tap) entry that reads a masked (b, frame, c) element zeroed, so that element's gradient is 0 whatever
    ReLU mask is applied to it."""
    b, t, c = frames_mask.shape
    src = causal3_sources(t)                                         # (t, 3)
    m = frames_mask[:, src, :]                                       # (b, t, 3, c)
    return torch.where(m.reshape(b, t, 3 * c), torch.zeros((), dtype=dr.dtype), dr)


def gn_backward(x: torch.Tensor, dr: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """Autograd of the causal rows of ReLU(GroupNorm(x)) in x's dtype: dx (b, t, c) and the per-sample parameter parts (b, c) that the
    device writes: dgamma_part = sum_t dy * xh, dbeta_part = sum_t dy with dy the gradient reaching the GroupNorm output."""
    xr = x.clone().requires_grad_(True)
    xh = F.group_norm(xr.permute(0, 2, 1), groups, eps=eps).permute(0, 2, 1)          # (b, t, c)
    pre = xh * gamma.to(x.dtype) + beta.to(x.dtype)
    pre.retain_grad()
    rows = causal3_rows(F.relu(pre))
    (rows * dr.to(x.dtype)).sum().backward()
    dy = pre.grad
    return xr.grad, (dy * xh.detach()).sum(1), dy.sum(1)


def bar_from(dev32: torch.Tensor, ref: torch.Tensor) -> float:
    """4 x the largest deviation of an fp32 computation from fp64, floored at 2^-20 max|ref|."""
    return max(4.0 * float((dev32.double() - ref).abs().max()), 2.0 ** -20 * float(ref.abs().max()))


def gemm_ref(x16: torch.Tensor, w16: torch.Tensor, bias: torch.Tensor, residual16, relu: bool) -> torch.Tensor:
    """fp64 (rows, cout) = x (rows, K) @ w (cout, K)^T + bias [+ residual] [ReLU], on whatever device the operands are."""
    y = x16.double() @ w16.double().t() + bias.double()
    if residual16 is not None:
        y = y + residual16.double()
    return F.relu(y) if relu else y


def adamw_ref(p0, m0, v0, g, step: int, lr: float, b1: float, b2: float, eps: float, wd: float):
    """torch.optim.AdamW in fp64 from the state (p0, m0, v0) after step - 1 steps: (p, m, v) after `step`.  The hyper-parameters are
    passed through fp32 first: the device receives them as floats."""
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))      # noqa: E731
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps), weight_decay=f(wd))
    if step > 1:
        opt.state[p] = {"step": torch.tensor(float(step - 1), dtype=torch.float64), "exp_avg": m0.double().clone(),
                        "exp_avg_sq": v0.double().clone()}
    p.grad = g.double().clone()
    opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]
