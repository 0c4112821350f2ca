"""Integer-lattice operands for the matrix-core kernels, and their fp64 references -- test infrastructure only, no GPU needed.

Every operand is ``integer x 2^e`` and exactly representable in its type.  When, for every output, the sum of the absolute values of all
terms (products, bias, residual) stays below 2^24 lattice units, every partial sum of any subset of the terms in any order is a multiple
of the unit below 2^24: exact in fp32.  The accumulation order then does not matter, and the device must agree with the fp64 reference
bit for bit after the single rounding of its epilogue.  ``assert_exact_precondition`` checks that bound; nothing here tolerates anything.

Two regimes per case:
  small  every output (and every intermediate of a chain) is itself representable in the stored type: nothing is rounded, so a missing,
         doubled or misplaced non-zero product changes the output's bits.
  wide   outputs of a few thousand units: the epilogue rounds, and a few per cent of the outputs sit exactly halfway between two
         representable values.  ``tie_shares`` counts them by the parity of the neighbour of smaller magnitude: "down" ties (that
         neighbour is even: round-to-nearest-even keeps it, round-half-away would not) and "up" ties (it is odd: truncation would keep it).

The references are the project's own formulations: ``conv_bias_act_emulated`` / ``conv_cat_emulated`` (oracle/resnet50_oracle.py),
``fp8_reference`` (tests/test_kernels_gpu.py), tests/pair_reference.py and ``gemm_ref`` (tests/head_kernels_reference.py); chains apply
them stage by stage from the inputs, with the 16-bit rounding of each intermediate the kernels store.
"""
import math
import zlib
from dataclasses import dataclass
from typing import List, Optional

import torch

from oracle.resnet50_oracle import conv_bias_act_emulated, conv_cat_emulated, elem_round, fp8_round

REGIMES = ("small", "wide")
LIMIT = 2.0 ** 24


@dataclass(frozen=True)
class Fmt:
    dtype: torch.dtype
    max_int: int          # integers up to this are exact in the type
    drop: int             # fp32 significand bits the type drops
    min_normal: float
    max_finite: float


FORMATS = {
    "bf16": Fmt(torch.bfloat16, 256, 16, 2.0 ** -126, math.inf),
    "fp16": Fmt(torch.float16, 2048, 13, 2.0 ** -14, 65504.0),
    "e4m3": Fmt(torch.float8_e4m3fn, 16, 20, 2.0 ** -6, 448.0),
}

# per regime: std of the outputs a case aims at (lattice units), the same for a chain's intermediates, bias range, residual range
TARGET = {"small": 20.0, "wide": 4000.0}
INTER = {"small": 3.0, "wide": 300.0}
LAST = {"small": 40.0, "wide": 4000.0}
BIAS_R = {"small": 8, "wide": 500}
RES_R = {"small": 16, "wide": 255}
UX, UW = 2.0 ** -2, 2.0 ** -3        # units of activations and weights; a conv's outputs, bias and residual are in UX * UW


def seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def round_to(t: torch.Tensor, fmt: str) -> torch.Tensor:
    """The stored value of t in the type (round to nearest even, fp16 / e4m3 saturating), as fp32."""
    if fmt == "e4m3":
        return fp8_round(t)
    return elem_round(t.to(torch.float32), fmt)


def representable(t: torch.Tensor, fmt: str) -> bool:
    return bool((round_to(t, fmt).double() == t.double()).all())


def lattice(shape, r: int, gen: torch.Generator, density: Optional[float] = None, unit: float = 1.0, fmt: str = "bf16",
            nonneg: bool = False) -> torch.Tensor:
    """Seeded ``integer * unit`` values as fp32: integers uniform in [-r, r]; with ``density`` (the share of non-zeros) the non-zeros
    are uniform in [-r, r] without 0.  ``unit`` is a power of two; every value is exact in ``fmt`` (|integer| <= 256 / 2048 / 16)."""
    f = FORMATS[fmt]
    if r > f.max_int or math.frexp(unit)[0] != 0.5:
        raise ValueError(f"lattice: r {r} / unit {unit} not exact in {fmt}")
    shape = tuple(shape)
    if density is None:
        v = torch.randint(-r, r + 1, shape, generator=gen)
    else:
        mag = torch.randint(1, r + 1, shape, generator=gen)
        sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
        v = mag * sign * (torch.rand(shape, generator=gen) < density)
    if nonneg:
        v = v.abs()
    t = v.to(torch.float32) * unit
    assert representable(t, fmt)
    return t


def spread(sigma: float):
    """(r, density) of a lattice draw with standard deviation ~ sigma: uniform integers in [-r, r] (variance r (r + 1) / 3) from
    sigma = 1 up, below that -1 / 0 / 1 with density sigma^2."""
    if sigma >= 1.0:
        return max(1, int(round(math.sqrt(3.0 * sigma * sigma + 0.25) - 0.5))), None
    return 1, max(sigma * sigma, 1e-4)


def draw(shape, sigma: float, gen, unit=1.0, fmt="bf16", nonneg=False) -> torch.Tensor:
    r, density = spread(sigma)
    return lattice(shape, min(r, FORMATS[fmt].max_int), gen, density, unit, fmt, nonneg)


def tie_shares(pre: torch.Tensor, fmt: str):
    """Shares of the elements of ``pre`` (exact fp32 values before the rounding to ``fmt``) that sit exactly halfway between two
    neighbours of the type: (down, up) by the parity of the neighbour of smaller magnitude (even, odd)."""
    f = FORMATS[fmt]
    p = pre.to(torch.float32).contiguous()
    assert bool((p.double() == pre.double()).all()), "tie_shares: not an fp32 value"
    bits = p.view(torch.int32) & 0x7FFFFFFF
    a = p.abs()
    tie = ((bits & ((1 << f.drop) - 1)) == (1 << (f.drop - 1))) & (a >= f.min_normal) & (a < f.max_finite)
    odd = ((bits >> f.drop) & 1) == 1
    n = max(1, p.numel())
    return float((tie & ~odd).sum()) / n, float((tie & odd).sum()) / n


def rne_by_integer_arithmetic(pre: torch.Tensor, fmt: str) -> torch.Tensor:
    """Round-to-nearest-even of fp32 values in the normal, unsaturated range of ``fmt``, done on the bit pattern (independent of
    torch's conversions): add half an ulp minus one plus the kept lsb, clear the dropped bits."""
    f = FORMATS[fmt]
    p = pre.to(torch.float32).contiguous()
    bits = p.view(torch.int32)
    mag = bits & 0x7FFFFFFF
    lsb = (mag >> f.drop) & 1
    mag = ((mag + ((1 << (f.drop - 1)) - 1) + lsb) >> f.drop) << f.drop
    return (mag | (bits & -0x80000000)).view(torch.float32)


@dataclass
class Exact:
    """One rounding point: ``pre`` the exact value before it (fp32, NCHW or (rows, cout)), ``ref`` the stored value (fp32 holding a
    value of the type), ``bound`` the largest sum of absolute terms of any output in lattice units, ``unit`` the lattice unit."""
    name: str
    pre: torch.Tensor
    ref: torch.Tensor
    bound: float
    unit: float
    fmt: str

    def ties(self):
        """(down, up) tie shares; a (head, tail) pair output has no single rounding, so none."""
        return tie_shares(self.pre, self.fmt) if self.fmt in FORMATS else (0.0, 0.0)

    def as_fmt(self, fmt: str) -> "Exact":
        """The same exact values stored in another 16-bit type (the lattice operands are exact in both)."""
        return Exact(self.name, self.pre, round_to(self.pre, fmt), self.bound, self.unit, fmt)

    def report(self) -> str:
        dn, up = self.ties()
        return (f"{self.name} [{self.fmt}]: {self.pre.numel()} outputs, max|out| {float(self.pre.abs().max()) / self.unit:.0f} units, "
                f"B {self.bound:.3g}, ties down {100 * dn:.2f} % up {100 * up:.2f} %, "
                f"rounded {100 * float((self.ref.double() != self.pre.double()).double().mean()):.1f} %")


def assert_exact_precondition(stages, regime: str, tie_floor: bool = True) -> None:
    """What makes bit equality a theorem, on every rounding point of a case: all terms are multiples of the unit, the sum of their
    absolute values is below 2^24 units (so every partial sum in any order is exact in fp32), fp16 does not saturate; small regime:
    nothing is rounded; wide regime (``tie_floor``): with 1000 outputs or more at least 1 % are ties of each parity."""
    for s in stages if isinstance(stages, (list, tuple)) else [stages]:
        q = s.pre.double() / s.unit
        assert bool((q == q.round()).all()), f"{s.name}: off the lattice"
        assert s.bound < LIMIT, f"{s.name}: B = {s.bound:.4g} units >= 2^24"
        assert float(q.abs().max()) <= s.bound
        if s.fmt == "fp16":
            assert float(s.ref.abs().max()) < 65504.0, f"{s.name}: saturates in fp16"
        if regime == "small":
            assert bool((s.ref.double() == s.pre.double()).all()), f"{s.name}: an output of the small regime is rounded: {s.report()}"
        elif tie_floor and s.pre.numel() >= 1000:
            dn, up = s.ties()
            assert dn >= 0.01 and up >= 0.01, f"{s.name}: too few ties: {s.report()}"


# ------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------
def conv_exact(name, x, w, bias, stride, pad, relu, res=None, *, unit, fmt="bf16") -> Exact:
    """One fused conv launch (NCHW / OIHW fp32 lattice tensors) through ``conv_bias_act_emulated``: the unrounded value, the stored
    one, and the bound B = conv(|x|, |w|) + |bias| + |residual| by the same function on the absolute values."""
    pre = conv_bias_act_emulated(x, w, bias, stride, pad, relu, residual_bf=res, fmt="fp32")
    b = conv_bias_act_emulated(x.abs(), w.abs(), bias.abs(), stride, pad, False, residual_bf=None if res is None else res.abs(), fmt="fp32")
    return Exact(name, pre, round_to(pre, fmt), float(b.max()) / unit, unit, fmt)


def cat_exact(name, x1, w1, x2, w2, bias, stride2, relu, *, unit, fmt="bf16") -> Exact:
    """The two-source 1x1 conv (NCHW / OIHW): ONE accumulation over K = [x1 | x2 at stride2].  With ReLU through ``conv_cat_emulated``
    (bias as b3, zero bd); without, the same sum as one conv over the concatenated channels."""
    zero = torch.zeros_like(bias)
    if relu:
        pre = conv_cat_emulated(x1, w1, bias, x2, w2, zero, stride2, fmt="fp32")
    else:
        pre = conv_bias_act_emulated(torch.cat([x1, x2[:, :, ::stride2, ::stride2]], 1), torch.cat([w1, w2], 1), bias, 1, 0, False, fmt="fp32")
    b = conv_bias_act_emulated(torch.cat([x1, x2[:, :, ::stride2, ::stride2]], 1).abs(), torch.cat([w1, w2], 1).abs(), bias.abs(), 1, 0, False,
                               fmt="fp32")
    return Exact(name, pre, round_to(pre, fmt), float(b.max()) / unit, unit, fmt)


def gemm_exact(name, x, w, bias, res, relu, *, unit, fmt) -> Exact:
    """One head GEMM through ``gemm_ref`` (fp64 on whatever device the operands are); the tensors of the result stay on that device."""
    from tests.head_kernels_reference import gemm_ref
    pre = gemm_ref(x, w, bias, res, relu).to(torch.float32)
    b = gemm_ref(x.abs(), w.abs(), bias.abs(), None if res is None else res.abs(), False)
    return Exact(name, pre, round_to(pre, fmt), float(b.max()) / unit, unit, fmt)


def _ms(t: torch.Tensor, unit: float) -> float:
    return max(float((t.double() / unit).pow(2).mean()), 1e-6)


def _w_for(shape_oihw, target: float, in_ms: float, gen, fmt="bf16") -> torch.Tensor:
    """Lattice weights (unit UW) that take inputs of mean square ``in_ms`` units to outputs of std ~ ``target`` units."""
    k = shape_oihw[1] * shape_oihw[2] * shape_oihw[3]
    return draw(shape_oihw, target / math.sqrt(k * in_ms), gen, UW, fmt)


def _bias(cout, r, unit, gen):
    return lattice((cout,), r, gen, unit=unit, fmt="fp16")       # fp32 on the device; 11 bits are plenty


# ------------------------------------------------------------------------------------------------------------------------------
# cases: host tensors (NCHW / OIHW unless said otherwise) and the rounding points of their reference
# ------------------------------------------------------------------------------------------------------------------------------
def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def conv_case(case, fmt: str, regime: str):
    """One CONV_CASES row: (x, w, bias, res or None) and its rounding point.  Both operands get the same spread,
    sigma^2 = target / sqrt(K) (wide: r ~ sqrt(4000 / sqrt(K)) / 0.58)."""
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    g = torch.Generator().manual_seed(seed_of("conv", case, regime))
    sig = math.sqrt(TARGET[regime] / math.sqrt(cin * k * k))
    x = draw((n, cin, h, w), sig, g, UX, fmt)
    wt = draw((cout, cin, k, k), sig, g, UW, fmt)
    u = UX * UW
    bias = _bias(cout, BIAS_R[regime], u, g)
    ho, wo = out_hw(h, w, k, stride, pad)
    res = lattice((n, cout, ho, wo), RES_R[regime], g, unit=u, fmt=fmt) if has_res else None
    return (x, wt, bias, res), conv_exact("conv", x, wt, bias, stride, pad, relu, res, unit=u, fmt=fmt)


def cat_case(case, fmt: str, regime: str):
    """One CAT_CASES row: (x1, x2 [NHWC], wcat (cout, c1 + c2), bias) in _cat_tensors' layout, and its rounding point."""
    n, h, c1, h2, c2, s2, cout, relu, _tile = case
    g = torch.Generator().manual_seed(seed_of("cat", case, regime))
    sig = math.sqrt(TARGET[regime] / math.sqrt(c1 + c2))
    x1 = draw((n, c1, h, h), sig, g, UX, fmt)
    x2 = draw((n, c2, h2, h2), sig, g, UX, fmt)
    w1 = draw((cout, c1, 1, 1), sig, g, UW, fmt)
    w2 = draw((cout, c2, 1, 1), sig, g, UW, fmt)
    bias = _bias(cout, BIAS_R[regime], UX * UW, g)
    st = cat_exact("cat", x1, w1, x2, w2, bias, s2, bool(relu), unit=UX * UW, fmt=fmt)
    dt = FORMATS[fmt].dtype
    tensors = (x1.permute(0, 2, 3, 1).contiguous().to(dt), x2.permute(0, 2, 3, 1).contiguous().to(dt),
               torch.cat([w1.view(cout, c1), w2.view(cout, c2)], 1).contiguous().to(dt), bias)
    return tensors, st


def gemm_case(shape, fmt: str, regime: str, device="cpu"):
    """One HEAD_GEMMS row: (x (rows, K), w (cout, K), bias, res or None) in _gemm_tensors' layout on the host, and its rounding point
    computed on ``device``.  "dw" rows keep their zero padding of K; "dx" / "dw" rows keep their zero bias."""
    rows, k, cout, relu, has_res, kind = shape[:6]
    g = torch.Generator().manual_seed(seed_of("gemm", shape, regime))
    keff = shape[6] if kind == "dw" else k
    sig = math.sqrt(TARGET[regime] / math.sqrt(keff))
    x = draw((rows, k), sig, g, UX, fmt)
    w = draw((cout, k), sig, g, UW, fmt)
    if kind == "dw":
        x[:, shape[6]:] = 0
        w[:, shape[6]:] = 0
    u = UX * UW
    bias = _bias(cout, BIAS_R[regime], u, g) if kind == "fwd" else torch.zeros(cout)
    res = lattice((rows, cout), RES_R[regime], g, unit=u, fmt=fmt) if has_res else None
    dt = FORMATS[fmt].dtype
    st = gemm_exact("gemm", x.to(device), w.to(device), bias.to(device), res.to(device) if has_res else None, bool(relu), unit=u, fmt=fmt)
    return (x.to(dt), w.to(dt), bias, res.to(dt) if has_res else None), st


def fp8_case(case, regime: str):
    """One FP8_CASES row with power-of-two scales: (xq, wq, bias, rq or None, (sx, sw, sr, sy)) in _fp8_tensors' layout (NHWC / OHWI
    e4m3) and its rounding point, in units of sy.  wide: the scale sx sw / sy puts the outputs' std near 250, so that part of them
    saturates at 448 and the rest is spread over the binades where e4m3 rounds; small: every output is an integer up to 16."""
    from tests.test_kernels_gpu import fp8_reference
    n, h, w, cin, cout, k, stride, pad, relu, has_res, _tile = case
    g = torch.Generator().manual_seed(seed_of("fp8", case, regime))
    kk = cin * k * k
    ho, wo = out_hw(h, w, k, stride, pad)
    sx, sw = 2.0 ** -3, 2.0 ** -5
    if regime == "small":
        sig = math.sqrt(2.5 / math.sqrt(kk))
        f, fr, br, rr = 1.0, 1.0, 1, 2
    else:
        sig = 2.58                                                       # integers in [-4, 4]
        f = 2.0 ** round(math.log2(250.0 / (sig * sig * math.sqrt(kk))))
        fr, br, rr = 8.0, 16, 16
    sy = sx * sw / f
    sr = fr * sy
    xq = draw((n, h, w, cin), sig, g, fmt="e4m3")
    wq = draw((cout, k, k, cin), sig, g, fmt="e4m3")
    bias = lattice((cout,), br, g, unit=sy * max(f, 1.0), fmt="fp16")
    rq = lattice((n, ho, wo, cout), rr, g, fmt="e4m3") if has_res else None
    scales = (sx, sw, sr, sy)
    pre = fp8_reference(xq, wq, bias, rq, scales, stride, pad, bool(relu))
    b = fp8_reference(xq.abs(), wq.abs(), bias.abs(), None if rq is None else rq.abs(), scales, stride, pad, False)
    unit = min(f, 1.0)
    assert bool((pre.float().double() == pre).all())
    st = Exact("fp8", pre.float(), fp8_round(pre), float(b.max()) / unit, unit, "e4m3")
    dt = torch.float8_e4m3fn
    return (xq.to(dt), wq.to(dt), bias, rq.to(dt) if has_res else None, scales), st


def w2_case(case, regime: str):
    """One PAIR_CASES row in the bf16w2 mode, head and tail planes each a lattice of its own: (x, w_head, w_tail, bias, res or None)
    and the rounding point of x.w_head + x.w_tail in one accumulator -- one conv over K = [x | x] against [w_head | w_tail]."""
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    g = torch.Generator().manual_seed(seed_of("w2", case, regime))
    sig = math.sqrt(TARGET[regime] / math.sqrt(2 * cin * k * k))
    x = draw((n, cin, h, w), sig, g, UX)
    wh = draw((cout, cin, k, k), sig, g, UW)
    wt = draw((cout, cin, k, k), sig, g, UW)
    u = UX * UW
    bias = _bias(cout, BIAS_R[regime], u, g)
    ho, wo = out_hw(h, w, k, stride, pad)
    res = lattice((n, cout, ho, wo), RES_R[regime], g, unit=u) if has_res else None
    st = conv_exact("w2", torch.cat([x, x], 1), torch.cat([wh, wt], 1), bias, stride, pad, relu, res, unit=u)
    return (x, wh, wt, bias, res), st


def split_case(case, regime: str):
    """One PAIR_CASES row in the fp32x mode, every plane a lattice of its own: ((x_head, x_tail), (w_head, w_tail), bias, (r_head,
    r_tail) or None) and the fp32 value before the result is split: x_head.w_head + x_tail.w_head + x_head.w_tail as one conv over
    K = [x_head | x_tail | x_head] against [w_head | w_head | w_tail] (the device's packed rows).  The stored planes are
    ``split_pair`` of it; ``Exact.ref`` holds the pair's value, which ``fp32x_conv(..., mutation="device")`` defines."""
    from tests import pair_reference as P
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    g = torch.Generator().manual_seed(seed_of("split", case, regime))
    # a pair holds 16 significant bits: the wide regime aims 16 x higher than the 16-bit types', past 2^16 units, so that the tail rounds
    sig = math.sqrt((16.0 if regime == "wide" else 1.0) * TARGET[regime] / math.sqrt(3 * cin * k * k))
    xh, xt = draw((n, cin, h, w), sig, g, UX), draw((n, cin, h, w), sig, g, UX)
    wh, wt = draw((cout, cin, k, k), sig, g, UW), draw((cout, cin, k, k), sig, g, UW)
    u = UX * UW
    bias = _bias(cout, BIAS_R[regime], u, g)
    ho, wo = out_hw(h, w, k, stride, pad)
    rp = (lattice((n, cout, ho, wo), RES_R[regime], g, unit=u), lattice((n, cout, ho, wo), RES_R[regime], g, unit=u)) if has_res else None
    st = conv_exact("split", torch.cat([xh, xt, xh], 1), torch.cat([wh, wh, wt], 1), bias, stride, pad, relu,
                    None if rp is None else rp[0] + rp[1], unit=u)
    hd, tl = P.split_pair(st.pre)
    st.ref = P.pair_value(hd, tl).float()
    dev = P.fp32x_conv((xh, xt), (wh, wt), bias, stride, pad, relu, rp, mutation="device")
    assert bool((dev == st.ref.double()).all()), "split_case: the packed-row conv is not pair_reference's device arithmetic"
    st.fmt = "pair"
    return ((xh, xt), (wh, wt), bias, rp), st


def stem_case(n: int, regime: str):
    """Lattice frames (N,3,224,224) fp32 and lattice folded stem weights (64,3,7,7) fp32, K = 147: (x, w, bias) and the rounding point."""
    g = torch.Generator().manual_seed(seed_of("stem", n, regime))
    sig = math.sqrt(TARGET[regime] / math.sqrt(147.0))
    x = draw((n, 3, 224, 224), sig, g, UX)
    wf = draw((64, 3, 7, 7), sig, g, UW)
    bias = _bias(64, BIAS_R[regime], UX * UW, g)
    return (x, wf, bias), conv_exact("stem", x, wf, bias, 2, 3, True, unit=UX * UW)


def avgpool_case(shape):
    """Lattice (N,H,W,C) bf16 input and float32(exact sum) * float32(1 / HW), what avgpool_kernel computes."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed_of("avgpool", shape))
    x = lattice(shape, 255, g, unit=UX)
    s = x.double().view(n, h * w, c).sum(dim=1)
    assert float(x.abs().double().view(n, h * w, c).sum(dim=1).max()) / UX < LIMIT
    ref = s.to(torch.float32) * torch.tensor(1.0 / (h * w), dtype=torch.float32)
    return x.to(torch.bfloat16), ref


class _Chain:
    """Stages of a fused chain, from the inputs: each stage reads the stored (rounded) value of the one before."""

    def __init__(self, key, regime):
        self.g = torch.Generator().manual_seed(seed_of(key, regime))
        self.regime = regime
        self.stages: List[Exact] = []

    def conv(self, name, x, x_unit, cout, k, stride, pad, relu, target, res=None, w=None, bias_r=None):
        """Draw weights and bias for ``x`` (values in ``x_unit``), append the stage, return (w, bias, stage)."""
        if w is None:
            w = _w_for((cout, x.shape[1], k, k), target, _ms(x, x_unit), self.g)
        u = x_unit * UW
        bias = _bias(cout, BIAS_R[self.regime] if bias_r is None else bias_r, u, self.g)
        st = conv_exact(name, x, w, bias, stride, pad, relu, res, unit=u)
        self.stages.append(st)
        return w, bias, st

    def act(self, shape, sigma, unit=UX, nonneg=False):
        return draw(shape, sigma, self.g, unit, nonneg=nonneg)


def _targets(regime, stages: int, emph: Optional[int]):
    """Output std each stage of a chain aims at.  The small regime bounds the PRODUCT of the stages' non-zero term counts (magnitudes
    multiply along the chain and every output must stay within 256 units), so one stage is chosen to be dense: the stages before
    ``emph`` stay near 3 units, ``emph`` aims at 40 (20 when stages follow it), and the stages after it add only a term or two of that
    size.  Default: the last."""
    if regime == "wide":
        return [INTER[regime]] * (stages - 1) + [LAST[regime]]
    emph = stages - 1 if emph is None else emph
    return [INTER[regime] if i < emph else 8.0 if i > emph else LAST[regime] if i == stages - 1 else 20.0 for i in range(stages)]


def _inter_r(regime):
    """(bias range, identity spread) of an intermediate stage."""
    return (1, 2.0) if regime == "small" else (100, 150.0)


def tail_case(cmid, c1, shape, ds, regime, key=(), emph=None):
    """A bottleneck tail (``bneck_tail_bf16``; c1 = 0: ``conv3_identity_tail3_bf16``): host tensors in the order of _tail_tensors
    (cmid 64: y2, w3, b3, w1, b1, idn | xin, wd, bd) or of _tail2_tensors / _tail3_inputs (y2, w3, b3, idn, w1, b1), NCHW / OIHW bf16,
    and the rounding points [identity,] out, y1n."""
    n, h, w = shape
    c = _Chain(("tail", cmid, c1, shape, ds, key), regime)
    br, isig = _inter_r(regime)
    last = c1 == 0
    t_out, t_y1 = _targets(regime, 2, emph)
    y2 = c.act((n, cmid, h, w), math.sqrt(t_out / math.sqrt(cmid)) if not last else math.sqrt(TARGET[regime] / math.sqrt(cmid)))
    u = UX * UW
    if ds:
        xin = c.act((n, cmid, h, w), 1.0 if regime == "small" else 4.0)
        wd, bd, st_id = c.conv("identity", xin, UX, 4 * cmid, 1, 1, 0, False, isig, bias_r=br)
        idn = st_id.ref
    else:
        idn = draw((n, 4 * cmid, h, w), isig if not last else RES_R[regime] * 0.58, c.g, u)
    w3, b3, st_out = c.conv("out", y2, UX, 4 * cmid, 1, 1, 0, True, t_out if not last else TARGET[regime], res=idn,
                            bias_r=None if last else br)
    bf = torch.bfloat16
    if last:
        return (y2.to(bf), w3.to(bf), b3, idn.to(bf), None, None), c.stages
    w1, b1, _ = c.conv("y1n", st_out.ref, u, c1, 1, 1, 0, True, t_y1)
    if cmid == 64:
        rest = (xin.to(bf), wd.to(bf), bd) if ds else (idn.to(bf),)
        return (y2.to(bf), w3.to(bf), b3, w1.to(bf), b1) + rest, c.stages
    return (y2.to(bf), w3.to(bf), b3, idn.to(bf), w1.to(bf), b1), c.stages


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def block_case(layer, n, c1, regime, ds=False, emph=None):
    """A bottleneck body (``bneck_block1_bf16`` / ``bneck_block1_ds_bf16`` / ``bneck_block2_bf16``; c1 = 0: no chained conv1): host
    tensors in the order of _block1_tensors / _block2_tensors (t1, idn, w2, w3, w1, b2, b3, b1) or _block1_ds_tensors
    (t1, x, w2, w3, wd, w1, b2, b3, bd, b1), NHWC / OHWI bf16, and the rounding points t2, [identity,] out, [y1n]."""
    hw, cm = (56, 64) if layer == 1 else (28, 128)
    c = _Chain(("block", layer, n, c1, ds), regime)
    br, isig = _inter_r(regime)
    t_t2, t_out, t_y1 = _targets(regime, 3, emph)
    t1 = c.act((n, cm, hw, hw), 1.0 if regime == "small" else 4.0, nonneg=True)
    w2, b2, st2 = c.conv("t2", t1, UX, cm, 3, 1, 1, True, t_t2, bias_r=br)
    u2 = UX * UW
    u = u2 * UW
    if ds:
        x = c.act((n, cm, hw, hw), 1.0 if regime == "small" else 4.0, unit=u2, nonneg=True)
        wd, bd, st_id = c.conv("identity", x, u2, 4 * cm, 1, 1, 0, False, isig, bias_r=br)
        idn = st_id.ref
    else:
        idn = draw((n, 4 * cm, hw, hw), isig, c.g, u, nonneg=True)
    w3, b3, st_out = c.conv("out", st2.ref, u2, 4 * cm, 1, 1, 0, True, t_out, res=idn, bias_r=br)
    ohwi = lambda t: t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)       # noqa: E731
    if c1:
        w1, b1, _ = c.conv("y1n", st_out.ref, u, c1, 1, 1, 0, True, t_y1)
        w1 = ohwi(w1)
    else:
        w1 = b1 = None
    if ds:
        return (_nhwc(t1), _nhwc(x), ohwi(w2), ohwi(w3), ohwi(wd), w1, b2, b3, bd, b1), c.stages
    return (_nhwc(t1), _nhwc(idn), ohwi(w2), ohwi(w3), w1, b2, b3, b1), c.stages


def cat_chain_case(n, regime, emph=None):
    """``bneck_cat_chain_bf16``: host tensors in the order of _cat_chain_tensors (t2, x, w3, wd, bcat, w1, b1; NCHW / OIHW bf16) and
    the rounding points out (``conv_cat_emulated``), y1n."""
    c = _Chain(("cat_chain", n), regime)
    br, _ = _inter_r(regime)
    t_out, t_y1 = _targets(regime, 2, emph)
    sig = math.sqrt(t_out / math.sqrt(384.0))
    t2 = c.act((n, 128, 28, 28), sig)
    x = c.act((n, 256, 56, 56), sig)
    w3 = draw((512, 128, 1, 1), sig, c.g, UW)
    wd = draw((512, 256, 1, 1), sig, c.g, UW)
    u = UX * UW
    bcat = _bias(512, br, u, c.g)
    st = cat_exact("out", t2, w3, x, wd, bcat, 2, True, unit=u)
    c.stages.append(st)
    w1, b1, _ = c.conv("y1n", st.ref, u, 128, 1, 1, 0, True, t_y1)
    bf = torch.bfloat16
    return (t2.to(bf), x.to(bf), w3.to(bf), wd.to(bf), bcat, w1.to(bf), b1), c.stages


def nchw_of(y_nhwc: torch.Tensor) -> torch.Tensor:
    """A device NHWC result as fp32 NCHW on the host, the layout of the references."""
    return y_nhwc.float().cpu().permute(0, 3, 1, 2).contiguous()


def assert_bits_equal(got_f32: torch.Tensor, st: Exact, what: str) -> None:
    """Zero tolerance: the stored values are the reference's, element for element (values of a 16-bit / 8-bit type held in fp32
    compare as their bit patterns do, up to the sign of zero, which the bit view below includes)."""
    ref = st.ref.to(got_f32.device)
    assert got_f32.shape == ref.shape, f"{what}: shape {tuple(got_f32.shape)} vs {tuple(ref.shape)}"
    same = got_f32.contiguous().view(torch.int32) == ref.to(torch.float32).contiguous().view(torch.int32)
    if not bool(same.all()):
        bad = ~same
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements differ from the exact reference; first at {idx}: "
                             f"got {float(got_f32[tuple(idx)])!r}, ref {float(ref[tuple(idx)])!r}, unrounded {float(st.pre[tuple(idx)])!r} "
                             f"({st.report()})")


# ------------------------------------------------------------------------------------------------------------------------------
# the fused-chain cases the GPU file runs: id -> (runner in tests/test_kernels_gpu.py, its arguments, builder of (tensors, stages))
# ------------------------------------------------------------------------------------------------------------------------------
def chain_cases():
    """The dense stage of the small regime (``_targets``) rotates over a kernel's cases, so that each stage of each kernel is dense in one."""
    cases = {}
    for i, (shape, c1) in enumerate((((2, 7, 9), 64), ((1, 56, 56), 128), ((3, 5, 16), 64), ((5, 56, 56), 64))):
        for ds in (False, True):
            cases["tail1_%s_c%d_%s" % ("x".join(map(str, shape)), c1, "ds" if ds else "id")] = (
                "_run_bneck_tail", (shape, c1, ds), lambda r, a=(64, c1, shape, ds), e=i % 2: tail_case(*a, r, emph=e))
    for i, shape in enumerate(((2, 7, 9), (1, 28, 28), (3, 5, 16), (9, 28, 28))):
        cases["tail2_" + "x".join(map(str, shape))] = (
            "_run_bneck_tail_layer2", (shape,), lambda r, s=shape, e=i % 2: tail_case(128, 128, s, False, r, emph=e))
    for i, (shape, bp) in enumerate((((2, 7, 9), 0), ((1, 14, 14), 0), ((5, 14, 14), 33), ((20, 14, 14), 7))):
        cases["tail3_%s_bp%d" % ("x".join(map(str, shape)), bp)] = (
            "_run_bneck_tail_layer3", (shape, bp), lambda r, s=shape, b=bp, e=i % 2: tail_case(256, 256, s, False, r, key=b, emph=e))
    for n in (1, 5):
        cases["tail3_last_n%d" % n] = ("_run_layer3_last_block", (n,), lambda r, n=n: tail_case(256, 0, (n, 14, 14), False, r))
    for i, n in enumerate((1, 3, 20)):
        for c1 in (64, 128):
            cases["block1_n%d_c%d" % (n, c1)] = ("_run_bneck_block1", (n, c1), lambda r, n=n, c=c1, e=i: block_case(1, n, c, r, emph=e))
        cases["block1_ds_n%d" % n] = ("_run_bneck_block1_ds", (n,), lambda r, n=n, e=i: block_case(1, n, 64, r, ds=True, emph=e))
    for i, n in enumerate((1, 3, 70)):
        for chain in (False, True):
            cases["block2_n%d_%s" % (n, "chained" if chain else "last")] = (
                "_run_bneck_block2", (n, chain), lambda r, n=n, e=i if chain else min(i, 1): block_case(2, n, 128, r, emph=e))
    for i, n in enumerate((1, 3, 37)):
        cases["cat_chain_n%d" % n] = ("_run_bneck_cat_chain", (n,), lambda r, n=n, e=i % 2: cat_chain_case(n, r, emph=e))
    return cases


CHAIN_CASES = chain_cases()
STEM_N = (1, 3)
AVGPOOL_SHAPES = ((4, 7, 7, 2048), (1, 3, 3, 8))
