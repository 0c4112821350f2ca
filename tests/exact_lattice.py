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

Two more regimes hold the fp16 and e4m3 kernels at the ENDS of their formats (``EDGE_REGIMES``).  They are the wide regime's integer
draws (same seeds, same integers) at other power-of-two units, so everything above carries over: scaling by 2^a is exact, and the
2^24-unit argument does not care where the unit sits as long as the fp32 accumulator stays normal (every unit here is >= 2^-27).
  low    fp16: one operand carries subnormal values (unit 2^-16; ``side`` "x": the activations, "w": the weights), the other sits at
         unit 2^-11; the outputs are multiples of 2^-27 around 2^-15: most of them round on the subnormal grid 2^-24 and drop three
         bits.  Residuals are stored in fp16: multiples of 2^-24 (the wide integers truncated to multiples of 8); the fp32 bias stays on
         2^-27.  e4m3: operands at unit 2^-9 (integers 1..7 subnormal, 8..16 normal), outputs multiples of 2^-12 of sy on both sides of
         2^-6, the residual subnormal too.
  high   fp16 only: operands at unit 2^2, products at 2^4, so the wide outputs straddle 65504 (4094 units of 2^4).  The bias (fp32)
         sits on 2^3 and plants, for each sign the op can produce, outputs exactly at 65504, 65512 (strictly between), 65520 (the tie
         IEEE rounds to infinity) and 65536.  The reference clamps, then rounds: +-65504, never an infinity.  (e4m3 saturation at 448
         is the wide regime's.)
  Not built: bf16 low / high.  A bf16 subnormal is an fp32 subnormal and bf16's top is fp32's top; the lattice argument needs a normal
  fp32 accumulator, and no activation of this network gets near either end.

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
EDGE_REGIMES = ("low", "high")       # the ends of fp16 / e4m3: the wide regime's integer draws at other units
BASE = {"small": "small", "wide": "wide", "low": "wide", "high": "wide"}      # whose seeds, spreads and ranges a regime draws with
LIMIT = 2.0 ** 24
FP32_MIN_NORMAL = 2.0 ** -126


@dataclass(frozen=True)
class Fmt:
    dtype: torch.dtype
    max_int: int          # integers up to this are exact in the type
    drop: int             # fp32 significand bits the type drops
    min_normal: float
    max_finite: float

    @property
    def sub_step(self) -> float:
        """Spacing of the type's subnormal grid: min_normal / 2^(explicit significand bits)."""
        return self.min_normal * 2.0 ** (self.drop - 23)


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
HIGH_PLANTS = (65504.0, 65512.0, 65520.0, 65536.0)      # the largest finite half, a value the clamp alone decides, the tie to infinity, 2^16


@dataclass(frozen=True)
class Units:
    """Power-of-two units of one case: activations, weights, the lattice unit of the rounding point (bias and outputs are multiples
    of it) and the step of the residual's integers in product units (a stored residual must be representable in the type)."""
    ux: float
    uw: float
    out: float
    res_step: int = 1

    @property
    def prod(self) -> float:
        return self.ux * self.uw


def units_of(regime: str, fmt: str = "bf16", side: str = "x", gain: float = 1.0) -> Units:
    """small / wide: UX, UW for every type (unchanged).  low / high exist for fp16 only (module docstring); ``side`` names the operand
    that carries the subnormal values of the low regime; ``gain`` (a power of two) raises the activations' unit of the high regime
    for a case whose outputs see only part of K (a 3x3 conv of a single pixel), so that it straddles 65504 like the others."""
    if regime in REGIMES:
        return Units(UX, UW, UX * UW)
    if fmt != "fp16":
        raise ValueError(f"the {regime} regime is built for fp16 (and, low, for e4m3 through fp8_case), not for {fmt}")
    if regime == "low":
        sub, other = 2.0 ** -16, 2.0 ** -11
        ux, uw = (sub, other) if side == "x" else (other, sub)
        return Units(ux, uw, 2.0 ** -27, 8)
    if regime == "high":
        return Units(4.0 * gain, 4.0, 8.0)
    raise ValueError(regime)


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


def tie_shares(pre: torch.Tensor, fmt: str, grid: str = "normal"):
    """Shares of the elements of ``pre`` (exact fp32 values before the rounding to ``fmt``) that sit exactly halfway between two
    neighbours of the type: (down, up) by the parity of the neighbour of smaller magnitude (even, odd).  ``grid`` "normal" counts the
    ties between min_normal and max_finite, "subnormal" -- a separate count -- those below min_normal, halfway between two multiples
    of the subnormal spacing (0 is the even neighbour of half a step).  Values at or beyond max_finite are in neither: the clamp
    decides them, not the rounding."""
    f = FORMATS[fmt]
    p = pre.to(torch.float32).contiguous()
    assert bool((p.double() == pre.double()).all()), "tie_shares: not an fp32 value"
    a = p.abs()
    n = max(1, p.numel())
    if grid == "subnormal":
        q = a.double() / f.sub_step                    # exact: a power-of-two scaling of an fp32 value
        fl = q.floor()
        tie = (q - fl == 0.5) & (a < f.min_normal)
        odd = fl.remainder(2.0) == 1.0
    else:
        bits = p.view(torch.int32) & 0x7FFFFFFF
        tie = ((bits & ((1 << f.drop) - 1)) == (1 << (f.drop - 1))) & (a >= f.min_normal) & (a < f.max_finite)
        odd = ((bits >> f.drop) & 1) == 1
    return float((tie & ~odd).sum()) / n, float((tie & odd).sum()) / n


def subnormal_share(t: torch.Tensor, fmt: str) -> float:
    """Share of the NONZERO elements of ``t`` whose magnitude is below the type's smallest normal number."""
    a = t.abs()
    nz = a > 0
    return float(((a < FORMATS[fmt].min_normal) & nz).sum()) / max(1, int(nz.sum()))


def rne_by_integer_arithmetic(pre: torch.Tensor, fmt: str) -> torch.Tensor:
    """Round-to-nearest-even of fp32 values to ``fmt`` with saturation at the largest finite value, done on the bit pattern
    (independent of torch's conversions).  Normal range: add half an ulp minus one plus the kept lsb, clear the dropped bits.  Below
    min_normal: the 24-bit significand m (value m 2^(e - 150)) is shifted right onto the subnormal grid by s = log2(step) + 150 - e
    bits with the same add-and-shift; s >= 26 leaves 0.  At the top: a rounded magnitude beyond max_finite becomes max_finite (the same
    as clamping first: max_finite is representable, so min(rne(x), max) == rne(min(x, max)))."""
    f = FORMATS[fmt]
    p = pre.to(torch.float32).contiguous()
    bits = p.view(torch.int32)
    mag = bits & 0x7FFFFFFF
    lsb = (mag >> f.drop) & 1
    normal = ((mag + ((1 << (f.drop - 1)) - 1) + lsb) >> f.drop) << f.drop
    if math.isfinite(f.max_finite):
        top = int(torch.tensor(f.max_finite, dtype=torch.float32).view(torch.int32))
        normal = torch.minimum(normal, torch.tensor(top, dtype=torch.int32))
    out = (normal | (bits & -0x80000000)).view(torch.float32)
    min_bits = int(torch.tensor(f.min_normal, dtype=torch.float32).view(torch.int32))
    sub = mag < min_bits
    if fmt != "bf16" and bool(sub.any()):
        e = (mag >> 23).to(torch.int64)
        m = (mag & 0x7FFFFF).to(torch.int64) | torch.where(e > 0, 1 << 23, 0)
        e = e.clamp_min(1)                                                # an fp32 subnormal: m 2^-149
        s = (int(math.log2(f.sub_step)) + 150 - e).clamp(1, 40)
        k = (m + (torch.ones_like(s) << (s - 1)) - 1 + ((m >> s) & 1)) >> s
        small = k.to(torch.float32) * f.sub_step                          # k <= 2^10: exact
        small = torch.where(bits < 0, -small, small)
        out = torch.where(sub, small, out)
    return out


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
    operands: tuple = ()       # edge regimes: the fp32 tensors of the operand side(s) that carry subnormal values (their share is a condition)
    planted: tuple = ()        # high regime: the boundary values the bias plants

    def ties(self):
        """(down, up) tie shares; a (head, tail) pair output has no single rounding, so none."""
        return tie_shares(self.pre, self.fmt) if self.fmt in FORMATS else (0.0, 0.0)

    def as_fmt(self, fmt: str) -> "Exact":
        """The same exact values stored in another 16-bit type (the lattice operands are exact in both)."""
        return Exact(self.name, self.pre, round_to(self.pre, fmt), self.bound, self.unit, fmt, self.operands, self.planted)

    def edge_report(self) -> str:
        """What the low / high conditions read, as shares."""
        f = FORMATS[self.fmt]
        a = self.pre.abs()
        dn, up = tie_shares(self.pre, self.fmt, "subnormal")
        return (f"{self.name} [{self.fmt}]: nonzero outputs subnormal {100 * subnormal_share(self.pre, self.fmt):.1f} %, subnormal-grid ties down "
                f"{100 * dn:.2f} % up {100 * up:.2f} %, operand subnormal "
                f"{'/'.join('%.1f' % (100 * subnormal_share(o, self.fmt)) for o in self.operands) or '-'} %, beyond max "
                f"{100 * float((a > f.max_finite).float().mean()):.1f} %, top binade {100 * float(((a >= 2.0 ** math.floor(math.log2(f.max_finite))) & (a <= f.max_finite)).float().mean()):.1f} %")

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
        assert s.unit >= FP32_MIN_NORMAL, f"{s.name}: a term of one unit would be an fp32 subnormal"
        if regime in EDGE_REGIMES:
            continue                                   # assert_edge_precondition holds what these regimes add
        if s.fmt == "fp16":
            assert float(s.ref.abs().max()) < 65504.0, f"{s.name}: saturates in fp16"
        if regime == "small":
            assert bool((s.ref.double() == s.pre.double()).all()), f"{s.name}: an output of the small regime is rounded: {s.report()}"
        elif tie_floor and s.pre.numel() >= 1000:
            dn, up = s.ties()
            assert dn >= 0.01 and up >= 0.01, f"{s.name}: too few ties: {s.report()}"


def low_output_condition(s: "Exact") -> bool:
    """At least 20 % of the nonzero outputs are subnormal in the stored type and, with 1000 outputs or more, at least 1 % of all
    outputs are subnormal-grid ties of each parity."""
    dn, up = tie_shares(s.pre, s.fmt, "subnormal")
    return subnormal_share(s.pre, s.fmt) >= 0.20 and (s.pre.numel() < 1000 or (dn >= 0.01 and up >= 0.01))


def assert_edge_precondition(stages, regime: str) -> None:
    """The conditions of the low and high regimes, on top of ``assert_exact_precondition`` (lattice, B < 2^24 units, no term below
    2^-126), as conditions a case must meet and not as measurements.
    low   the output condition (``low_output_condition``) at one stage of a chain at least (a single launch: at its one stage), and
          at least 5 % of the nonzero values of every operand listed as carrying them are subnormal;
    high  between 5 % and 50 % of the outputs lie beyond +-65504, at least 5 % lie in [32768, 65504], and the planted boundary
          values are present: outputs exactly at 65504, 65512, 65520 and 65536, negative ones too where the op has no ReLU."""
    stages = list(stages) if isinstance(stages, (list, tuple)) else [stages]
    assert_exact_precondition(stages, regime)
    assert regime in EDGE_REGIMES
    for s in stages:
        assert s.fmt in ("fp16", "e4m3") and (regime == "low" or s.fmt == "fp16"), f"{s.name}: no {regime} regime for {s.fmt}"
    if regime == "low":
        assert any(low_output_condition(s) for s in stages), "; ".join(s.edge_report() for s in stages)
        carriers = [(s, o) for s in stages for o in s.operands]
        assert carriers, "a low case must name the operand that carries subnormal values"
        for s, o in carriers:
            assert subnormal_share(o, s.fmt) >= 0.05, f"{s.name}: too few subnormal operand values: {s.edge_report()}"
        return
    for s in stages:
        a = s.pre.abs()
        beyond = float((a > 65504.0).float().mean())
        top = float(((a >= 32768.0) & (a <= 65504.0)).float().mean())
        assert 0.05 <= beyond <= 0.50 and top >= 0.05, f"{s.name}: {s.edge_report()}"
        assert bool(torch.isfinite(s.ref).all()) and float(s.ref.abs().max()) == 65504.0, f"{s.name}: the reference must saturate, finite"
        assert s.planted, f"{s.name}: nothing planted"
        for v in s.planted:
            assert bool((s.pre == v).any()), f"{s.name}: no output exactly at {v}"


def describe_mismatch(got_f32: torch.Tensor, st: "Exact") -> str:
    """Counts that tell the ways an end of a format goes wrong apart: a flush (0 where the reference is not), an infinity or NaN, a
    result one grid step of the stored type away (a mis-rounding), anything else."""
    ref = st.ref.to(got_f32.device).to(torch.float32)
    bad = got_f32.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)
    flush = bad & (got_f32 == 0) & (ref != 0)
    nonfin = bad & ~torch.isfinite(got_f32)
    if st.fmt in FORMATS:
        f = FORMATS[st.fmt]
        a = torch.maximum(got_f32.abs(), ref.abs()).clamp_min(f.min_normal)
        step = torch.pow(2.0, torch.floor(torch.log2(a.double())) - (23 - f.drop))
        one = bad & ~flush & ~nonfin & ((got_f32.double() - ref.double()).abs() <= step)
    else:
        one = torch.zeros_like(bad)
    sign0 = bad & (got_f32 == 0) & (ref == 0)
    other = bad & ~flush & ~nonfin & ~one & ~sign0
    return (f"{int(bad.sum())} of {ref.numel()} differ: flushed to zero {int(flush.sum())}, infinite or NaN {int(nonfin.sum())}, "
            f"one grid step off {int(one.sum())}, sign of zero {int(sign0.sum())}, other {int(other.sum())}")


# ------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------
def conv_exact(name, x, w, bias, stride, pad, relu, res=None, *, unit, fmt="bf16", **kw) -> Exact:
    """One fused conv launch (NCHW / OIHW fp32 lattice tensors) through ``conv_bias_act_emulated``: the unrounded value, the stored
    one, and the bound B = conv(|x|, |w|) + |bias| + |residual| by the same function on the absolute values."""
    pre = conv_bias_act_emulated(x, w, bias, stride, pad, relu, residual_bf=res, fmt="fp32")
    b = conv_bias_act_emulated(x.abs(), w.abs(), bias.abs(), stride, pad, False, residual_bf=None if res is None else res.abs(), fmt="fp32")
    return Exact(name, pre, round_to(pre, fmt), float(b.max()) / unit, unit, fmt, **kw)


def cat_exact(name, x1, w1, x2, w2, bias, stride2, relu, *, unit, fmt="bf16", **kw) -> Exact:
    """The two-source 1x1 conv (NCHW / OIHW): ONE accumulation over K = [x1 | x2 at stride2].  With ReLU through ``conv_cat_emulated``
    (bias as b3, zero bd); without, the same sum as one conv over the concatenated channels."""
    zero = torch.zeros_like(bias)
    if relu:
        pre = conv_cat_emulated(x1, w1, bias, x2, w2, zero, stride2, fmt="fp32")
    else:
        pre = conv_bias_act_emulated(torch.cat([x1, x2[:, :, ::stride2, ::stride2]], 1), torch.cat([w1, w2], 1), bias, 1, 0, False, fmt="fp32")
    b = conv_bias_act_emulated(torch.cat([x1, x2[:, :, ::stride2, ::stride2]], 1).abs(), torch.cat([w1, w2], 1).abs(), bias.abs(), 1, 0, False,
                               fmt="fp32")
    return Exact(name, pre, round_to(pre, fmt), float(b.max()) / unit, unit, fmt, **kw)


def gemm_exact(name, x, w, bias, res, relu, *, unit, fmt, **kw) -> Exact:
    """One head GEMM through ``gemm_ref`` (fp64 on whatever device the operands are); the tensors of the result stay on that device."""
    from tests.head_kernels_reference import gemm_ref
    pre = gemm_ref(x, w, bias, res, relu).to(torch.float32)
    b = gemm_ref(x.abs(), w.abs(), bias.abs(), None if res is None else res.abs(), False)
    return Exact(name, pre, round_to(pre.cpu(), fmt).to(pre.device), float(b.max()) / unit, unit, fmt, **kw)      # the CPU's conversion is the one checked


def _ms(t: torch.Tensor, unit: float) -> float:
    return max(float((t.double() / unit).pow(2).mean()), 1e-6)


def _w_for(shape_oihw, target: float, in_ms: float, gen, fmt="bf16", unit=UW) -> torch.Tensor:
    """Lattice weights (unit UW) that take inputs of mean square ``in_ms`` units to outputs of std ~ ``target`` units."""
    k = shape_oihw[1] * shape_oihw[2] * shape_oihw[3]
    return draw(shape_oihw, target / math.sqrt(k * in_ms), gen, unit, fmt)


def _bias(cout, r, unit, gen):
    return lattice((cout,), r, gen, fmt="fp16") * unit           # fp32 on the device; 11 bits are plenty (the scaling is exact)


def _res(shape, r, un: Units, gen, fmt):
    """A stored residual: the regime's integers (truncated toward zero to multiples of ``un.res_step``) in product units."""
    v = lattice(shape, r, gen, fmt=fmt)
    if un.res_step > 1:
        v = torch.trunc(v / un.res_step) * un.res_step
    v = v * un.prod
    assert representable(v, fmt)
    return v


def plant_boundaries(lin: torch.Tensor, bias: torch.Tensor, relu: bool):
    """High regime: shift the bias of the first 4 (ReLU) or 8 channels so that one output of each -- the one already closest, to keep
    the shift small -- lands exactly on +-65504, +-65512, +-65520, +-65536.  ``lin`` (channels in dim 1) is the exact pre-activation
    value with ``bias``; returns (the new bias, the planted values)."""
    bias = bias.clone()
    planted = tuple(sg * v for sg in ((1.0,) if relu else (1.0, -1.0)) for v in HIGH_PLANTS)
    assert lin.shape[1] >= len(planted)
    for c, v in enumerate(planted):
        d = (v - lin[:, c].double()).flatten()
        bias[c] += float(d[d.abs().argmin()])
    return bias, planted


# ------------------------------------------------------------------------------------------------------------------------------
# cases: host tensors (NCHW / OIHW unless said otherwise) and the rounding points of their reference
# ------------------------------------------------------------------------------------------------------------------------------
def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def _edge_kw(regime, side, x, w):
    """The operand an edge case names as the carrier of subnormal values."""
    return {"operands": (x if side == "x" else w,)} if regime == "low" else {}


def conv_case(case, fmt: str, regime: str, side: str = "x"):
    """One CONV_CASES row: (x, w, bias, res or None) and its rounding point.  Both operands get the same spread,
    sigma^2 = target / sqrt(K) (wide: r ~ sqrt(4000 / sqrt(K)) / 0.58).  low / high: the wide row at ``units_of(regime, fmt, side)``."""
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    taps = min(k, h) * min(k, w)                                  # of the k x k taps, those a centre pixel has inside the image
    base, un = BASE[regime], units_of(regime, fmt, side, 2.0 ** round(math.log2(math.sqrt(k * k / taps))) if regime == "high" else 1.0)
    g = torch.Generator().manual_seed(seed_of("conv", case, base))
    sig = math.sqrt(TARGET[base] / math.sqrt(cin * k * k))
    x = draw((n, cin, h, w), sig, g, un.ux, fmt)
    wt = draw((cout, cin, k, k), sig, g, un.uw, fmt)
    bias = _bias(cout, BIAS_R[base], un.prod, g)
    ho, wo = out_hw(h, w, k, stride, pad)
    res = _res((n, cout, ho, wo), RES_R[base], un, g, fmt) if has_res else None
    kw = _edge_kw(regime, side, x, wt)
    if regime == "high":
        lin = conv_bias_act_emulated(x, wt, bias, stride, pad, False, residual_bf=res, fmt="fp32")
        bias, kw["planted"] = plant_boundaries(lin, bias, relu)
    return (x, wt, bias, res), conv_exact("conv", x, wt, bias, stride, pad, relu, res, unit=un.out, fmt=fmt, **kw)


def cat_case(case, fmt: str, regime: str, side: str = "x"):
    """One CAT_CASES row: (x1, x2 [NHWC], wcat (cout, c1 + c2), bias) in _cat_tensors' layout, and its rounding point."""
    n, h, c1, h2, c2, s2, cout, relu, _tile = case
    base, un = BASE[regime], units_of(regime, fmt, side)
    g = torch.Generator().manual_seed(seed_of("cat", case, base))
    sig = math.sqrt(TARGET[base] / math.sqrt(c1 + c2))
    x1 = draw((n, c1, h, h), sig, g, un.ux, fmt)
    x2 = draw((n, c2, h2, h2), sig, g, un.ux, fmt)
    w1 = draw((cout, c1, 1, 1), sig, g, un.uw, fmt)
    w2 = draw((cout, c2, 1, 1), sig, g, un.uw, fmt)
    bias = _bias(cout, BIAS_R[base], un.prod, g)
    kw = {"operands": (x1, x2) if side == "x" else (w1, w2)} if regime == "low" else {}
    if regime == "high":
        lin = cat_exact("cat", x1, w1, x2, w2, bias, s2, False, unit=un.out, fmt=fmt).pre
        bias, kw["planted"] = plant_boundaries(lin, bias, bool(relu))
    st = cat_exact("cat", x1, w1, x2, w2, bias, s2, bool(relu), unit=un.out, fmt=fmt, **kw)
    dt = FORMATS[fmt].dtype
    tensors = (x1.permute(0, 2, 3, 1).contiguous().to(dt), x2.permute(0, 2, 3, 1).contiguous().to(dt),
               torch.cat([w1.view(cout, c1), w2.view(cout, c2)], 1).contiguous().to(dt), bias)
    return tensors, st


def gemm_case(shape, fmt: str, regime: str, device="cpu", side: str = "x"):
    """One HEAD_GEMMS row: (x (rows, K), w (cout, K), bias, res or None) in _gemm_tensors' layout on the host, and its rounding point
    computed on ``device``.  "dw" rows keep their zero padding of K; "dx" / "dw" rows keep their zero bias."""
    rows, k, cout, relu, has_res, kind = shape[:6]
    base, un = BASE[regime], units_of(regime, fmt, side)
    g = torch.Generator().manual_seed(seed_of("gemm", shape, base))
    keff = shape[6] if kind == "dw" else k
    sig = math.sqrt(TARGET[base] / math.sqrt(keff))
    x = draw((rows, k), sig, g, un.ux, fmt)
    w = draw((cout, k), sig, g, un.uw, fmt)
    if kind == "dw":
        x[:, shape[6]:] = 0
        w[:, shape[6]:] = 0
    bias = _bias(cout, BIAS_R[base], un.prod, g) if kind == "fwd" else torch.zeros(cout)
    res = _res((rows, cout), RES_R[base], un, g, fmt) if has_res else None
    dt = FORMATS[fmt].dtype
    kw = _edge_kw(regime, side, x, w)
    on = lambda t: None if t is None else t.to(device)                     # noqa: E731
    if regime == "high":         # the kernel adds whatever bias it is given: the boundary values are planted through it for "dx" / "dw" rows too
        from tests.head_kernels_reference import gemm_ref
        lin = gemm_ref(on(x[:, :]), on(w[:8]), on(bias[:8]), None if res is None else on(res[:, :8]), False).float().cpu()
        b8, kw["planted"] = plant_boundaries(lin, bias[:8], bool(relu))
        bias = torch.cat([b8, bias[8:]])
    st = gemm_exact("gemm", on(x), on(w), on(bias), on(res), bool(relu), unit=un.out, fmt=fmt, **kw)
    return (x.to(dt), w.to(dt), bias, res.to(dt) if has_res else None), st


def fp8_case(case, regime: str):
    """One FP8_CASES row with power-of-two scales: (xq, wq, bias, rq or None, (sx, sw, sr, sy)) in _fp8_tensors' layout (NHWC / OHWI
    e4m3) and its rounding point, in units of sy.  wide: the scale sx sw / sy puts the outputs' std near 250, so that part of them
    saturates at 448 and the rest is spread over the binades where e4m3 rounds; small: every output is an integer up to 16.
    low: ``fp8_low_case``."""
    from tests.kernel_cases import fp8_reference
    if regime == "low":
        return fp8_low_case(case)
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


def fp8_low_case(case):
    """One FP8_CASES row at the bottom of e4m3.  xq, wq and rq are lattices at unit 2^-9, integers up to 16: 1..7 are e4m3 subnormals,
    8..16 normal.  A product of two such integers reaches 256 units of 2^-18 while the smallest normal OUTPUT is 64 of them (sx sw / sy
    = 2^6 puts the outputs on 2^-12 of sy), so outputs on both sides of 2^-6 need few products per output: the operands are
    ``lattice``'s sparse draw with about two non-zero products per output (the small regime's way to stay in range).  sr / sy = 2^-3
    puts the residual on the same 2^-12; the bias is on it as well, and channel 0's bias adds 1.25 sy, a column of outputs in e4m3's
    normal range (|v| in [1, 2): step 2^-3)."""
    from tests.kernel_cases import fp8_reference
    n, h, w, cin, cout, k, stride, pad, relu, has_res, _tile = case
    g = torch.Generator().manual_seed(seed_of("fp8", case, "low"))
    kk = cin * k * k
    ho, wo = out_hw(h, w, k, stride, pad)
    u, unit = 2.0 ** -9, 2.0 ** -12
    d = math.sqrt(2.0 / kk)
    sx, sw = 2.0 ** -3, 2.0 ** -5
    sy = sx * sw * (u * u / unit)
    sr = (unit / u) * sy
    xq = lattice((n, h, w, cin), 16, g, d, u, "e4m3")
    wq = lattice((cout, k, k, cin), 16, g, d, u, "e4m3")
    bias = lattice((cout,), 16, g, fmt="fp16") * (unit * sy)
    bias[0] += 1.25 * sy
    rq = lattice((n, ho, wo, cout), 16, g, unit=u, fmt="e4m3") if has_res else None
    scales = (sx, sw, sr, sy)
    pre = fp8_reference(xq, wq, bias, rq, scales, stride, pad, bool(relu))
    b = fp8_reference(xq.abs(), wq.abs(), bias.abs(), None if rq is None else rq.abs(), scales, stride, pad, False)
    assert bool((pre.float().double() == pre).all())
    st = Exact("fp8", pre.float(), fp8_round(pre), float(b.max()) / unit, unit, "e4m3", operands=(xq, wq) + ((rq,) if has_res else ()))
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


def stem_case(n: int, regime: str, fmt: str = "bf16", side: str = "x"):
    """Lattice frames (N,3,224,224) fp32 and lattice folded stem weights (64,3,7,7) fp32, K = 147: (x, w, bias) and the rounding point.
    The kernel converts both to ``fmt`` itself (exactly: they are representable)."""
    base, un = BASE[regime], units_of(regime, fmt, side)
    g = torch.Generator().manual_seed(seed_of("stem", n, base))
    sig = math.sqrt(TARGET[base] / math.sqrt(147.0))
    x = draw((n, 3, 224, 224), sig, g, un.ux, fmt)
    wf = draw((64, 3, 7, 7), sig, g, un.uw, fmt)
    bias = _bias(64, BIAS_R[base], un.prod, g)
    kw = _edge_kw(regime, side, x, wf)
    if regime == "high":
        lin = conv_bias_act_emulated(x, wf, bias, 2, 3, False, fmt="fp32")
        bias, kw["planted"] = plant_boundaries(lin, bias, True)
    return (x, wf, bias), conv_exact("stem", x, wf, bias, 2, 3, True, unit=un.out, fmt=fmt, **kw)


def avgpool_case(shape, fmt: str = "bf16", unit: float = UX):
    """Lattice (N,H,W,C) input of the type and float32(exact sum) * float32(1 / HW), what avgpool_kernel computes.  fp16 with unit
    2^-24: every addend is an fp16 subnormal (up to 255 steps of the subnormal grid), the sum still exact in fp32."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed_of("avgpool", shape))
    x = lattice(shape, 255, g, unit=unit, fmt=fmt)
    s = x.double().view(n, h * w, c).sum(dim=1)
    assert float(x.abs().double().view(n, h * w, c).sum(dim=1).max()) / unit < LIMIT and unit >= FP32_MIN_NORMAL
    ref = s.to(torch.float32) * torch.tensor(1.0 / (h * w), dtype=torch.float32)
    return x.to(FORMATS[fmt].dtype), ref


class _Chain:
    """Stages of a fused chain, from the inputs: each stage reads the stored (rounded) value of the one before.

    Units: the chain's inputs are at ``ua``, the weights of the stages that read them at ``uw1``, the weights of the stages that read a
    stored intermediate at ``uwn``.  small / wide: UX, UW, UW.  low (fp16): 2^-13, 2^-14 and 1 -- the first stage runs on NORMAL
    operands and stores subnormal intermediates (multiples of 2^-27 rounded onto 2^-24), which the next stage re-reads from LDS or HBM
    against weights at unit 1, so every stage's outputs are multiples of 2^-27 again.  Stored identities are multiples of 2^-24."""

    def __init__(self, key, regime, fmt="bf16"):
        self.base = BASE[regime]
        self.g = torch.Generator().manual_seed(seed_of(key, self.base))
        self.regime, self.fmt = regime, fmt
        self.stages: List[Exact] = []
        if regime in REGIMES:
            self.ua, self.uw1, self.uwn, self.res_step = UX, UW, UW, 1
        elif regime == "low" and fmt == "fp16":
            self.ua, self.uw1, self.uwn, self.res_step = 2.0 ** -13, 2.0 ** -14, 1.0, 8
        else:
            raise ValueError(f"no {regime} chain cases for {fmt}")
        self.dt = FORMATS[fmt].dtype

    @property
    def u(self):
        """Unit of the first stage's outputs."""
        return self.ua * self.uw1

    def conv(self, name, x, x_unit, cout, k, stride, pad, relu, target, res=None, w=None, bias_r=None, w_unit=None, stored=False):
        """Draw weights and bias for ``x`` (values in ``x_unit``), append the stage, return (w, bias, stage).  ``stored``: x is an
        intermediate the kernel stored (low regime: the operand that carries the subnormal values)."""
        w_unit = (self.uwn if stored else self.uw1) if w_unit is None else w_unit
        if w is None:
            w = _w_for((cout, x.shape[1], k, k), target, _ms(x, x_unit), self.g, self.fmt, w_unit)
        u = x_unit * w_unit
        bias = _bias(cout, BIAS_R[self.base] if bias_r is None else bias_r, u, self.g)
        kw = {"operands": ((x,) if stored else ()) + ((res,) if res is not None else ())} if self.regime == "low" else {}
        st = conv_exact(name, x, w, bias, stride, pad, relu, res, unit=u, fmt=self.fmt, **kw)
        self.stages.append(st)
        return w, bias, st

    def act(self, shape, sigma, unit=None, nonneg=False):
        return draw(shape, sigma, self.g, self.ua if unit is None else unit, self.fmt, nonneg=nonneg)

    def stored(self, shape, sigma, unit, nonneg=False):
        """A stored tensor at the outputs' unit (an identity): integers of ``unit``, multiples of ``res_step``, exact in the type."""
        v = draw(shape, sigma, self.g, 1.0, self.fmt, nonneg=nonneg)
        if self.res_step > 1:
            v = torch.trunc(v / self.res_step) * self.res_step
        v = v * unit
        assert representable(v, self.fmt)
        return v


def _targets(regime, stages: int, emph: Optional[int]):
    """Output std each stage of a chain aims at.  The small regime bounds the PRODUCT of the stages' non-zero term counts (magnitudes
    multiply along the chain and every output must stay within 256 units), so one stage is chosen to be dense: the stages before
    ``emph`` stay near 3 units, ``emph`` aims at 40 (20 when stages follow it), and the stages after it add only a term or two of that
    size.  Default: the last."""
    regime = BASE[regime]
    if regime == "wide":
        return [INTER[regime]] * (stages - 1) + [LAST[regime]]
    emph = stages - 1 if emph is None else emph
    return [INTER[regime] if i < emph else 8.0 if i > emph else LAST[regime] if i == stages - 1 else 20.0 for i in range(stages)]


def _inter_r(regime):
    """(bias range, identity spread) of an intermediate stage."""
    return (1, 2.0) if BASE[regime] == "small" else (100, 150.0)


def tail_case(cmid, c1, shape, ds, regime, key=(), emph=None, fmt="bf16"):
    """A bottleneck tail (``bneck_tail_bf16``; c1 = 0: ``conv3_identity_tail3_bf16``): host tensors in the order of _tail_tensors
    (cmid 64: y2, w3, b3, w1, b1, idn | xin, wd, bd) or of _tail2_tensors / _tail3_inputs (y2, w3, b3, idn, w1, b1), NCHW / OIHW bf16,
    and the rounding points [identity,] out, y1n."""
    n, h, w = shape
    c = _Chain(("tail", cmid, c1, shape, ds, key), regime, fmt)
    base = c.base
    br, isig = _inter_r(regime)
    last = c1 == 0
    t_out, t_y1 = _targets(regime, 2, emph)
    y2 = c.act((n, cmid, h, w), math.sqrt(t_out / math.sqrt(cmid)) if not last else math.sqrt(TARGET[base] / math.sqrt(cmid)))
    u = c.u
    if ds:
        xin = c.act((n, cmid, h, w), 1.0 if base == "small" else 4.0)
        wd, bd, st_id = c.conv("identity", xin, c.ua, 4 * cmid, 1, 1, 0, False, isig, bias_r=br)
        idn = st_id.ref
    else:
        idn = c.stored((n, 4 * cmid, h, w), isig if not last else RES_R[base] * 0.58, u)
    w3, b3, st_out = c.conv("out", y2, c.ua, 4 * cmid, 1, 1, 0, True, t_out if not last else TARGET[base], res=idn,
                            bias_r=None if last else br)
    bf = c.dt
    if last:
        return (y2.to(bf), w3.to(bf), b3, idn.to(bf), None, None), c.stages
    w1, b1, _ = c.conv("y1n", st_out.ref, u, c1, 1, 1, 0, True, t_y1, stored=True)
    if cmid == 64:
        rest = (xin.to(bf), wd.to(bf), bd) if ds else (idn.to(bf),)
        return (y2.to(bf), w3.to(bf), b3, w1.to(bf), b1) + rest, c.stages
    return (y2.to(bf), w3.to(bf), b3, idn.to(bf), w1.to(bf), b1), c.stages


def _nhwc(t, dt=torch.bfloat16):
    return t.permute(0, 2, 3, 1).contiguous().to(dt)


def block_case(layer, n, c1, regime, ds=False, emph=None, fmt="bf16"):
    """A bottleneck body (``bneck_block1_bf16`` / ``bneck_block1_ds_bf16`` / ``bneck_block2_bf16``; c1 = 0: no chained conv1): host
    tensors in the order of _block1_tensors / _block2_tensors (t1, idn, w2, w3, w1, b2, b3, b1) or _block1_ds_tensors
    (t1, x, w2, w3, wd, w1, b2, b3, bd, b1), NHWC / OHWI bf16, and the rounding points t2, [identity,] out, [y1n]."""
    hw, cm = (56, 64) if layer == 1 else (28, 128)
    c = _Chain(("block", layer, n, c1, ds), regime, fmt)
    base = c.base
    br, isig = _inter_r(regime)
    t_t2, t_out, t_y1 = _targets(regime, 3, emph)
    t1 = c.act((n, cm, hw, hw), 1.0 if base == "small" else 4.0, nonneg=True)
    w2, b2, st2 = c.conv("t2", t1, c.ua, cm, 3, 1, 1, True, t_t2, bias_r=br)
    u2 = c.u
    u = u2 * c.uwn
    if ds:      # the block input and Wd: units whose product is the block output's (small / wide: u2 and UW; low: the chain inputs' units)
        xu, wdu = (u2, UW) if regime in REGIMES else (c.ua, c.uw1)
        x = c.act((n, cm, hw, hw), 1.0 if base == "small" else 4.0, unit=xu, nonneg=True)
        wd, bd, st_id = c.conv("identity", x, xu, 4 * cm, 1, 1, 0, False, isig, bias_r=br, w_unit=wdu)
        idn = st_id.ref
    else:
        idn = c.stored((n, 4 * cm, hw, hw), isig, u, nonneg=True)
    w3, b3, st_out = c.conv("out", st2.ref, u2, 4 * cm, 1, 1, 0, True, t_out, res=idn, bias_r=br, stored=True)
    dt = c.dt
    ohwi = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dt)       # noqa: E731
    if c1:
        w1, b1, _ = c.conv("y1n", st_out.ref, u, c1, 1, 1, 0, True, t_y1, stored=True)
        w1 = ohwi(w1)
    else:
        w1 = b1 = None
    if ds:
        return (_nhwc(t1, dt), _nhwc(x, dt), ohwi(w2), ohwi(w3), ohwi(wd), w1, b2, b3, bd, b1), c.stages
    return (_nhwc(t1, dt), _nhwc(idn, dt), ohwi(w2), ohwi(w3), w1, b2, b3, b1), c.stages


def cat_chain_case(n, regime, emph=None, fmt="bf16"):
    """``bneck_cat_chain_bf16``: host tensors in the order of _cat_chain_tensors (t2, x, w3, wd, bcat, w1, b1; NCHW / OIHW bf16) and
    the rounding points out (``conv_cat_emulated``), y1n."""
    c = _Chain(("cat_chain", n), regime, fmt)
    br, _ = _inter_r(regime)
    t_out, t_y1 = _targets(regime, 2, emph)
    sig = math.sqrt(t_out / math.sqrt(384.0))
    t2 = c.act((n, 128, 28, 28), sig)
    x = c.act((n, 256, 56, 56), sig)
    w3 = draw((512, 128, 1, 1), sig, c.g, c.uw1, fmt)
    wd = draw((512, 256, 1, 1), sig, c.g, c.uw1, fmt)
    u = c.u
    bcat = _bias(512, br, u, c.g)
    st = cat_exact("out", t2, w3, x, wd, bcat, 2, True, unit=u, fmt=fmt)
    c.stages.append(st)
    w1, b1, _ = c.conv("y1n", st.ref, u, 128, 1, 1, 0, True, t_y1, stored=True)
    bf = c.dt
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
                             f"got {float(got_f32[tuple(idx)])!r}, ref {float(ref[tuple(idx)])!r}, unrounded {float(st.pre[tuple(idx)])!r}; "
                             f"{describe_mismatch(got_f32, st)} ({st.report()})")


# ------------------------------------------------------------------------------------------------------------------------------
# the fused-chain cases the GPU file runs: id -> (runner in tests/test_kernels_gpu.py, its arguments, builder of (tensors, stages))
# ------------------------------------------------------------------------------------------------------------------------------
def chain_cases():
    """The dense stage of the small regime (``_targets``) rotates over a kernel's cases, so that each stage of each kernel is dense in one.
    A builder takes the regime and, optionally, the element type ("fp16" with the low regime)."""
    cases = {}
    for i, (shape, c1) in enumerate((((2, 7, 9), 64), ((1, 56, 56), 128), ((3, 5, 16), 64), ((5, 56, 56), 64))):
        for ds in (False, True):
            cases["tail1_%s_c%d_%s" % ("x".join(map(str, shape)), c1, "ds" if ds else "id")] = (
                "_run_bneck_tail", (shape, c1, ds), lambda r, f="bf16", a=(64, c1, shape, ds), e=i % 2: tail_case(*a, r, emph=e, fmt=f))
    for i, shape in enumerate(((2, 7, 9), (1, 28, 28), (3, 5, 16), (9, 28, 28))):
        cases["tail2_" + "x".join(map(str, shape))] = (
            "_run_bneck_tail_layer2", (shape,), lambda r, f="bf16", s=shape, e=i % 2: tail_case(128, 128, s, False, r, emph=e, fmt=f))
    for i, (shape, bp) in enumerate((((2, 7, 9), 0), ((1, 14, 14), 0), ((5, 14, 14), 33), ((20, 14, 14), 7))):
        cases["tail3_%s_bp%d" % ("x".join(map(str, shape)), bp)] = (
            "_run_bneck_tail_layer3", (shape, bp), lambda r, f="bf16", s=shape, b=bp, e=i % 2: tail_case(256, 256, s, False, r, key=b, emph=e, fmt=f))
    for n in (1, 5):
        cases["tail3_last_n%d" % n] = ("_run_layer3_last_block", (n,), lambda r, f="bf16", n=n: tail_case(256, 0, (n, 14, 14), False, r, fmt=f))
    for i, n in enumerate((1, 3, 20)):
        for c1 in (64, 128):
            cases["block1_n%d_c%d" % (n, c1)] = ("_run_bneck_block1", (n, c1), lambda r, f="bf16", n=n, c=c1, e=i: block_case(1, n, c, r, emph=e, fmt=f))
        cases["block1_ds_n%d" % n] = ("_run_bneck_block1_ds", (n,), lambda r, f="bf16", n=n, e=i: block_case(1, n, 64, r, ds=True, emph=e, fmt=f))
    for i, n in enumerate((1, 3, 70)):
        for chain in (False, True):
            cases["block2_n%d_%s" % (n, "chained" if chain else "last")] = (
                "_run_bneck_block2", (n, chain), lambda r, f="bf16", n=n, e=i if chain else min(i, 1): block_case(2, n, 128, r, emph=e, fmt=f))
    for i, n in enumerate((1, 3, 37)):
        cases["cat_chain_n%d" % n] = ("_run_bneck_cat_chain", (n,), lambda r, f="bf16", n=n, e=i % 2: cat_chain_case(n, r, emph=e, fmt=f))
    return cases


CHAIN_CASES = chain_cases()
# the chains the low regime runs in fp16: one tail per layer kind (identity and downsample forms of layer1's), the three bodies, the chain
LOW_CHAINS = ("tail1_2x7x9_c64_id", "tail1_3x5x16_c64_ds", "tail2_2x7x9", "tail3_2x7x9_bp0", "tail3_5x14x14_bp33", "tail3_last_n1",
              "block1_n1_c64", "block1_n3_c128", "block1_ds_n1", "block2_n1_chained", "block2_n3_last", "cat_chain_n1", "cat_chain_n3")
STEM_N = (1, 3)
AVGPOOL_SHAPES = ((4, 7, 7, 2048), (1, 3, 3, 8))
