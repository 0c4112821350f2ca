"""The lifting head's own kernels through the C ABI against plain fp64 references (tests/head_kernels_reference.py), at the shapes, element
types and edges where they can go wrong: GroupNorm slabs whose mean is large against their spread, 16-bit rounding ties and saturation,
the overflow check's exact bit patterns, reductions at the drivers' sizes, AdamW's bias corrections, and the head's GEMMs at the row
counts and K the head launches them with.

Bars.  A 16-bit result may differ from the fp64 value by one rounding (half an ulp) plus what the kernel's fp32 arithmetic adds; where
that arithmetic is the reference's own (GroupNorm), the allowance is 4x torch's fp32 deviation from fp64 on the same input, floored at
2^-20 of the result's scale.  Reductions get the worst-case bound of their summation structure, and a second input whose partial sums
are all exact in fp32, where the result must be the fp64 value itself.  The GEMMs keep tests/test_kernels_gpu.py's bar."""
import pytest
import torch

from tests import head_kernels_reference as R
from tests.kernel_cases import HEAD_GEMMS, _gn_inputs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _ok(lib, rc, what):
    assert rc == 0, f"{what}: {lib.r50_last_error(None)}"
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int16)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------- a. GroupNorm ------------------------------------------------------
GN_SHAPES = [(4, 40, 1024, 32), (3, 40, 256, 32), (2, 40, 512, 2), (3, 1, 1024, 32), (3, 2, 256, 32), (3, 3, 512, 2)]   # b, t, c, groups
GN_RATIOS = {1: (0, 30, 300, 1000), 0: (0, 10, 30, 100)}      # slab mean / std; bf16 stops at 100: its slabs still hold ~8 distinct values
GN_CASES = [(et, r, s) for et in (1, 0) for r in GN_RATIOS[et] for s in GN_SHAPES]


def _gn_id(case):
    et, r, (b, t, c, g) = case
    return f"{'fp16' if et else 'bf16'}-ratio{r}-b{b}t{t}c{c}g{g}"


@pytest.mark.parametrize("case", GN_CASES, ids=_gn_id)
def test_gn_forward_against_fp64(lib, case):
    """r50_op_gn_relu_causal3 and r50_op_gn_relu_causal3_tm (t0 = 0 and t - 1) within one rounding of fp64 + 4x torch's fp32 error."""
    et, ratio, (b, t, c, groups) = case
    dt = R.DTYPE[et]
    x, gamma, beta, _ = _gn_inputs(et, ratio, (b, t, c, groups))
    ref, abs_term = R.gn_forward_bar(x, groups, gamma, beta, EPS)             # (b, t, 3c)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    buf = torch.full((b * t + 4, 3 * c), 7.0, dtype=dt, device=DEV)             # guard band behind the output
    _ok(lib, lib.r50_op_gn_relu_causal3(xd.data_ptr(), b, t, c, groups, gd.data_ptr(), bd.data_ptr(), EPS, buf.data_ptr(), et, _s()), "gn")
    assert bool((buf[b * t:] == 7.0).all()), "wrote past the end of the output"
    R.assert_within_rounding(buf[: b * t].cpu().view(b, t, 3 * c), ref, et, abs_term, "gn_relu_causal3")
    x_tm = xd.transpose(0, 1).contiguous()
    for t0 in sorted({0, t - 1}):
        rows = (t - t0) * b
        out = torch.full((rows + 4, 3 * c), 7.0, dtype=dt, device=DEV)
        _ok(lib, lib.r50_op_gn_relu_causal3_tm(x_tm.data_ptr(), b, t, t0, c, groups, gd.data_ptr(), bd.data_ptr(), EPS, out.data_ptr(), et,
                                               _s()), "gn_tm")
        assert bool((out[rows:] == 7.0).all()), f"t0={t0}: wrote past the end of the output"
        got = out[:rows].cpu().view(t - t0, b, 3 * c).transpose(0, 1)
        R.assert_within_rounding(got, ref[:, t0:], et, abs_term, f"gn_relu_causal3_tm t0={t0}")


def _gn_bwd(lib, kind, dr, x, b, t, t0, c, groups, gamma, beta, add, et):
    """One backward launch: kind "bm" (dr, x, add batch-major (b, t, .)) or "tm" (the same tensors, passed time-major; dr only for the rows
    t0.. the forward emitted).  Returns dx (b, t, c) on the CPU and the parts (2, b, c); checks the guard band behind dx."""
    tm = lambda v: v.transpose(0, 1).contiguous()                               # noqa: E731  (b, t, .) -> (t, b, .)
    dx = torch.full((t * b + 4, c), 7.0, dtype=x.dtype, device=DEV)
    part = torch.empty((2, b, c), device=DEV)
    if kind == "bm":
        drd, xd, ad = dr.to(DEV), x.to(DEV), add.to(DEV)
        rc = lib.r50_op_gn_relu_causal3_bwd(drd.data_ptr(), xd.data_ptr(), b, t, c, groups, gamma.data_ptr(), beta.data_ptr(), EPS,
                                            ad.data_ptr(), dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), et, _s())
    else:
        drd, xd, ad = tm(dr.to(DEV))[t0:].contiguous(), tm(x.to(DEV)), tm(add.to(DEV))
        rc = lib.r50_op_gn_relu_causal3_tm_bwd(drd.data_ptr(), xd.data_ptr(), b, t, t0, c, groups, gamma.data_ptr(), beta.data_ptr(), EPS,
                                               ad.data_ptr(), dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), et, _s())
    _ok(lib, rc, f"gn bwd {kind}")
    assert bool((dx[t * b:] == 7.0).all()), f"gn bwd {kind} t0={t0}: wrote past the end of dx"
    got = dx[: t * b].cpu().view(b, t, c) if kind == "bm" else dx[: t * b].cpu().view(t, b, c).transpose(0, 1)
    return got, part.cpu()


@pytest.mark.parametrize("case", GN_CASES, ids=_gn_id)
def test_gn_backward_against_fp64(lib, case):
    """r50_op_gn_relu_causal3_bwd and _tm_bwd (t0 = 0 and t - 1): dx + add within one rounding of fp64 autograd + 4x torch's fp32
    autograd error; the per-sample dgamma / dbeta parts within 4x that error.  Gradient taps that read an element whose pre-activation lies
    within 2^-10 of the ReLU's edge are zeroed: there fp32 and fp64 may legitimately pick different sides."""
    et, ratio, (b, t, c, groups) = case
    dt = R.DTYPE[et]
    x, gamma, beta, g = _gn_inputs(et, ratio, (b, t, c, groups))
    amb = R.gn_relu_ambiguous(x, groups, gamma, beta, EPS, 2.0 ** -10)
    dr_all = R.zero_taps_of(torch.randn(b, t, 3 * c, generator=g), amb).to(dt)
    add = torch.randn(b, t, c, generator=g).to(dt)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    for t0 in sorted({0, t - 1}):
        dr = dr_all.clone()
        dr[:, :t0] = 0                                                          # the rows the forward did not emit carry no gradient
        dx64, pg64, pb64 = R.gn_backward(x.double(), dr.double(), groups, gamma.double(), beta.double(), EPS)
        dx32, pg32, pb32 = R.gn_backward(x.float(), dr.float(), groups, gamma.float(), beta.float(), EPS)
        ref = dx64 + add.double()
        abs_dx = R.bar_from(dx32 + add.float(), ref)
        for kind in (("tm",) if t0 else ("bm", "tm")):
            got, part = _gn_bwd(lib, kind, dr, x, b, t, t0, c, groups, gd, bd, add, et)
            R.assert_within_rounding(got, ref, et, abs_dx, f"gn bwd {kind} t0={t0} dx")
            for name, p, p64, p32 in (("dgamma", part[0], pg64, pg32), ("dbeta", part[1], pb64, pb32)):
                d = float((p.double() - p64).abs().max())
                lim = R.bar_from(p32, p64)
                assert d <= lim, f"gn bwd {kind} t0={t0} {name}: max |d| {d:.3g} > {lim:.3g}"


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(3, 40, 1024, 32), (2, 3, 256, 32), (2, 40, 512, 2)], ids=lambda s: "b%dt%dc%dg%d" % s)
def test_gn_constant_slabs(lib, et, shape):
    """Every (sample, group) slab constant (0.75, -2.5 or 1000): variance 0, rstd = 1/sqrt(eps).  A constant slab's sums are exact in fp32,
    so the forward is relu(beta) rounded once, bit for bit, batch- and time-major.  Backward: xh = 0, so dgamma_part is exactly 0 and
    dx = rstd (g - mean g) + add with g = dy gamma; bars from the summation structure: dx within one rounding + 64 u rstd max sum|taps|
    |gamma|, dbeta_part (per channel a sum over t of up to 5 taps each) within 48 u of the sum of the taps' magnitudes."""
    b, t, c, groups = shape
    dt = R.DTYPE[et]
    g = torch.Generator().manual_seed(b * t + c + et)
    level = torch.tensor([0.75, -2.5, 1000.0])[torch.randint(0, 3, (b, 1, groups, 1), generator=g)]
    x = level.expand(b, t, groups, c // groups).reshape(b, t, c).to(dt)
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    want = R.causal3_rows(R.round16(beta.clamp_min(0), et).view(1, 1, c).expand(b, t, c))
    out = torch.empty(b * t, 3 * c, dtype=dt, device=DEV)
    _ok(lib, lib.r50_op_gn_relu_causal3(xd.data_ptr(), b, t, c, groups, gd.data_ptr(), bd.data_ptr(), EPS, out.data_ptr(), et, _s()), "gn")
    assert torch.equal(_bits(out.cpu().view(b, t, 3 * c)), _bits(want)), "batch-major"
    x_tm = xd.transpose(0, 1).contiguous()
    _ok(lib, lib.r50_op_gn_relu_causal3_tm(x_tm.data_ptr(), b, t, 0, c, groups, gd.data_ptr(), bd.data_ptr(), EPS, out.data_ptr(), et, _s()),
        "gn_tm")
    assert torch.equal(_bits(out.cpu().view(t, b, 3 * c).transpose(0, 1)), _bits(want)), "time-major"
    dr = (torch.randn(b, t, 3 * c, generator=g) * 2.0 ** -6).to(dt)           # rstd = 316: dx stays O(1)
    add = torch.randn(b, t, c, generator=g).to(dt)
    dx64, _, pb64 = R.gn_backward(x.double(), dr.double(), groups, gamma.double(), beta.double(), EPS)
    src = R.causal3_sources(t)
    taps = torch.zeros(b, t, c, dtype=torch.float64)                           # per element, the sum of |dr| over the taps that read it
    for k in range(3):
        taps.index_add_(1, src[:, k], dr.double().abs()[:, :, k * c: (k + 1) * c])
    taps = taps * (beta.double() > 0)
    rstd = 1.0 / EPS ** 0.5
    for kind in ("bm", "tm"):
        got, part = _gn_bwd(lib, kind, dr, x, b, t, 0, c, groups, gd, bd, add, et)
        R.assert_within_rounding(got, dx64 + add.double(), et, 64 * R.U32 * rstd * float((taps * gamma.double().abs()).max()), f"{kind} dx")
        assert bool((part[0] == 0).all()), f"{kind}: dgamma_part of a constant slab is not 0"
        assert bool(((part[1].double() - pb64).abs() <= 48 * R.U32 * taps.sum(1)).all()), f"{kind}: dbeta_part"


# ---------------------------------------------------------------- b. casts and row ops ----------------------------------------------
def _ties(et, n, g):
    """n fp32 values exactly halfway between two adjacent finite 16-bit values (both parities of the lower neighbour).  fp16: every
    fourth one lies on the subnormal grid, between the bit patterns 0x0000 .. 0x03ff and their successors (0x0000: half the smallest
    subnormal, which goes to +-0; 0x03ff: the tie with the smallest normal)."""
    dt = R.DTYPE[et]
    lim = 0x7bfe if et else 0x7f7e                                              # below the largest finite magnitude
    bits = torch.randint(0x0400 if et else 0x0080, lim, (n,), generator=g, dtype=torch.int32)
    if et:
        sub = torch.randint(0x0000, 0x0400, (n,), generator=g, dtype=torch.int32)
        bits = torch.where(torch.arange(n) % 4 == 3, sub, bits)
    lo = bits.to(torch.int16).view(dt).float()
    hi = (bits + 1).to(torch.int16).view(dt).float()
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (lo + hi) / 2 * sign


def _cast_input(et, rows, c, g):
    x = torch.randn(rows, c, generator=g) * 3
    flat = x.view(-1)
    k = flat.numel() // 3
    flat[:k] = _ties(et, k, g)
    # the bottom of fp16, both signs: around the smallest normal 2^-14, around half the smallest subnormal 2^-25 (below it and at it:
    # +-0, the sign kept; above it: +-2^-24), and far below; for bf16 these are ordinary normal values
    e = 2.0 ** -12
    edge = torch.tensor([2.0 ** -14 * (1 - e), 2.0 ** -14, 2.0 ** -14 * (1 + e), 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -24, 1.5 * 2.0 ** -24,
                         2.0 ** -25 * (1 - e), 2.0 ** -25, 2.0 ** -25 * (1 + e), 2.0 ** -26, 2.0 ** -30, 2.0 ** -40])
    edge = torch.cat([edge, -edge])
    m = min((flat.numel() - k) // 2, 20 * edge.numel())
    flat[k: k + m] = edge.repeat(m // edge.numel() + 1)[:m]
    return x


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(40, 2048, 2048), (40, 51, 64), (33, 33, 34), (1, 1, 2)], ids=lambda s: "r%d_c%d_cp%d" % s)
def test_cast_rows_rounds_to_nearest_even(lib, et, shape):
    """fp32 (rows, c) -> 16-bit (rows, cpad): round to nearest even, a third of the inputs exact ties (fp16: a quarter of them on the
    subnormal grid), values around fp16's smallest normal and around half its smallest subnormal (+-0 with the sign kept, or +-2^-24);
    zero columns c..cpad-1."""
    rows, c, cpad = shape
    dt = R.DTYPE[et]
    g = torch.Generator().manual_seed(rows * 7 + c + et)
    x = _cast_input(et, rows, c, g)
    want = torch.zeros(rows, cpad, dtype=dt)
    want[:, :c] = R.round16(x, et)
    buf = torch.full((rows * cpad + 64,), 7.0, dtype=dt, device=DEV)
    xd = x.to(DEV)
    _ok(lib, lib.r50_op_cast_rows(xd.data_ptr(), rows, c, buf.data_ptr(), cpad, et, _s()), "cast_rows")
    assert torch.equal(_bits(buf[: rows * cpad].cpu().view(rows, cpad)), _bits(want)), "cast_rows differs from round-to-nearest-even"
    assert bool((buf[rows * cpad:] == 7.0).all()), "wrote past the end of the output"


def _overflow(lib, x16, et):
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    _ok(lib, lib.r50_op_check_overflow16(x16.data_ptr(), x16.numel(), found.data_ptr(), et, _s()), "check_overflow16")
    return int(found)


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
def test_cast_rows_saturates_and_the_overflow_check_sees_it(lib, et):
    """fp16: values at and beyond +-65504 (and +-inf) come out as +-65504, never as infinity, and check_overflow16 flags them; bf16 keeps
    IEEE rounding (huge finite values stay finite, infinities stay infinite).  A NaN input must come out flagged: NaN, or for fp16 the
    saturated value the clamp makes of it."""
    dt = R.DTYPE[et]
    big = [65504.0, 65519.0, 65520.0, 1e5, 3e38, float("inf")]
    vals = torch.tensor(big + [-v for v in big] + [1.0, -2.5, 0.0, 65503.0 if et else 1e38])
    x = vals.view(1, -1).contiguous()
    out = torch.empty(1, vals.numel(), dtype=dt, device=DEV)
    xd = x.to(DEV)
    _ok(lib, lib.r50_op_cast_rows(xd.data_ptr(), 1, vals.numel(), out.data_ptr(), vals.numel(), et, _s()), "cast_rows")
    assert torch.equal(_bits(out.cpu()), _bits(R.round16(x, et))), (out.cpu(), R.round16(x, et))
    if et:
        assert bool(torch.isfinite(out).all()), "fp16 conversion produced an infinity"
    assert _overflow(lib, out[:, : len(big)].contiguous(), et) == 1
    assert _overflow(lib, out[:, len(big): 2 * len(big)].contiguous(), et) == 1
    assert _overflow(lib, out[:, 2 * len(big): 2 * len(big) + 3].contiguous(), et) == 0
    nan = torch.tensor([[1.0, float("nan"), -3.0, float("nan")]])
    out = torch.empty(1, 4, dtype=dt, device=DEV)
    nd = nan.to(DEV)
    _ok(lib, lib.r50_op_cast_rows(nd.data_ptr(), 1, 4, out.data_ptr(), 4, et, _s()), "cast_rows nan")
    o = out.cpu().float()[0]
    assert o[0] == 1.0 and o[2] == -3.0
    for v in (o[1], o[3]):
        assert bool(torch.isnan(v)) or (et == 1 and abs(float(v)) == 65504.0), f"NaN came out as {float(v)}"
    assert _overflow(lib, out[:, 1:2].contiguous(), et) == 1 and _overflow(lib, out[:, 3:4].contiguous(), et) == 1


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
def test_concat_pad(lib, et):
    """[phi (rows, 1024) | y (rows, 51) fp32 | 0] -> (rows, 1088): phi's bits, y rounded to nearest even (ties included), a zero tail that
    overwrites whatever the buffer held."""
    rows, d, ny, dp = 40, 1024, 51, 1088
    dt = R.DTYPE[et]
    g = torch.Generator().manual_seed(11 + et)
    phi = torch.randn(rows, d, generator=g).to(dt)
    y = _cast_input(et, rows, ny, g)
    buf = torch.full((rows * dp + 64,), 7.0, dtype=dt, device=DEV)
    phid, yd = phi.to(DEV), y.to(DEV)
    _ok(lib, lib.r50_op_concat_pad(phid.data_ptr(), d, yd.data_ptr(), ny, rows, buf.data_ptr(), dp, et, _s()), "concat_pad")
    got = buf[: rows * dp].cpu().view(rows, dp)
    assert torch.equal(_bits(got[:, :d]), _bits(phi))
    assert torch.equal(_bits(got[:, d: d + ny]), _bits(R.round16(y, et)))
    assert bool((_bits(got[:, d + ny:]) == 0).all()), "padding columns are not +0"
    assert bool((buf[rows * dp:] == 7.0).all()), "wrote past the end of the output"


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("dp", [64, 1088])
def test_add_rows(lib, et, dp):
    """y (rows, 51) fp32 += the first 51 columns of dy (rows, dp): one fp32 rounding of the exact sum; the other columns are not read."""
    rows, ny = 40, 51
    dt = R.DTYPE[et]
    g = torch.Generator().manual_seed(dp + et)
    y = torch.randn(rows, ny, generator=g)
    dy = (torch.randn(rows, dp, generator=g) * 0.1).to(dt)
    dy[:, ny:] = float("nan")                                                   # must not leak into y
    # a quarter of the sums cancel into fp16's subnormal range: two normal addends, y = -dy + k 2^-24 (exact in fp32: |dy| < 1), so the
    # exact sum k 2^-24, k in -1023 .. 1023, must come out as it is (k = 0: +0)
    kk = torch.randint(-1023, 1024, (rows, ny), generator=g)
    cancel = (torch.rand(rows, ny, generator=g) < 0.25) & (dy[:, :ny].float().abs() < 1) & (dy[:, :ny].float().abs() >= 2.0 ** -14)
    y = torch.where(cancel, (-dy[:, :ny].double() + kk.double() * 2.0 ** -24).float(), y)
    assert int(cancel.sum()) > 100 and bool(((y.double() + dy[:, :ny].double())[cancel] == kk.double()[cancel] * 2.0 ** -24).all())
    buf = torch.full((rows * ny + 64,), 7.0, device=DEV)
    buf[: rows * ny] = y.view(-1).to(DEV)
    dyd = dy.to(DEV)
    _ok(lib, lib.r50_op_add_rows(buf.data_ptr(), ny, dyd.data_ptr(), dp, rows, et, _s()), "add_rows")
    want = (y.double() + dy[:, :ny].double()).float()
    assert torch.equal(buf[: rows * ny].cpu().view(rows, ny).view(torch.int32), want.view(torch.int32))
    assert bool((buf[rows * ny:] == 7.0).all())


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
def test_relu_bwd_mask_scale_grad_accum(lib, et):
    """Each is one fp32 product of the 16-bit value and the fp32 scale, rounded once to 16 bits (relu_bwd, mask_scale) or added in fp32
    (grad_accum): bit-equal to that emulation, and within one 16-bit rounding + one fp32 rounding of fp64.  n spans more than one grid."""
    dt = R.DTYPE[et]
    n = 256 * 8192 + 1001
    g = torch.Generator().manual_seed(21 + et)
    scale = 1.0 / 0.9                                                           # dropout's 1 / (1 - p): not a power of two
    s32 = _f32(scale)
    act = torch.randn(n, generator=g).to(dt)
    act[::97] = 0.0                                                             # act == 0 is not > 0
    dy = (torch.randn(n, generator=g) * 4).to(dt)
    dyd, actd = dy.to(DEV), act.to(DEV)
    _ok(lib, lib.r50_op_relu_bwd(dyd.data_ptr(), actd.data_ptr(), scale, n, et, _s()), "relu_bwd")
    want = torch.where(act.float() > 0, R.round16(dy.float() * s32, et).float(), torch.zeros(()))
    assert torch.equal(_bits(dyd.cpu()), _bits(want.to(dt)))
    exact = torch.where(act.double() > 0, dy.double() * s32, torch.zeros((), dtype=torch.float64))
    got = dyd.cpu().double()
    assert bool(((got - exact).abs() <= 0.5 * R.ulp16(torch.maximum(got.abs(), exact.abs()), et) + R.U32 * exact.abs()).all())
    mask = (torch.rand(n, generator=g) > 0.1).to(torch.uint8)
    h = (torch.randn(n, generator=g) * 4).to(dt)
    hd, maskd = h.to(DEV), mask.to(DEV)
    _ok(lib, lib.r50_op_mask_scale(hd.data_ptr(), maskd.data_ptr(), scale, n, et, _s()), "mask_scale")
    want = torch.where(mask.bool(), R.round16(h.float() * s32, et).float(), torch.zeros(()))
    assert torch.equal(_bits(hd.cpu()), _bits(want.to(dt)))
    for acc in (0, 1):
        dst0 = torch.randn(n, generator=g)
        dst = dst0.to(DEV)
        _ok(lib, lib.r50_op_grad_accum(hd.data_ptr(), 0.25, dst.data_ptr(), n, acc, et, _s()), "grad_accum")
        want = (dst0 if acc else torch.zeros(n)) + hd.cpu().float() * 0.25     # one fp32 rounding of the exact sum
        assert torch.equal(dst.cpu(), want), f"grad_accum accumulate={acc}"


def _exact_grid(shape, g, step, lim):
    """Values k * step with |k * step| < lim: sums of up to 10240 of them are exact in fp32 for the step / lim used below."""
    k = int(lim / step)
    return torch.randint(-k + 1, k, shape, generator=g).double() * step


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("cols", [51, 1024])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_colsum_at_driver_rows(lib, et, cols, accumulate):
    """r50_op_colsum over 10240 rows of a (rows, ld > cols) matrix.  16 row groups of 640 rows summed in order, 16 partials in order, one
    scale and one add: |error| <= (640 + 16 + 2) u sum|x| |scale| + u |out|.  On values whose sums are exact in fp32 the result is exact."""
    rows, ld = 10240, cols + 64
    dt = R.DTYPE[et]
    g = torch.Generator().manual_seed(cols + 2 * accumulate + et)
    for exact in (False, True):
        x = (_exact_grid((rows, ld), g, 2.0 ** -8 if et else 2.0 ** -5, 4.0) if exact else torch.randn(rows, ld, generator=g) * 2).to(dt)
        out0 = _exact_grid((cols,), g, 2.0 ** -8, 8.0).float() if exact else torch.randn(cols, generator=g)
        scale = 0.5 if exact else 0.37
        out = torch.cat([out0, torch.full((64,), 7.0)]).to(DEV)
        xd = x.to(DEV)
        _ok(lib, lib.r50_op_colsum(xd.data_ptr(), rows, cols, ld, scale, out.data_ptr(), accumulate, et, _s()), "colsum")
        got = out[:cols].cpu().double()
        s32 = _f32(scale)
        ref = (out0.double() if accumulate else 0) + s32 * x[:, :cols].double().sum(0)
        if exact:
            assert torch.equal(got, ref), f"colsum exact sums: max |d| {float((got - ref).abs().max())}"
        else:
            bound = 658 * R.U32 * x[:, :cols].double().abs().sum(0) * s32 + R.U32 * got.abs() + 1e-30
            d = (got - ref).abs()
            assert bool((d <= bound).all()), f"colsum: max |d| / bound {float((d / bound).max()):.3g}"
        assert bool((out[cols:] == 7.0).all())


@pytest.mark.parametrize("cols", [51, 1024])
def test_colsum_f32_at_driver_rows(lib, cols):
    """r50_op_colsum_f32 over 10240 rows (the GroupNorm parameter parts of a B 256 x T 40 step): rows summed in order per column."""
    rows = 10240
    g = torch.Generator().manual_seed(cols)
    for exact, accumulate in ((False, 0), (False, 1), (True, 1)):
        x = (_exact_grid((rows, cols), g, 2.0 ** -8, 4.0) if exact else torch.randn(rows, cols, generator=g)).float()
        out0 = torch.randn(cols, generator=g).round()
        out = torch.cat([out0, torch.full((64,), 7.0)]).to(DEV)
        xd = x.to(DEV)
        _ok(lib, lib.r50_op_colsum_f32(xd.data_ptr(), rows, cols, 2.0, out.data_ptr(), accumulate, _s()), "colsum_f32")
        got = out[:cols].cpu().double()
        ref = (out0.double() if accumulate else 0) + 2.0 * x.double().sum(0)
        if exact:
            assert torch.equal(got, ref)
        else:
            bound = (rows + 1) * R.U32 * 2.0 * x.double().abs().sum(0) + R.U32 * got.abs()
            d = (got - ref).abs()
            assert bool((d <= bound).all()), f"colsum_f32: max |d| / bound {float((d / bound).max()):.3g}"
        assert bool((out[cols:] == 7.0).all())


# ---------------------------------------------------------------- c. the overflow check -----------------------------------------------
FLAGGED = {1: [0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00, 0xfe00, 0x7c01], 0: [0x7f80, 0xff80, 0x7fc0, 0xffc0, 0x7f81]}
NOT_FLAGGED = {1: [0x7bfe, 0xfbfe], 0: [0x7f7f, 0xff7f]}


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
def test_check_overflow16_bit_patterns(lib, et):
    """fp16 flags |x| >= 0x7bff (65504: what a saturated conversion leaves), inf and NaN; bf16 flags inf and NaN only.  One bad element at
    index 0, at the last index of an n that is not a multiple of 256, and beyond the first grid's span (8192 workgroups x 256)."""
    n_small, n_big = 5001, 256 * 8192 + 3000
    g = torch.Generator().manual_seed(5 + et)
    bits = torch.randint(-32768, 32768, (n_big,), generator=g, dtype=torch.int32)
    ab = bits & 0x7fff
    bad = (ab >= 0x7bff) if et else ((ab & 0x7f80) == 0x7f80)
    bits = torch.where(bad, bits & 0x03ff, bits)                                # random finite, unflagged background
    x = bits.to(torch.int16).to(DEV)
    x16 = x.view(R.DTYPE[et])
    assert _overflow(lib, x16, et) == 0
    found = torch.ones(1, dtype=torch.int32, device=DEV)                        # found |= ...: a raised flag stays raised
    _ok(lib, lib.r50_op_check_overflow16(x16.data_ptr(), n_big, found.data_ptr(), et, _s()), "check_overflow16")
    assert int(found) == 1
    for n, idx in ((n_small, 0), (n_small, n_small - 1), (n_big, 256 * 8192 + 1234), (n_big, n_big - 1)):
        for pat in FLAGGED[et] + NOT_FLAGGED[et]:
            keep = x[idx].clone()
            x[idx] = torch.tensor(pat, dtype=torch.int32).to(torch.int16)
            got = _overflow(lib, x16[:n], et)
            x[idx] = keep
            assert got == (pat in FLAGGED[et]), f"pattern {pat:#06x} at {idx} of {n}: flag {got}"
    x[n_small] = 0x7c00 if et else 0x7f80                                       # just past n: must not be read
    assert _overflow(lib, x16[:n_small], et) == 0


# ---------------------------------------------------------------- d. reductions at driver sizes --------------------------------------
def test_mse_loss_grad_at_driver_size(lib):
    """n = 256 * 40 * 51 (B 256 x T 40): one workgroup, 680 joints per thread in order, a tree of 8 levels.  dy: two fp32 roundings of
    2 (y - gt) / n * loss_scale (loss_scale a power of two); both losses are sums of non-negative terms, so |rel error| <= (680 + 8 + 6) u.
    On a grid where every partial sum is exact, loss[0] is the fp64 mean rounded once."""
    n = 256 * 40 * 51
    g = torch.Generator().manual_seed(17)
    for exact in (False, True):
        if exact:
            gt = _exact_grid((n,), g, 2.0 ** -3, 4.0).float()
            y = gt + _exact_grid((n,), g, 2.0 ** -3, 0.5).float()
        else:
            y, gt = torch.randn(n, generator=g), torch.randn(n, generator=g)
        yd, gtd = y.to(DEV), gt.to(DEV)
        dy = torch.full((n + 64,), 7.0, device=DEV)
        loss = torch.empty(2, device=DEV)
        _ok(lib, lib.r50_op_mse_loss_grad(yd.data_ptr(), gtd.data_ptr(), n, 1024.0, dy.data_ptr(), loss.data_ptr(), _s()), "mse_loss_grad")
        d64 = y.double() - gt.double()
        want = 2.0 * d64 / n * 1024.0
        got = dy[:n].cpu().double()
        assert bool(((got - want).abs() <= 2.01 * R.U32 * want.abs()).all()), "dy beyond two fp32 roundings"
        assert bool((dy[n:] == 7.0).all())
        mse = (d64 ** 2).mean()
        mpjpe = d64.view(-1, 3).norm(dim=1).mean()
        tol = 694 * R.U32
        assert abs(float(loss[0]) - float(mse)) <= tol * float(mse), (float(loss[0]), float(mse))
        assert abs(float(loss[1]) - float(mpjpe)) <= (tol + 2 * R.U32) * float(mpjpe), (float(loss[1]), float(mpjpe))
        if exact:
            assert float(loss[0]) == _f32(float(mse))


# ---------------------------------------------------------------- e. AdamW ------------------------------------------------------------
@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [5001, 256 * 8192 + 777])
def test_adamw_against_fp64_torch(lib, et, n):
    """Steps 1 and 10^4 (bias corrections far from and close to 1), weight decay on and off, lr = 0 (p unchanged), and the skip flag,
    against torch.optim.AdamW in fp64 from the same fp32 state.  About 20 fp32 roundings feed the update: |dp| <= 4u (|p0| + |p|) + 24u
    lr/bc1 (b1 |m0| + (1 - b1) |g|) / denom (the terms of m, which may cancel); m and v within 3u / 4u of their terms.  p16 is p rounded
    to nearest even."""
    dt = R.DTYPE[et]
    g = torch.Generator().manual_seed(n % 1000 + et)
    b1, b2, eps = 0.9, 0.999, 1e-8
    b1f, b2f = _f32(b1), _f32(b2)
    for step, lr, wd in ((1, 1e-3, 1e-2), (10_000, 1e-3, 1e-2), (1, 1e-3, 0.0), (10_000, 0.0, 1e-2)):
        p0 = torch.randn(n, generator=g)
        grad = torch.randn(n, generator=g) * 1e-2
        if step == 1:
            m0, v0 = torch.zeros(n), torch.zeros(n)
        else:
            m0 = torch.randn(n, generator=g) * 1e-2
            v0 = torch.rand(n, generator=g) * 1e-4
        p, m, v, gd = p0.to(DEV), m0.to(DEV), v0.to(DEV), grad.to(DEV)
        p16 = torch.full((n + 64,), 7.0, dtype=dt, device=DEV)
        found = torch.zeros(1, dtype=torch.int32, device=DEV)
        _ok(lib, lib.r50_op_adamw(p.data_ptr(), m.data_ptr(), v.data_ptr(), gd.data_ptr(), p16.data_ptr(), n, lr, b1, b2, eps, wd, step,
                                  found.data_ptr(), et, _s()), "adamw")
        pr, mr, vr = R.adamw_ref(p0, m0, v0, grad, step, lr, b1, b2, eps, wd)
        what = f"step {step} lr {lr} wd {wd}"
        pc = p.cpu()
        if lr == 0.0:
            assert torch.equal(pc, p0), f"{what}: p changed"
        m_terms = b1f * m0.double().abs() + (1 - b1f) * grad.double().abs()
        denom = vr.sqrt() / (1 - b2f ** step) ** 0.5 + _f32(eps)
        upd = _f32(lr) / (1 - b1f ** step) * m_terms / denom
        dp = (pc.double() - pr).abs()
        assert bool((dp <= 4 * R.U32 * (p0.double().abs() + pr.abs()) + 24 * R.U32 * upd).all()), f"{what}: p max |d| {float(dp.max()):.3g}"
        dm = (m.cpu().double() - mr).abs()
        assert bool((dm <= 3 * R.U32 * m_terms).all()), f"{what}: m"
        dv = (v.cpu().double() - vr).abs()
        assert bool((dv <= 4 * R.U32 * (b2f * v0.double() + (1 - b2f) * grad.double() ** 2)).all()), f"{what}: v"
        assert torch.equal(_bits(p16[:n].cpu()), _bits(pc.to(dt))), f"{what}: p16 is not p rounded to nearest even"
        assert bool((p16[n:] == 7.0).all())
    found.fill_(1)
    before = [t.clone() for t in (p, m, v, p16)]
    _ok(lib, lib.r50_op_adamw(p.data_ptr(), m.data_ptr(), v.data_ptr(), gd.data_ptr(), p16.data_ptr(), n, 1e-3, b1, b2, eps, 1e-2, 3,
                              found.data_ptr(), et, _s()), "adamw skipped")
    for a, b_ in zip((p, m, v, p16), before):
        assert torch.equal(a, b_), "the step ran with the overflow flag up"


# ---------------------------------------------------------------- f. the head's GEMMs -------------------------------------------------
BIG_GEMMS = [                                     # B 256 x T 40: the automatic tile and the big tiles
    (10240, 3072, 1024, False, True, "fwd"),
    (10240, 2048, 1024, False, False, "fwd"),
    (1024, 10240, 3072, False, False, "dw", 10240),   # dW with K = B*T = 10240
]


def _gemm_check(got16, ref64, et, what):
    """tests/test_kernels_gpu.py's bar against the fp64 product rounded once: |d| <= 2^-m |ref| + 2^-16 max(1, max|ref|) (m = 7 bf16,
    10 fp16), at most 1 % of elements differing at all, rel-L2 < 1e-3.  On the device."""
    ref = R.round16(ref64, et).double()
    got = got16.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    diff = (got - ref).abs()
    lim = ref.abs() * 2.0 ** -R.MANT[et] + 2.0 ** -16 * max(1.0, float(ref.abs().max()))
    nbad = int((diff > lim).sum())
    assert nbad == 0, f"{what}: {nbad} elements beyond tolerance, max diff {float(diff.max())}"
    frac = float((diff > 0).double().mean())
    assert frac < 0.01, f"{what}: {frac:.4f} of elements differ"
    rel = float(diff.norm() / ref.norm().clamp_min(1e-30))
    assert rel < 1e-3, f"{what}: rel-L2 {rel}"


def _gemm_tensors(et, shape):
    """The seeded host tensors of one HEAD_GEMMS / BIG_GEMMS row: x (rows, K), w (cout, K), bias, residual (rows, cout) or None."""
    rows, k, cout, relu, has_res, kind = shape[:6]
    dt = R.DTYPE[et]
    g = torch.Generator().manual_seed(rows + 3 * k + 7 * cout + 11 * len(kind) + et)
    x = torch.randn(rows, k, generator=g).to(dt)
    w = (torch.randn(cout, k, generator=g) * (2.0 / k) ** 0.5).to(dt)
    if kind == "dw":                                                            # the zero padding of K = B*T
        x[:, shape[6]:] = 0
        w[:, shape[6]:] = 0
    bias = torch.randn(cout, generator=g) * 0.1 if kind == "fwd" else torch.zeros(cout)
    res = torch.randn(rows, cout, generator=g).to(dt) if has_res else None
    return x, w, bias, res


def _run_gemm(et, shape, tiles, tensors=None):
    """Every tile id of `tiles` on one row against the fp64 product; ``tensors``: host tensors in _gemm_tensors' order instead of the
    seeded ones.  Returns the outputs, one (rows, cout) tensor per tile."""
    from implementation_phd_lab_vision_amd import ops
    rows, k, cout, relu, has_res, kind = shape[:6]
    dt = R.DTYPE[et]
    x, w, bias, res = tensors or _gemm_tensors(et, shape)
    res = res.to(DEV) if has_res else None
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    ref = R.gemm_ref(xd, wd, bd, res, relu)                                     # fp64, on the device
    numel = rows * cout
    outs = []
    for tile in tiles:
        buf = torch.full((numel + 512 * cout,), -7.0, dtype=dt, device=DEV)
        y = ops.conv2d_bf16(xd.view(rows, 1, 1, k), wd.view(cout, 1, 1, k), bd, relu=relu,
                            residual=res.view(rows, 1, 1, cout) if has_res else None, tile=tile, out=buf)
        torch.cuda.synchronize()
        _gemm_check(y.view(rows, cout), ref, et, f"rows {rows} K {k} cout {cout} tile {tile}")
        assert bool((buf[numel:] == -7.0).all()), f"tile {tile}: wrote past the end of the output"
        outs.append(y.view(rows, cout))
    return outs


def _gemm_id(s):
    return "%s_m%d_k%d_n%d_relu%d_res%d" % ((s[5],) + tuple(int(v) for v in s[:5])) + ("_bt%d" % s[6] if len(s) > 6 else "")


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", HEAD_GEMMS, ids=_gemm_id)
def test_head_gemm_every_tile(lib, et, shape):
    from tests.test_kernels_gpu import _tiles_for
    _run_gemm(et, shape, _tiles_for(shape[2], k=1, pad=0))


@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", BIG_GEMMS, ids=_gemm_id)
def test_head_gemm_driver_rows(lib, et, shape):
    from implementation_phd_lab_vision_amd import ops
    _run_gemm(et, shape, [ops.TILE_AUTO, ops.TILE_256x256 | ops.PERSISTENT, ops.WS | 8, ops.TILE_G8, ops.TILE_G8_224])
