"""The matrix-core kernels held to EXACT results on the MI355X: integer-lattice operands (tests/exact_lattice.py) whose products and
partial sums are all exact in fp32, so the accumulation order does not matter and every kernel must reproduce the fp64 reference bit for
bit after the one rounding of its epilogue -- no tolerance, no share of differing elements.  tests/test_exact_lattice_cpu.py shows that
the preconditions hold for every case here and that a dropped, swapped or misplaced product, or a double rounding, cannot pass.

The launches are the ones tests/test_kernels_gpu.py and tests/test_head_kernels_gpu.py drive (their runners take the lattice tensors
instead of their seeded ones, and still assert what they always assert); fused chains are compared end to end from the inputs.

The ``low`` and ``high`` regimes move the same integer cases to the ends of fp16 and e4m3 (subnormal operands and outputs; outputs
across +-65504): what the f16 / f8 MFMA reads of a subnormal operand, what ``v_cvt_pk_f16_f32`` / ``v_cvt_pk_fp8_f32`` store on the
subnormal grid, and the clamp in front of the fp16 conversion, still at zero tolerance.  A failure counts flushes (0 where the reference
is not), infinities and results one grid step off apart (``exact_lattice.describe_mismatch``).
"""
import pytest
import torch

from tests import exact_lattice as L
from tests import pair_reference as P
from tests.test_head_kernels_gpu import HEAD_GEMMS, _gemm_id
from tests.test_kernels_gpu import CAT_CASES, CONV_CASES, FP8_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = -7.0
FMTS = ("bf16", "fp16")
_conv_id = P.case_id


def _same_bits(y: torch.Tensor, ref_same_layout_f32: torch.Tensor) -> bool:
    ref = ref_same_layout_f32.to(y.dtype).to(y.device)
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[y.element_size()]
    return y.shape == ref.shape and torch.equal(y.contiguous().view(view), ref.contiguous().view(view))


def _assert_nhwc_exact(y_nhwc: torch.Tensor, st: L.Exact, what: str):
    """Bit equality of a device NHWC result with a rounding point of the reference (NCHW); the slow path only words the failure."""
    print(st.report())
    if not _same_bits(y_nhwc, st.ref.permute(0, 2, 3, 1)):
        L.assert_bits_equal(L.nchw_of(y_nhwc), st, what)
        raise AssertionError(f"{what}: bit patterns differ from the exact reference")


def _nhwc_dev(t_nchw, fmt="bf16"):
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(L.FORMATS[fmt].dtype).to(DEV)


def _side(i):
    """The operand that carries the subnormal values of a list's i-th low case (tests/test_exact_lattice_cpu.py: side_of)."""
    return "xw"[i % 2]


def _conv_launches(case, fmt, regime, tiles, side="x"):
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    (x, wt, bias, res), st = L.conv_case(case, fmt, regime, side)
    if regime in L.EDGE_REGIMES:
        L.assert_edge_precondition(st, regime)
        print(st.edge_report())
    else:
        L.assert_exact_precondition(st, regime, tie_floor=st.pre.numel() >= 1000)
    xd, wd, bd = _nhwc_dev(x, fmt), _nhwc_dev(wt, fmt), bias.to(DEV)
    rd = _nhwc_dev(res, fmt) if has_res else None
    ref = st.ref.permute(0, 2, 3, 1).contiguous().to(xd.dtype).to(DEV)
    numel = ref.numel()
    print(st.report())
    for tile in tiles:
        buf = torch.full((numel + 512 * cout,), GUARD, dtype=xd.dtype, device=DEV)
        y = ops.conv2d_bf16(xd, wd, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile, out=buf)
        torch.cuda.synchronize()
        if not torch.equal(y.view(torch.int16), ref.view(torch.int16)):
            L.assert_bits_equal(L.nchw_of(y), st, f"conv {_conv_id(case)} {fmt} {regime} tile={tile}")
            raise AssertionError(f"conv tile={tile}: bit patterns differ from the exact reference")
        assert bool((buf[numel:] == GUARD).all()), f"conv tile={tile}: wrote past the end of the output"


# ---- the foundation: one MFMA tile's worth.  Runs first: if MFMA accumulation were not exact under the precondition, this is where it shows.
@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("fmt", FMTS)
def test_foundation_one_mfma_tile(lib_built, fmt, regime):
    from implementation_phd_lab_vision_amd import ops
    _conv_launches((1, 4, 4, 64, 64, 1, 1, 0, True, False), fmt, regime, [ops.TILE_AUTO])


@pytest.mark.parametrize("regime", L.REGIMES)
def test_foundation_smallest_fp8_case(lib_built, regime):
    _fp8(FP8_CASES[0], regime)


@pytest.mark.parametrize("regime", L.EDGE_REGIMES)
def test_foundation_one_mfma_tile_at_the_ends_of_fp16(lib_built, regime):
    from implementation_phd_lab_vision_amd import ops
    _conv_launches((1, 4, 4, 64, 64, 1, 1, 0, True, False), "fp16", regime, [ops.TILE_AUTO])


def test_foundation_smallest_fp8_case_at_the_bottom_of_e4m3(lib_built):
    _fp8(FP8_CASES[0], "low")


# ---- plain convs: every row x every tile id the one-ulp test runs for it x both types x both regimes, one reference per test
@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_conv2d_every_tile_is_exact(lib_built, case, fmt, regime):
    from tests.test_kernels_gpu import _conv_tiles
    _conv_launches(case, fmt, regime, _conv_tiles(case))


@pytest.mark.parametrize("regime", L.EDGE_REGIMES)
@pytest.mark.parametrize("i", range(len(CONV_CASES)), ids=lambda i: "%d_%s" % (i, _conv_id(CONV_CASES[i])))
def test_conv2d_every_tile_is_exact_at_the_ends_of_fp16(lib_built, i, regime):
    from tests.test_kernels_gpu import _conv_tiles
    _conv_launches(CONV_CASES[i], "fp16", regime, _conv_tiles(CONV_CASES[i]), _side(i))


# ---- two-source 1x1
@pytest.mark.parametrize("regime", L.EDGE_REGIMES)
@pytest.mark.parametrize("i", range(len(CAT_CASES)))
def test_conv1x1_two_k_sources_is_exact_at_the_ends_of_fp16(lib_built, i, regime):
    from tests.test_kernels_gpu import _run_conv1x1_cat
    case = CAT_CASES[i]
    tensors, st = L.cat_case(case, "fp16", regime, _side(i))
    L.assert_edge_precondition(st, regime)
    print(st.edge_report())
    y = _run_conv1x1_cat(case, torch.float16, tensors)
    _assert_nhwc_exact(y, st, f"conv1x1_cat {case} fp16 {regime}")


@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", CAT_CASES, ids=lambda c: "n%d_%dx%d_c%d_src%d_c%d_s%d_o%d_r%d_t%d" % ((c[0], c[1]) + tuple(int(v) for v in c[1:])))
def test_conv1x1_two_k_sources_is_exact(lib_built, case, fmt, regime):
    from tests.test_kernels_gpu import _run_conv1x1_cat
    tensors, st = L.cat_case(case, fmt, regime)
    L.assert_exact_precondition(st, regime)
    y = _run_conv1x1_cat(case, L.FORMATS[fmt].dtype, tensors)
    _assert_nhwc_exact(y, st, f"conv1x1_cat {case} {fmt} {regime}")


# ---- fp8
def _fp8(case, regime):
    from tests.test_kernels_gpu import _run_conv2d_fp8
    tensors, st = L.fp8_case(case, regime)
    if regime == "low":
        L.assert_edge_precondition(st, regime)
        print(st.edge_report())
    else:
        L.assert_exact_precondition(st, regime)
    if regime == "wide":
        sat = float((st.pre.abs() >= 448.0).float().mean())
        print(f"saturating outputs {100 * sat:.2f} %")
        assert 0.0 < sat < 0.5, "the wide fp8 regime needs outputs on both sides of 448"
    y = _run_conv2d_fp8(case, tensors)
    _assert_nhwc_exact(y, st, f"conv2d_fp8 {case} {regime}")


@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("case", FP8_CASES, ids=lambda c: "n%d_%dx%d_c%d_o%d_k%d_s%d_p%d_r%d_res%d_t%d" % tuple(int(v) for v in c))
def test_conv2d_fp8_is_exact(lib_built, case, regime):
    _fp8(case, regime)


@pytest.mark.parametrize("case", FP8_CASES, ids=lambda c: "n%d_%dx%d_c%d_o%d_k%d_s%d_p%d_r%d_res%d_t%d" % tuple(int(v) for v in c))
def test_conv2d_fp8_is_exact_at_the_bottom_of_e4m3(lib_built, case):
    _fp8(case, "low")


# ---- pair modes
@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_w2_conv_every_tile_is_exact(lib_built, case, regime):
    from implementation_phd_lab_vision_amd import ops
    from tests.test_kernels_gpu import _tiles_for
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    (x, wh, wt, bias, res), st = L.w2_case(case, regime)
    L.assert_exact_precondition(st, regime, tie_floor=st.pre.numel() >= 1000)
    print(st.report())
    xd, bd = _nhwc_dev(x), bias.to(DEV)
    wd = torch.cat([wh.permute(0, 2, 3, 1), wt.permute(0, 2, 3, 1)], dim=3).contiguous().to(torch.bfloat16).to(DEV)
    rd = _nhwc_dev(res) if has_res else None
    ref = st.ref.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
    numel = ref.numel()
    refused = (ops.TILE_C64, ops.TILE_XRES, ops.TILE_S2, ops.TILE_G8, ops.TILE_G8_224)
    for tile in [t for t in _tiles_for(cout, k, pad) if t not in refused]:
        buf = torch.full((numel + 512 * cout,), GUARD, dtype=torch.bfloat16, device=DEV)
        y = ops.conv2d_w2(xd, wd, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile, out=buf)
        torch.cuda.synchronize()
        if not torch.equal(y.view(torch.int16), ref.view(torch.int16)):
            L.assert_bits_equal(L.nchw_of(y), st, f"w2 conv {P.case_id(case)} {regime} tile={tile}")
            raise AssertionError(f"w2 conv tile={tile}: bit patterns differ from the exact reference")
        assert bool((buf[numel:] == GUARD).all()), f"w2 conv tile={tile}: wrote past the end of the output"


@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_split_conv_is_exact(lib_built, case, regime):
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    ((xh, xt), (wh, wt), bias, rp), st = L.split_case(case, regime)
    L.assert_exact_precondition(st, regime, tie_floor=False)
    print(st.report())
    bf = torch.bfloat16
    xd = P.nhwc_pair(xh.to(bf), xt.to(bf)).to(DEV)
    wd = torch.cat([t.to(bf).permute(0, 2, 3, 1) for t in (wh, wh, wt)], dim=3).contiguous().to(DEV)
    rd = P.nhwc_pair(rp[0].to(bf), rp[1].to(bf)).to(DEV) if has_res else None
    ref = P.nhwc_pair(*P.split_pair(st.pre)).to(DEV)
    numel = ref.numel()
    buf = torch.full((numel + 512 * 2 * cout,), GUARD, dtype=bf, device=DEV)
    y = ops.conv2d_split(xd, wd, bias.to(DEV), stride=stride, pad=pad, relu=relu, residual_pair=rd, out=buf)
    torch.cuda.synchronize()
    bad = y.view(torch.int16) != ref.view(torch.int16)
    assert not bool(bad.any()), f"{int(bad.sum())} of {numel} plane values differ; heads {int(bad[..., :cout].sum())}, tails {int(bad[..., cout:].sum())}"
    assert bool((buf[numel:] == GUARD).all()), "split conv wrote past the end of the output"


# ---- fused chains, end to end from the inputs
@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("name", list(L.CHAIN_CASES))
def test_fused_chain_is_exact_from_the_inputs(lib_built, name, regime, monkeypatch):
    import tests.test_kernels_gpu as K
    runner, args, build = L.CHAIN_CASES[name]
    if runner == "_run_bneck_tail_layer3" and args[1]:
        monkeypatch.setenv("R50_TAIL3_BP", str(args[1]))
    else:
        monkeypatch.delenv("R50_TAIL3_BP", raising=False)
    tensors, stages = build(regime)
    L.assert_exact_precondition(stages, regime)
    got = getattr(K, runner)(*args, tensors=tensors)
    got = got if isinstance(got, tuple) else (got,)
    by_name = {s.name: s for s in stages}
    for y, key in zip(got, ("out", "y1n")):
        if y is not None and key in by_name:
            _assert_nhwc_exact(y, by_name[key], f"{name} {regime} {key}")
    assert got[0] is not None


# ---- stem and average pool
@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("n", L.STEM_N)
def test_stem_is_exact(lib_built, n, regime):
    from implementation_phd_lab_vision_amd import ops
    (x, wf, bias), st = L.stem_case(n, regime)
    L.assert_exact_precondition(st, regime)
    y = ops.stem_bf16(x.to(DEV), wf, bias.to(DEV))
    torch.cuda.synchronize()
    _assert_nhwc_exact(y, st, f"stem n={n} {regime}")


@pytest.mark.parametrize("shape", L.AVGPOOL_SHAPES)
def test_avgpool_is_exact(lib_built, shape):
    from implementation_phd_lab_vision_amd import ops
    x, ref = L.avgpool_case(shape)
    y = ops.avgpool_bf16(x.to(DEV))
    assert _same_bits(y, ref), f"{int((y.cpu() != ref).sum())} of {ref.numel()} means differ from float32(sum) * float32(1 / HW)"


# ---- the head's GEMMs
@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("et", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", HEAD_GEMMS, ids=_gemm_id)
def test_head_gemm_every_tile_is_exact(lib_built, shape, et, regime):
    from tests.test_head_kernels_gpu import _run_gemm
    from tests.test_kernels_gpu import _tiles_for
    fmt = ("bf16", "fp16")[et]
    tensors, st = L.gemm_case(shape, fmt, regime, device=DEV)
    L.assert_exact_precondition(st, regime)
    print(st.report())
    tiles = _tiles_for(shape[2], k=1, pad=0)
    for tile, y in zip(tiles, _run_gemm(et, shape, tiles, tensors)):
        if not _same_bits(y, st.ref):
            L.assert_bits_equal(y.float(), st, f"gemm {_gemm_id(shape)} {fmt} {regime} tile={tile}")
            raise AssertionError(f"gemm tile={tile}: bit patterns differ from the exact reference")


@pytest.mark.parametrize("regime", L.EDGE_REGIMES)
@pytest.mark.parametrize("i", range(len(HEAD_GEMMS)), ids=lambda i: "%d_%s" % (i, _gemm_id(HEAD_GEMMS[i])))
def test_head_gemm_every_tile_is_exact_at_the_ends_of_fp16(lib_built, i, regime):
    """fwd, dx and dw rows: under the trainers' loss scaling the backward products are the ones that live in fp16's subnormal range."""
    from tests.test_head_kernels_gpu import _run_gemm
    from tests.test_kernels_gpu import _tiles_for
    shape = HEAD_GEMMS[i]
    tensors, st = L.gemm_case(shape, "fp16", regime, device=DEV, side=_side(i))
    L.assert_edge_precondition(st, regime)
    print(st.report())
    print(st.edge_report())
    tiles = _tiles_for(shape[2], k=1, pad=0)
    for tile, y in zip(tiles, _run_gemm(1, shape, tiles, tensors)):
        if not _same_bits(y, st.ref):
            L.assert_bits_equal(y.float(), st, f"gemm {_gemm_id(shape)} fp16 {regime} tile={tile}")
            raise AssertionError(f"gemm tile={tile}: bit patterns differ from the exact reference")


# ---- fused chains, stem and average pool in fp16 (the op-level hooks run their IEEE-half kernels for fp16 tensors: ops._op_et)
@pytest.mark.parametrize("name", L.LOW_CHAINS)
def test_fused_chain_is_exact_at_the_bottom_of_fp16(lib_built, name, monkeypatch):
    """The first stage runs on normal operands and stores subnormal intermediates; the next stage re-reads what the kernel stored
    itself, from LDS or HBM, as an MFMA operand.  The reference rounds every stored intermediate onto the subnormal grid."""
    import tests.test_kernels_gpu as K
    runner, args, build = L.CHAIN_CASES[name]
    if runner == "_run_bneck_tail_layer3" and args[1]:
        monkeypatch.setenv("R50_TAIL3_BP", str(args[1]))
    else:
        monkeypatch.delenv("R50_TAIL3_BP", raising=False)
    tensors, stages = build("low", "fp16")
    L.assert_edge_precondition(stages, "low")
    for s in stages:
        print(s.edge_report())
    got = getattr(K, runner)(*args, tensors=tensors)
    got = got if isinstance(got, tuple) else (got,)
    by_name = {s.name: s for s in stages}
    for y, key in zip(got, ("out", "y1n")):
        if y is not None and key in by_name:
            assert y.dtype == torch.float16
            _assert_nhwc_exact(y, by_name[key], f"{name} fp16 low {key}")
    assert got[0] is not None


@pytest.mark.parametrize("regime,side", [("low", "x"), ("low", "w"), ("high", "x")])
def test_stem_is_exact_at_the_ends_of_fp16(lib_built, regime, side):
    from implementation_phd_lab_vision_amd import ops
    (x, wf, bias), st = L.stem_case(1, regime, "fp16", side)
    L.assert_edge_precondition(st, regime)
    print(st.edge_report())
    y = ops.stem_bf16(x.to(DEV), wf, bias.to(DEV), dtype=torch.float16)
    torch.cuda.synchronize()
    _assert_nhwc_exact(y, st, f"stem n=1 fp16 {regime} {side}")


@pytest.mark.parametrize("shape", L.AVGPOOL_SHAPES)
def test_avgpool_is_exact_on_fp16_subnormal_addends(lib_built, shape):
    from implementation_phd_lab_vision_amd import ops
    x, ref = L.avgpool_case(shape, "fp16", 2.0 ** -24)
    a = x.float().abs()
    assert bool((a[a > 0] < 2.0 ** -14).all()) and bool((ref != 0).any())
    y = ops.avgpool_bf16(x.to(DEV))
    assert _same_bits(y, ref), f"{int((y.cpu() != ref).sum())} of {ref.numel()} means differ from float32(sum) * float32(1 / HW); zeros where the " \
                               f"reference has none: {int(((y.cpu() == 0) & (ref != 0)).sum())}"
