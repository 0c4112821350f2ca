"""Per-kernel parity on the MI355X: every HIP kernel, called through the C ABI (r50_op_*), against the
CPU oracle (oracle/resnet50_oracle.py) on the same seeded bf16 inputs.

Tolerance (stated once, used everywhere below): the device accumulates bf16 x bf16 products in fp32
(MFMA) where the oracle accumulates in fp64, then both round to bf16.  So outputs must agree to
within ONE bf16 ulp element-wise, plus an absolute term for results that are the cancellation of
O(1) terms (fp32 accumulation noise ~ 2^-16 of the tensor's scale):
|d| <= 2^-7 * |ref| + 2^-16 * max(1, max|ref|); at most 1 % of elements may differ at all, and the
tensor rel-L2 must be < 1e-3.
"""
import pytest
import torch
from tests.kernel_cases import (  # noqa: F401
    CAT_CASES, CONV_CASES, FP8_CASES, _conv_inputs, _dev, _rand_bf16, _tail3_inputs, _tiles_for, fp8_reference)

pytestmark = pytest.mark.gpu


def _check_bf16(dev_nhwc: torch.Tensor, ref_nchw: torch.Tensor, what: str, mant: int = 7):
    """The bar stated above; ``mant`` = 10 holds an fp16 tensor to one fp16 ulp instead (same absolute term, same counts)."""
    from oracle.resnet50_oracle import rel_l2
    got = dev_nhwc.float().cpu().permute(0, 3, 1, 2).contiguous()
    ref = ref_nchw.float()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    diff = (got - ref).abs()
    ulp = ref.abs() * 2.0 ** -mant + 2.0 ** -16 * max(1.0, float(ref.abs().max()))
    bad = diff > ulp
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond tolerance, max diff {float(diff.max())}"
    frac = float((diff > 0).float().mean())
    assert frac < 0.01, f"{what}: {frac:.4f} of elements differ"
    r = rel_l2(got, ref)
    assert r < 1e-3, f"{what}: rel-L2 {r}"


def _fmt_of(t: torch.Tensor):
    """(oracle fmt, mantissa bits of _check_bf16) of a runner's 16-bit tensors: the fused kernels run in bf16 or in fp16."""
    return ("fp16", 10) if t.dtype == torch.float16 else ("bf16", 7)


def _check_fp16(y: torch.Tensor, ref: torch.Tensor, what: str):
    """The fp16 form of _check_bf16: one fp16 ulp + 2^-19 of scale per element, < 1 % of elements differing, rel-L2 < 2e-4."""
    from oracle.resnet50_oracle import rel_l2
    assert y.dtype == torch.float16
    got = y.float().cpu().permute(0, 3, 1, 2)
    diff = (got - ref).abs()
    ulp = ref.abs() * 2.0 ** -10 + 2.0 ** -19 * max(1.0, float(ref.abs().max()))
    assert torch.isfinite(got).all() and not (diff > ulp).any(), f"{what}: max diff {float(diff.max())}"
    assert float((diff > 0).float().mean()) < 0.01 and rel_l2(got, ref) < 2e-4, what


def _conv_tile_check(case, inputs, tile):
    """One launch of a CONV_CASES row with tile id `tile` against the oracle, with a poisoned guard band behind the result; returns the output."""
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xd, wd, bd, rd, ref, (ho, wo) = inputs
    # guard band behind the result: the tile rows past M (ragged last tile) must not be stored anywhere
    numel = n * ho * wo * cout
    buf = torch.full((numel + 512 * cout,), -7.0, dtype=xd.dtype, device=xd.device)
    y = ops.conv2d_bf16(xd, wd, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile, out=buf)
    torch.cuda.synchronize()
    _check_bf16(y, ref, f"conv tile={tile}", 10 if xd.dtype == torch.float16 else 7)
    assert bool((buf[numel:] == -7.0).all()), f"conv tile={tile}: wrote past the end of the output"
    return y


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "n%d_%dx%d_c%d-%d_k%ds%dp%d_r%d_res%d" % tuple(int(v) for v in c))
def test_conv2d_matches_oracle(lib_built, case):
    xd, wd, bd, rd, ref, (ho, wo) = _conv_inputs(case)
    for tile in _conv_tiles(case):
        _conv_tile_check(case, (xd, wd, bd, rd, ref, (ho, wo)), tile)


def _conv_tiles(case):
    """Every tile id one CONV_CASES row runs under: the generic, persistent and role-specialised ones its cout allows, plus the
    shape-specialised kernels on their shapes."""
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    tiles = _tiles_for(cout, k, pad)
    if n >= 64:                      # the big case is there for the tile STREAM of the persistent kernels: the small tiles add nothing
        tiles = [ops.TILE_AUTO, ops.TILE_256x256 | ops.PERSISTENT, ops.WS | 8, ops.TILE_G8, ops.TILE_G8_224]
    if (h, w, cin, cout, k, stride, pad, has_res) == (56, 56, 64, 64, 3, 1, 1, False):
        tiles = tiles + [ops.TILE_C64]
    if (k, stride, pad, has_res) == (3, 1, 1, False) and (h, w, cin, cout) in ((28, 28, 128, 128), (14, 14, 256, 256), (7, 7, 512, 512)):
        tiles = tiles + [ops.TILE_XRES]
    if (k, stride, pad, has_res) == (3, 2, 1, False) and (h, w, cin, cout) in ((56, 56, 128, 128), (28, 28, 256, 256), (14, 14, 512, 512)):
        tiles = tiles + [ops.TILE_S2]
    return tiles


G8_SHAPES = [   # n, h (= w), cin, cout, residual: the streaming 1x1 convs of layer3 / layer4 at batch 256 (+ a batch that leaves the last tile ragged)
    (256, 28, 512, 256, False), (256, 14, 1024, 256, False), (256, 14, 1024, 512, False), (256, 7, 2048, 512, False), (256, 7, 512, 2048, True),
    (77, 7, 512, 2048, True), (50, 14, 1024, 512, False),
]


@pytest.mark.parametrize("et", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", G8_SHAPES, ids=lambda v: "n%d_%dx%d_c%d-%d_res%d" % (v[0], v[1], v[1], v[2], v[3], v[4]))
def test_gemm8p_tiles_give_the_bits_of_the_generic_tiles(lib_built, shape, et):
    """gemm8p_kernel keeps igemm_bf16_kernel's K order per accumulator (bias first, K-tiles ascending, two 32-deep MFMAs per K-tile) and its
    epilogue, so both of its tile widths must reproduce the two-stage 256x256 tile bit for bit -- at the sizes the network runs them at
    (one to four rounds of tiles per workgroup through the stream of LDS-DMA stages: a stale or early fragment read shows up here),
    three launches each, with a poisoned guard band behind the output."""
    from implementation_phd_lab_vision_amd import ops
    n, hw, cin, cout, has_res = shape
    g = torch.Generator().manual_seed(n * 7 + cin)
    d = _dev()
    x = (torch.randn((n, hw, hw, cin), generator=g)).to(et).to(d)
    wt = (torch.randn((cout, 1, 1, cin), generator=g) * (2.0 / cin) ** 0.5).to(et).to(d)
    bias = (torch.randn(cout, generator=g) * 0.1).to(d)
    res = torch.randn((n, hw, hw, cout), generator=g).to(et).to(d) if has_res else None
    ref = ops.conv2d_bf16(x, wt, bias, relu=True, residual=res, tile=ops.TILE_256x256)
    numel = ref.numel()
    for tile in (ops.TILE_G8, ops.TILE_G8_224):
        for rep in range(3):
            buf = torch.full((numel + 512 * cout,), -7.0, dtype=et, device=d)
            y = ops.conv2d_bf16(x, wt, bias, relu=True, residual=res, tile=tile, out=buf)
            torch.cuda.synchronize()
            assert torch.equal(y, ref), f"tile {tile} rep {rep}: {int((y != ref).sum())} of {numel} elements differ"
            assert bool((buf[numel:] == -7.0).all()), f"tile {tile}: wrote past the end of the output"


@pytest.mark.parametrize("shape", [(5, 7, 512), (3, 28, 128), (3, 14, 256), (70, 14, 256), (300, 14, 256), (260, 7, 512)],
                         ids=lambda v: "n%d_%dx%d_c%d" % (v[0], v[1], v[1], v[2]))
def test_xres_kernel_is_batch_invariant_and_stays_inside_its_output(lib_built, shape):
    _run_xres_batch_invariance(shape)


def _run_xres_batch_invariance(shape):
    """conv3x3_xres_kernel (row blocks) with several tiles per workgroup (n = 300 at 14x14: 600 tiles on 256 CUs: the stream of weight stages and
    input chunks crosses tile borders) and with panels / cout tiles left ragged: every image's result is the same bits as when the image is run
    alone, the generic kernel agrees to the bf16 tolerance (its K order differs), and nothing is stored past the output (poisoned guard band).
    (Rounds 2-3 compared eleven schedule variants of this kernel bit for bit here; they were removed in round 4.)"""
    from implementation_phd_lab_vision_amd import ops
    n, hw, c = shape
    g = torch.Generator().manual_seed(n * 1000 + hw)
    d = _dev()
    x = _rand_bf16((n, hw, hw, c), g).to(d)
    wt = _rand_bf16((c, 3, 3, c), g, scale=(2.0 / (9 * c)) ** 0.5).to(d)
    bias = (torch.randn(c, generator=g) * 0.1).to(d)
    numel = n * hw * hw * c
    buf = torch.full((numel + 512 * c,), -7.0, dtype=torch.bfloat16, device=d)
    y = ops.conv2d_bf16(x, wt, bias, stride=1, pad=1, relu=True, tile=ops.TILE_XRES, out=buf)
    torch.cuda.synchronize()
    assert bool((buf[numel:] == -7.0).all()), "wrote past the end of the output"
    for i in sorted({0, n // 2, n - 1}):
        alone = ops.conv2d_bf16(x[i:i + 1].contiguous(), wt, bias, stride=1, pad=1, relu=True, tile=ops.TILE_XRES)
        assert torch.equal(alone[0], y[i]), f"image {i} of {n} differs from the same image run alone"
    gen = ops.conv2d_bf16(x[:2].contiguous(), wt, bias, stride=1, pad=1, relu=True, tile=ops.WS | 8)
    d2 = (gen.float() - y[:2].float()).abs()
    assert float(d2.max()) <= 2.0 ** -6 * max(1.0, float(y[:2].float().abs().max())), float(d2.max())
    return y


@pytest.mark.parametrize("shape", [(1, 56, 128), (70, 56, 128), (300, 56, 128), (5, 28, 256), (300, 28, 256), (3, 14, 512), (300, 14, 512)],
                         ids=lambda v: "n%d_%dx%d_c%d" % (v[0], v[1], v[1], v[2]))
def test_s2_kernel_is_batch_invariant_and_stays_inside_its_output(lib_built, shape):
    _run_s2_batch_invariance(shape)


def _run_s2_batch_invariance(shape):
    """conv3x3_s2_kernel with several tiles per workgroup (n = 300: 1,200 / 600 tiles on 256 CUs: the plane stream crosses tile borders,
    the loader re-decodes its offsets in mid-stream): every image's result is the same bits as when the image is run alone, and nothing
    is stored past the output (poisoned guard band)."""
    from implementation_phd_lab_vision_amd import ops
    n, hw, c = shape
    g = torch.Generator().manual_seed(n * 100 + hw)
    d = _dev()
    x = _rand_bf16((n, hw, hw, c), g).to(d)
    wt = _rand_bf16((c, 3, 3, c), g, scale=(2.0 / (9 * c)) ** 0.5).to(d)
    bias = (torch.randn(c, generator=g) * 0.1).to(d)
    ho = hw // 2
    numel = n * ho * ho * c
    buf = torch.full((numel + 512 * c,), -7.0, dtype=torch.bfloat16, device=d)
    y = ops.conv2d_bf16(x, wt, bias, stride=2, pad=1, relu=True, tile=ops.TILE_S2, out=buf)
    torch.cuda.synchronize()
    assert bool((buf[numel:] == -7.0).all()), "wrote past the end of the output"
    for i in sorted({0, n // 2, n - 1}):
        alone = ops.conv2d_bf16(x[i:i + 1].contiguous(), wt, bias, stride=2, pad=1, relu=True, tile=ops.TILE_S2)
        assert torch.equal(alone[0], y[i]), f"image {i} of {n} differs from the same image run alone"
    return y


@pytest.mark.parametrize("chain", [False, True], ids=["last_block", "chained_conv1"])
@pytest.mark.parametrize("n", [1, 3, 70])
def test_bneck_block2_equals_unfused(lib_built, n, chain):
    _run_bneck_block2(n, chain)


def _block2_tensors(n):
    """The seeded host tensors of _run_bneck_block2 (NHWC / OHWI): t1, idn, w2, w3, w1, b2, b3, b1."""
    g = torch.Generator().manual_seed(4100 + n)
    t1 = _rand_bf16((n, 28, 28, 128), g).clamp_(min=0)
    idn = _rand_bf16((n, 28, 28, 512), g).clamp_(min=0)
    w2 = _rand_bf16((128, 3, 3, 128), g, scale=(2.0 / 1152) ** 0.5)
    w3 = _rand_bf16((512, 1, 1, 128), g, scale=(2.0 / 128) ** 0.5)
    w1 = _rand_bf16((128, 1, 1, 512), g, scale=(2.0 / 512) ** 0.5)
    b2 = torch.randn(128, generator=g) * 0.1
    b3 = torch.randn(512, generator=g) * 0.1
    b1 = torch.randn(128, generator=g) * 0.1
    return t1, idn, w2, w3, w1, b2, b3, b1


def _run_bneck_block2(n, chain, tensors=None):
    """Layer2 bottleneck body in one launch (conv2 3x3 + conv3 + identity + ReLU [+ next conv1]): block output and next t1 are the
    same bits as the input-resident 3x3 launch followed by the 1x1 igemm launches (n = 70: 280 tiles, more than one per workgroup).
    ``tensors``: host tensors in _block2_tensors' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    d = _dev()
    t1, idn, w2, w3, w1, b2, b3, b1 = (t.to(d) for t in (tensors or _block2_tensors(n)))
    t2 = ops.conv2d_bf16(t1, w2, b2, stride=1, pad=1, relu=True, tile=ops.TILE_XRES)
    out_ref = ops.conv2d_bf16(t2, w3, b3, stride=1, pad=0, relu=True, residual=idn)
    y1_ref = ops.conv2d_bf16(out_ref, w1, b1, stride=1, pad=0, relu=True)
    out, y1n = ops.bneck_block2_bf16(t1, w2, b2, w3.view(512, 128), b3, idn, w1.view(128, 512) if chain else None, b1 if chain else None)
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref), f"block output differs: max |diff| {float((out.float() - out_ref.float()).abs().max())}"
    if chain:
        assert torch.equal(y1n, y1_ref), f"next conv1 differs: max |diff| {float((y1n.float() - y1_ref.float()).abs().max())}"
    else:
        assert y1n is None
    return out, y1n


@pytest.mark.parametrize("c1", [64, 128])
@pytest.mark.parametrize("n", [1, 3, 20, 41])
def test_bneck_block1_equals_unfused(lib_built, n, c1):
    _run_bneck_block1(n, c1)


def _block1_tensors(n, c1):
    """The seeded host tensors of _run_bneck_block1 (NHWC / OHWI): t1, idn, w2, w3, w1, b2, b3, b1."""
    g = torch.Generator().manual_seed(5100 + n + c1)
    t1 = _rand_bf16((n, 56, 56, 64), g).clamp_(min=0)
    idn = _rand_bf16((n, 56, 56, 256), g).clamp_(min=0)
    w2 = _rand_bf16((64, 3, 3, 64), g, scale=(2.0 / 576) ** 0.5)
    w3 = _rand_bf16((256, 1, 1, 64), g, scale=(2.0 / 64) ** 0.5)
    w1 = _rand_bf16((c1, 1, 1, 256), g, scale=(2.0 / 256) ** 0.5)
    b2 = torch.randn(64, generator=g) * 0.1
    b3 = torch.randn(256, generator=g) * 0.1
    b1 = torch.randn(c1, generator=g) * 0.1
    return t1, idn, w2, w3, w1, b2, b3, b1


def _run_bneck_block1(n, c1, tensors=None):
    """Layer1 bottleneck body in one launch: block output and next t1 are the same bits as the resident-weights 3x3 launch followed by
    the 1x1 igemm launches (n = 20: 280 tiles, more than one per workgroup; n = 41: 574 tiles, up to three per workgroup).
    ``tensors``: host tensors in _block1_tensors' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    d = _dev()
    t1, idn, w2, w3, w1, b2, b3, b1 = (t.to(d) for t in (tensors or _block1_tensors(n, c1)))
    t2 = ops.conv2d_bf16(t1, w2, b2, stride=1, pad=1, relu=True, tile=ops.TILE_C64)
    out_ref = ops.conv2d_bf16(t2, w3, b3, stride=1, pad=0, relu=True, residual=idn)
    y1_ref = ops.conv2d_bf16(out_ref, w1, b1, stride=1, pad=0, relu=True)
    out, y1n = ops.bneck_block1_bf16(t1, w2, b2, w3.view(256, 64), b3, idn, w1.view(c1, 256), b1)
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref), f"block output differs: max |diff| {float((out.float() - out_ref.float()).abs().max())}"
    assert torch.equal(y1n, y1_ref), f"next conv1 differs: max |diff| {float((y1n.float() - y1_ref.float()).abs().max())}"
    return out, y1n


@pytest.mark.parametrize("n", [1, 3, 20, 41])
def test_bneck_block1_downsample_equals_unfused(lib_built, n):
    _run_bneck_block1_ds(n)


def _block1_ds_tensors(n):
    """The seeded host tensors of _run_bneck_block1_ds (NHWC / OHWI): t1, x, w2, w3, wd, w1, b2, b3, bd, b1."""
    g = torch.Generator().manual_seed(5300 + n)
    t1 = _rand_bf16((n, 56, 56, 64), g).clamp_(min=0)
    x = _rand_bf16((n, 56, 56, 64), g).clamp_(min=0)
    w2 = _rand_bf16((64, 3, 3, 64), g, scale=(2.0 / 576) ** 0.5)
    w3 = _rand_bf16((256, 1, 1, 64), g, scale=(2.0 / 64) ** 0.5)
    wd = _rand_bf16((256, 1, 1, 64), g, scale=(1.0 / 64) ** 0.5)
    w1 = _rand_bf16((64, 1, 1, 256), g, scale=(2.0 / 256) ** 0.5)
    b2 = torch.randn(64, generator=g) * 0.1
    b3 = torch.randn(256, generator=g) * 0.1
    bd = torch.randn(256, generator=g) * 0.1
    b1 = torch.randn(64, generator=g) * 0.1
    return t1, x, w2, w3, wd, w1, b2, b3, bd, b1


def _run_bneck_block1_ds(n, tensors=None):
    """layer1.0's body in one launch (bneck_block1_kernel<.., DS>): the identity is the downsample conv of the block input, computed in the
    kernel and rounded to bf16 as the separate launch stores it.  Block output and next t1 are the same bits as the resident-weights 3x3 launch,
    the 1x1 downsample launch, the 1x1 conv3 launch with that identity, and the next 1x1 launch.
    ``tensors``: host tensors in _block1_ds_tensors' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    d = _dev()
    t1, x, w2, w3, wd, w1, b2, b3, bd, b1 = (t.to(d) for t in (tensors or _block1_ds_tensors(n)))
    t2 = ops.conv2d_bf16(t1, w2, b2, stride=1, pad=1, relu=True, tile=ops.TILE_C64)
    idn = ops.conv2d_bf16(x, wd, bd, stride=1, pad=0, relu=False)
    out_ref = ops.conv2d_bf16(t2, w3, b3, stride=1, pad=0, relu=True, residual=idn)
    y1_ref = ops.conv2d_bf16(out_ref, w1, b1, stride=1, pad=0, relu=True)
    out, y1n = ops.bneck_block1_ds_bf16(t1, w2, b2, w3.view(256, 64), b3, x, wd.view(256, 64), bd, w1.view(64, 256), b1)
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref), f"block output differs: max |diff| {float((out.float() - out_ref.float()).abs().max())}"
    assert torch.equal(y1n, y1_ref), f"next conv1 differs: max |diff| {float((y1n.float() - y1_ref.float()).abs().max())}"
    return out, y1n


@pytest.mark.parametrize("ds", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("shape,c1", [((2, 7, 9), 64), ((1, 56, 56), 128), ((3, 5, 16), 64), ((5, 56, 56), 64)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_bneck_tail_matches_oracle_and_unfused(lib_built, shape, c1, ds):
    _run_bneck_tail(shape, c1, ds)


def _tail_tensors(shape, c1, ds):
    """The seeded host tensors of _run_bneck_tail (NCHW / OIHW): y2, w3, b3, w1, b1, then idn -- or, with ds, xin, wd, bd."""
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 + n * h * w + c1)
    y2 = _rand_bf16((n, 64, h, w), g)
    w3 = _rand_bf16((256, 64, 1, 1), g, scale=(2.0 / 64) ** 0.5)
    b3 = torch.randn(256, generator=g) * 0.1
    w1 = _rand_bf16((c1, 256, 1, 1), g, scale=(2.0 / 256) ** 0.5)
    b1 = torch.randn(c1, generator=g) * 0.1
    if ds:
        xin = _rand_bf16((n, 64, h, w), g)
        wd = _rand_bf16((256, 64, 1, 1), g, scale=(1.0 / 64) ** 0.5)
        bd = torch.randn(256, generator=g) * 0.1
        return y2, w3, b3, w1, b1, xin, wd, bd
    return y2, w3, b3, w1, b1, _rand_bf16((n, 256, h, w), g)


def _run_bneck_tail(shape, c1, ds, tensors=None):
    """Fused layer1 tail (conv3 + identity + ReLU, then the next conv1 + ReLU) against the oracle's two fused-op
    emulations chained, and bit-for-bit against the two igemm launches it replaces.  Pixel counts that are not a
    multiple of 16 exercise the descriptor-clamped last tile; a guard band checks nothing is stored past M.
    ``tensors``: host tensors in _tail_tensors' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    from oracle.resnet50_oracle import conv_bias_act_emulated
    n, h, w = shape
    y2, w3, b3, w1, b1, *rest = tensors or _tail_tensors(shape, c1, ds)
    fmt, mant = _fmt_of(y2)
    d = _dev()
    y2d = y2.permute(0, 2, 3, 1).contiguous().to(d)
    w3d, w1d = w3.view(256, 64).contiguous().to(d), w1.view(c1, 256).contiguous().to(d)
    b3d, b1d = b3.to(d), b1.to(d)
    if ds:      # first block of the stage: identity = downsample(block input), computed inside the kernel
        xin, wd, bd = rest
        idn = conv_bias_act_emulated(xin.float(), wd.float(), bd, 1, 0, False, fmt=fmt)
        xind = xin.permute(0, 2, 3, 1).contiguous().to(d)
        wdd, bdd = wd.view(256, 64).contiguous().to(d), bd.to(d)
        idd = ops.conv2d_bf16(xind, wdd.view(256, 1, 1, 64), bdd, relu=False, tile=ops.TILE_64x128)
        _check_bf16(idd, idn, "downsample identity", mant)
        idn = idd.float().cpu().permute(0, 3, 1, 2)        # chain the oracle from the device's identity (see below)
        out, y1n = ops.bneck_tail_bf16(y2d, w3d, b3d, xind, w1d, b1d, wd=wdd, bd=bdd)
    else:
        idn, = rest
        idd = idn.permute(0, 2, 3, 1).contiguous().to(d)
        out, y1n = ops.bneck_tail_bf16(y2d, w3d, b3d, idd, w1d, b1d)
    out_ref = conv_bias_act_emulated(y2.float(), w3.float(), b3, 1, 0, True, residual_bf=idn.float(), fmt=fmt)
    torch.cuda.synchronize()
    _check_bf16(out, out_ref, "bneck_tail out", mant)
    # the second GEMM reads the DEVICE's bf16 block output, so chain the oracle from it (one-ulp flips of `out`
    # are legal and would otherwise be amplified into a false mismatch of y1n)
    y1_ref = conv_bias_act_emulated(out.float().cpu().permute(0, 3, 1, 2), w1.float(), b1, 1, 0, True, fmt=fmt)
    _check_bf16(y1n, y1_ref, "bneck_tail y1n", mant)
    out_u = ops.conv2d_bf16(y2d, w3d.view(256, 1, 1, 64), b3d, relu=True, residual=idd, tile=ops.TILE_64x128)
    y1_u = ops.conv2d_bf16(out_u, w1d.view(c1, 1, 1, 256), b1d, relu=True, tile=ops.TILE_64x128)
    assert torch.equal(out, out_u), "fused block output differs from the igemm launch it replaces"
    assert torch.equal(y1n, y1_u), "fused next-conv1 output differs from the igemm launch it replaces"
    return out, y1n


@pytest.mark.parametrize("shape", [(2, 7, 9), (1, 28, 28), (3, 5, 16), (9, 28, 28)], ids=lambda v: str(v).replace(" ", ""))
def test_bneck_tail_layer2_shapes(lib_built, shape):
    _run_bneck_tail_layer2(shape)


def _tail2_tensors(shape):
    """The seeded host tensors of _run_bneck_tail_layer2 (NCHW / OIHW): y2, w3, b3, idn, w1, b1."""
    n, h, w = shape
    g = torch.Generator().manual_seed(2000 + n * h * w)
    y2 = _rand_bf16((n, 128, h, w), g)
    w3 = _rand_bf16((512, 128, 1, 1), g, scale=(2.0 / 128) ** 0.5)
    b3 = torch.randn(512, generator=g) * 0.1
    idn = _rand_bf16((n, 512, h, w), g)
    w1 = _rand_bf16((128, 512, 1, 1), g, scale=(2.0 / 512) ** 0.5)
    b1 = torch.randn(128, generator=g) * 0.1
    return y2, w3, b3, idn, w1, b1


def _run_bneck_tail_layer2(shape, tensors=None):
    """Fused layer2 tail (conv3 128->512 + identity + ReLU, next conv1 512->128 + ReLU; channels split over the waves,
    second conv reduced through LDS).  conv3's output must equal the igemm launch bit for bit; the second conv sums
    its K in eight slices, so it is held to the oracle under the bf16 tolerance.
    ``tensors``: host tensors in _tail2_tensors' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    from oracle.resnet50_oracle import conv_bias_act_emulated
    n, h, w = shape
    y2, w3, b3, idn, w1, b1 = tensors or _tail2_tensors(shape)
    fmt, mant = _fmt_of(y2)
    d = _dev()
    y2d = y2.permute(0, 2, 3, 1).contiguous().to(d)
    idd = idn.permute(0, 2, 3, 1).contiguous().to(d)
    w3d, w1d = w3.view(512, 128).contiguous().to(d), w1.view(128, 512).contiguous().to(d)
    b3d, b1d = b3.to(d), b1.to(d)
    out, y1n = ops.bneck_tail_bf16(y2d, w3d, b3d, idd, w1d, b1d)
    torch.cuda.synchronize()
    out_ref = conv_bias_act_emulated(y2.float(), w3.float(), b3, 1, 0, True, residual_bf=idn.float(), fmt=fmt)
    _check_bf16(out, out_ref, "bneck_tail2 out", mant)
    y1_ref = conv_bias_act_emulated(out.float().cpu().permute(0, 3, 1, 2), w1.float(), b1, 1, 0, True, fmt=fmt)
    _check_bf16(y1n, y1_ref, "bneck_tail2 y1n", mant)
    out_u = ops.conv2d_bf16(y2d, w3d.view(512, 1, 1, 128), b3d, relu=True, residual=idd, tile=ops.TILE_64x128)
    assert torch.equal(out, out_u), "fused block output differs from the igemm launch it replaces"
    return out, y1n


@pytest.mark.parametrize("shape,bp", [((2, 7, 9), 0), ((1, 14, 14), 0), ((3, 14, 14), 112), ((3, 14, 14), 98), ((20, 14, 14), 7), ((5, 14, 14), 33)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_bneck_tail_layer3_shapes(lib_built, shape, bp, monkeypatch):
    if bp:
        monkeypatch.setenv("R50_TAIL3_BP", str(bp))
    else:
        monkeypatch.delenv("R50_TAIL3_BP", raising=False)
    _run_bneck_tail_layer3(shape, bp)


def _run_bneck_tail_layer3(shape, bp, tensors=None):
    """Chained layer3 tail (conv3 256->1024 + identity + ReLU, next conv1 1024->256 + ReLU; weights streamed through the LDS ring,
    the residual as one more K-step against an identity operand, the block output handed to the second GEMM through LDS).
    Against the oracle's two fused-op emulations, and BIT FOR BIT against the two igemm launches it replaces (same summation
    orders).  bp = real pixels per tile: ragged tiles, several tiles per workgroup (bp 7: 560 tiles), full 112-pixel tiles and 98.
    The kernel is bneck_tail3p_kernel (two-group pipeline); rounds 2-3's bneck_tail3_kernel and the 98-row form were removed in round 4.
    ``tensors``: host tensors in _tail3_inputs' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    from oracle.resnet50_oracle import conv_bias_act_emulated
    n, h, w = shape
    y2, w3, b3, idn, w1, b1 = tensors or _tail3_inputs(n, h, w, 3000 + n * h * w + bp)
    fmt, mant = _fmt_of(y2)
    d = _dev()
    y2d = y2.permute(0, 2, 3, 1).contiguous().to(d)
    idd = idn.permute(0, 2, 3, 1).contiguous().to(d)
    w3d, w1d = w3.view(1024, 256).contiguous().to(d), w1.view(256, 1024).contiguous().to(d)
    b3d, b1d = b3.to(d), b1.to(d)
    m = n * h * w
    guard = 4096                                   # poisoned rows behind both outputs: nothing may be stored past M
    out_buf = torch.full((m + guard, 1024), -7.0, dtype=y2.dtype, device=d)
    y1_buf = torch.full((m + guard, 256), -7.0, dtype=y2.dtype, device=d)
    out, y1n = ops.bneck_tail_bf16(y2d, w3d, b3d, idd, w1d, b1d, out=out_buf[:m].view(n, h, w, 1024), y1n=y1_buf[:m].view(n, h, w, 256))
    torch.cuda.synchronize()
    assert bool((out_buf[m:] == -7.0).all()) and bool((y1_buf[m:] == -7.0).all()), "stored past M"
    out_u = ops.conv2d_bf16(y2d, w3d.view(1024, 1, 1, 256), b3d, relu=True, residual=idd, tile=ops.TILE_64x128)
    y1_u = ops.conv2d_bf16(out_u, w1d.view(256, 1, 1, 1024), b1d, relu=True, tile=ops.TILE_64x128)
    assert torch.equal(out, out_u), "chained block output differs from the igemm launch it replaces"
    assert torch.equal(y1n, y1_u), "chained next-conv1 output differs from the igemm launch it replaces"
    if m <= 1000:
        out_ref = conv_bias_act_emulated(y2.float(), w3.float(), b3, 1, 0, True, residual_bf=idn.float(), fmt=fmt)
        _check_bf16(out, out_ref, "bneck_tail3 out", mant)
        y1_ref = conv_bias_act_emulated(out.float().cpu().permute(0, 3, 1, 2), w1.float(), b1, 1, 0, True, fmt=fmt)
        _check_bf16(y1n, y1_ref, "bneck_tail3 y1n", mant)
    return out, y1n


def test_bneck_tail_layer3_batch256_equals_unfused(lib_built, monkeypatch):
    """The benchmarked size (256 x 14 x 14 = 50,176 pixels -> 448 full tiles of 112, up to two per workgroup): bit-identical to the launches it replaces."""
    from implementation_phd_lab_vision_amd import ops
    monkeypatch.delenv("R50_TAIL3_BP", raising=False)
    y2, w3, b3, idn, w1, b1 = _tail3_inputs(256, 14, 14, 3999)
    d = _dev()
    y2d = y2.permute(0, 2, 3, 1).contiguous().to(d)
    idd = idn.permute(0, 2, 3, 1).contiguous().to(d)
    w3d, w1d = w3.view(1024, 256).contiguous().to(d), w1.view(256, 1024).contiguous().to(d)
    b3d, b1d = b3.to(d), b1.to(d)
    out, y1n = ops.bneck_tail_bf16(y2d, w3d, b3d, idd, w1d, b1d)
    out_u = ops.conv2d_bf16(y2d, w3d.view(1024, 1, 1, 256), b3d, relu=True, residual=idd)
    y1_u = ops.conv2d_bf16(out_u, w1d.view(256, 1, 1, 1024), b1d, relu=True)
    assert torch.equal(out, out_u) and torch.equal(y1n, y1_u)


@pytest.mark.parametrize("n", [1, 3, 37, 256], ids=lambda v: "n%d" % v)
def test_bneck_cat_chain_equals_the_two_launches(lib_built, n):
    _run_bneck_cat_chain(n)


def _cat_chain_tensors(n):
    """The seeded host tensors of _run_bneck_cat_chain (NCHW / OIHW): t2, x, w3, wd, bcat, w1, b1."""
    g = torch.Generator().manual_seed(5100 + n)
    t2 = _rand_bf16((n, 128, 28, 28), g)
    x = _rand_bf16((n, 256, 56, 56), g)
    w3 = _rand_bf16((512, 128, 1, 1), g, scale=(1.0 / 128) ** 0.5)
    wd = _rand_bf16((512, 256, 1, 1), g, scale=(1.0 / 256) ** 0.5)
    bcat = torch.randn(512, generator=g) * 0.1
    w1 = _rand_bf16((128, 512, 1, 1), g, scale=(2.0 / 512) ** 0.5)
    b1 = torch.randn(128, generator=g) * 0.1
    return t2, x, w3, wd, bcat, w1, b1


def _run_bneck_cat_chain(n, tensors=None):
    """layer2.0's transition tail chained with layer2.1.conv1 (bneck_catchain_kernel): conv3 + downsample as one conv over K = [t2 | x at
    stride 2] + ReLU, then the next 1x1 + ReLU out of LDS -- BIT FOR BIT the two-source igemm launch followed by the 1x1 igemm launch it
    replaces (n = 1 / 3: fewer tiles than CUs, ragged tiles; 37: full tiles + a ragged one; 256: the benchmarked 1792 tiles, 7 per workgroup),
    nothing stored past M; the small cases also against the oracle's emulation.
    ``tensors``: host tensors in _cat_chain_tensors' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    from oracle.resnet50_oracle import conv_bias_act_emulated
    t2, x, w3, wd, bcat, w1, b1 = tensors or _cat_chain_tensors(n)
    fmt, mant = _fmt_of(t2)
    d = _dev()
    t2d = t2.permute(0, 2, 3, 1).contiguous().to(d)
    xd = x.permute(0, 2, 3, 1).contiguous().to(d)
    wcat = torch.cat([w3.view(512, 128), wd.view(512, 256)], dim=1).contiguous().to(d)
    w1d = w1.view(128, 512).contiguous().to(d)
    bcd, b1d = bcat.to(d), b1.to(d)
    out, y1n = ops.bneck_cat_chain_bf16(t2d, xd, wcat, bcd, w1d, b1d)
    torch.cuda.synchronize()
    out_u = ops.conv1x1_cat(t2d, xd, 2, wcat, bcd, relu=True)
    y1_u = ops.conv2d_bf16(out_u, w1d.view(128, 1, 1, 512), b1d, relu=True)
    assert torch.equal(out, out_u), "chained block output differs from the two-source igemm launch"
    assert torch.equal(y1n, y1_u), "chained next-conv1 output differs from the igemm launch"
    if n <= 3:
        xs = x[:, :, ::2, ::2]
        ref = conv_bias_act_emulated(torch.cat([t2, xs], dim=1).float(), torch.cat([w3, wd], dim=1).float(), bcat, 1, 0, True, fmt=fmt)
        _check_bf16(out, ref, "bneck_cat_chain out", mant)
        y1_ref = conv_bias_act_emulated(out.float().cpu().permute(0, 3, 1, 2), w1.float(), b1, 1, 0, True, fmt=fmt)
        _check_bf16(y1n, y1_ref, "bneck_cat_chain y1n", mant)
    return out, y1n


@pytest.mark.parametrize("n", [1, 5, 256], ids=lambda v: "n%d" % v)
def test_layer3_last_block_conv3_through_the_pipelined_tail(lib_built, n):
    _run_layer3_last_block(n)


def _run_layer3_last_block(n, tensors=None):
    """layer3.5: conv3 + identity + ReLU through bneck_tail3p_kernel<.., NOB> (no second GEMM; group B only copies out_c out) -- bit for bit the
    igemm launch with a residual it replaces; nothing written past M.
    ``tensors``: host tensors in _tail3_inputs' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    y2, w3, b3, idn, _w1, _b1 = tensors or _tail3_inputs(n, 14, 14, 4100 + n)
    d = _dev()
    y2d = y2.permute(0, 2, 3, 1).contiguous().to(d)
    idd = idn.permute(0, 2, 3, 1).contiguous().to(d)
    w3d, b3d = w3.view(1024, 256).contiguous().to(d), b3.to(d)
    out = ops.conv3_identity_tail3_bf16(y2d, w3d, b3d, idd)
    out_u = ops.conv2d_bf16(y2d, w3d.view(1024, 1, 1, 256), b3d, relu=True, residual=idd)
    assert torch.equal(out, out_u)
    return out


FP16_CASES = [CONV_CASES[i] for i in (1, 2, 3, 5, 6, 10, 12)]


@pytest.mark.parametrize("case", FP16_CASES, ids=lambda c: "n%d_%dx%d_c%d-%d_k%ds%dp%d_r%d_res%d" % tuple(int(v) for v in c))
def test_conv2d_fp16_matches_oracle(lib_built, case):
    """The same kernels with IEEE half as the element type (R50_PREC_FP16), every tile variant: within one fp16 ulp of
    the oracle's fused-op emulation with fp16 rounding points."""
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xd, wd, bd, rd, ref, _ = _conv_inputs(case, torch.float16)
    tiles = _tiles_for(cout, k, pad)
    if n >= 64:                      # the big case is there for the tile STREAM of the persistent kernels: the small tiles add nothing
        tiles = [ops.TILE_AUTO, ops.TILE_256x256 | ops.PERSISTENT, ops.WS | 8, ops.TILE_G8, ops.TILE_G8_224]
    if (h, w, cin, cout, k, stride, pad, has_res) == (56, 56, 64, 64, 3, 1, 1, False):
        tiles = tiles + [ops.TILE_C64]
    for tile in tiles:
        y = ops.conv2d_bf16(xd, wd, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile)
        _check_fp16(y, ref, f"fp16 conv tile={tile}")


def test_conv2d_fp16_saturates_instead_of_overflowing(lib_built):
    """fp16 mode converts with a clamp at +-65504: an accumulator beyond the half range must come out as the largest
    finite half, never as infinity (a single inf would poison every later layer)."""
    from implementation_phd_lab_vision_amd import ops
    d = _dev()
    x = torch.full((1, 4, 4, 64), 200.0, dtype=torch.float16, device=d)
    w = torch.full((64, 1, 1, 64), 30.0, dtype=torch.float16, device=d)          # 64 * 200 * 30 = 384,000 > 65,504
    w[1::2] = -30.0
    y = ops.conv2d_bf16(x, w, torch.zeros(64, device=d), relu=False, tile=ops.TILE_64x128)
    assert torch.isfinite(y).all()
    assert bool((y[..., 0::2] == 65504.0).all()) and bool((y[..., 1::2] == -65504.0).all())


def test_conv2d_identity_asymmetric(lib_built):
    """A = I check with an asymmetric B (cdna guide §3): 1x1 conv with identity weights must return
    the input exactly; a transposed operand or C/D map cannot pass."""
    from implementation_phd_lab_vision_amd import ops
    d = _dev()
    n, h, w, c = 2, 6, 5, 128
    x = torch.arange(n * h * w * c, dtype=torch.float32).remainder(251.0).sub(125.0).view(n, h, w, c).to(torch.bfloat16)
    wt = torch.eye(c).view(c, 1, 1, c).to(torch.bfloat16)
    for tile in (ops.TILE_64x128, ops.TILE_128x128, ops.TILE_128x64, ops.TILE_64x256, ops.TILE_128x256_P3,
                 ops.TILE_128x128_P3):
        for mode in (0, ops.PERSISTENT):
            y = ops.conv2d_bf16(x.to(d), wt.to(d), torch.zeros(c, device=d), relu=False, tile=tile | mode)
            assert torch.equal(y.cpu(), x), f"identity conv mismatch, tile {tile} mode {mode}"


def test_conv2d_rejects_bad_shapes(lib_built):
    from implementation_phd_lab_vision_amd import ops, _lib
    d = _dev()
    x = torch.zeros((1, 4, 4, 32), dtype=torch.bfloat16, device=d)       # cin % 64 != 0
    wt = torch.zeros((64, 1, 1, 32), dtype=torch.bfloat16, device=d)
    with pytest.raises(_lib.R50Error):
        ops.conv2d_bf16(x, wt, torch.zeros(64, device=d))


@pytest.mark.parametrize("n", [1, 3])
def test_stem_matches_oracle(lib_built, n):
    from implementation_phd_lab_vision_amd import ops
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from oracle.resnet50_oracle import bf16_round, conv_bias_act_emulated, folded
    sd = synthetic_state_dict(0)
    wf, bf = folded(sd, "conv1", "bn1")
    x = synthetic_frames(n, seed=7)
    ref = conv_bias_act_emulated(bf16_round(x), wf, bf, 2, 3, True)
    d = _dev()
    y = ops.stem_bf16(x.to(d), wf, bf.to(d))
    torch.cuda.synchronize()
    _check_bf16(y, ref, "stem")


@pytest.mark.parametrize("shape", [(2, 112, 112, 64), (1, 7, 9, 8), (3, 5, 5, 72)])
def test_maxpool_bit_exact(lib_built, shape):
    from implementation_phd_lab_vision_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(11)
    x = _rand_bf16(shape, g)                       # negative values too: padding must act as -inf
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    y = ops.maxpool_bf16(x.to(_dev()))
    assert torch.equal(y.float().cpu(), ref)


@pytest.mark.parametrize("et", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_maxpool_bit_exact_on_subnormals_and_signed_zeros(lib_built, et):
    """The same pool on an input of subnormals of both signs (bf16: bit patterns 0x0001 .. 0x007f, fp32 subnormals once unpacked; fp16:
    0x0001 .. 0x03ff), +0, -0 and the smallest normals, in equal shares: the maximum is one of the inputs, bit for bit -- a max or a
    conversion that flushed subnormals would return 0 or the wrong sign.  Only the sign of a zero maximum is left open (max(+0, -0))."""
    from implementation_phd_lab_vision_amd import ops
    import torch.nn.functional as F
    shape = (2, 7, 9, 16)
    first_normal = 0x0080 if et == torch.bfloat16 else 0x0400
    g = torch.Generator().manual_seed(12)
    bits = torch.randint(0x0001, first_normal, shape, generator=g, dtype=torch.int32)             # subnormal magnitudes
    kind = torch.randint(0, 4, shape, generator=g)
    bits = torch.where(kind == 2, torch.zeros_like(bits), bits)                                    # zeros
    bits = torch.where(kind == 3, torch.randint(first_normal, 4 * first_normal, shape, generator=g, dtype=torch.int32), bits)
    bits = bits | (torch.randint(0, 2, shape, generator=g, dtype=torch.int32) << 15)
    x = bits.to(torch.int16).view(et)
    tiny = torch.tensor(first_normal, dtype=torch.int16).view(et).double()
    assert bool((x == 0).any()) and bool(((x.double().abs() > 0) & (x.double().abs() < tiny)).any()) and bool((x.double().abs() >= tiny).any())
    ref = F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    y = ops.maxpool_bf16(x.to(_dev())).cpu()
    assert y.dtype == et
    assert torch.equal(y.double(), ref), f"{int((y.double() != ref).sum())} of {ref.numel()} maxima differ; zeros where the reference has none: " \
                                         f"{int(((y.double() == 0) & (ref != 0)).sum())}"
    nz = ref != 0
    assert torch.equal(y.view(torch.int16)[nz], ref.to(et).view(torch.int16)[nz]) and int(nz.sum()) > ref.numel() // 2


@pytest.mark.parametrize("shape", [(4, 7, 7, 2048), (1, 3, 3, 8)])
def test_avgpool_matches_oracle(lib_built, shape):
    from implementation_phd_lab_vision_amd import ops
    g = torch.Generator().manual_seed(13)
    x = _rand_bf16(shape, g)
    n, h, w, c = shape
    ref = x.double().view(n, h * w, c).mean(dim=1)
    y = ops.avgpool_bf16(x.to(_dev())).cpu().double()
    assert torch.allclose(y, ref, rtol=1e-5, atol=1e-6), float((y - ref).abs().max())


@pytest.mark.parametrize("et", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CAT_CASES, ids=lambda c: "n%d_%dx%d_c%d_src%d_c%d_s%d_o%d_r%d_t%d" % (c[0], c[1], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]))
def test_conv1x1_two_k_sources(lib_built, case, et):
    _run_conv1x1_cat(case, et)


def _cat_tensors(case, et):
    """The seeded host tensors of _run_conv1x1_cat (NHWC, wcat (cout, c1 + c2)): x1, x2, wcat, bias."""
    n, h, c1, h2, c2, s2, cout, relu, tile = case
    g = torch.Generator().manual_seed(h * 131 + c2)
    x1 = (torch.randn(n, h, h, c1, generator=g)).to(et)
    x2 = (torch.randn(n, h2, h2, c2, generator=g)).to(et)
    wcat = (torch.randn(cout, c1 + c2, generator=g) * (1.0 / (c1 + c2)) ** 0.5).to(et)
    bias = torch.randn(cout, generator=g) * 0.1
    return x1, x2, wcat, bias


def _run_conv1x1_cat(case, et, tensors=None):
    """One 1x1 conv over K = [x1 | x2 at stride2] (conv3 + downsample + add + ReLU of a stage's first bottleneck) against a wide
    accumulation of the same sum; a poisoned guard band behind the output must stay untouched.
    ``tensors``: host tensors in _cat_tensors' order and layout instead of the seeded ones."""
    import torch.nn.functional as F
    from implementation_phd_lab_vision_amd import ops
    n, h, c1, h2, c2, s2, cout, relu, tile = case
    x1, x2, wcat, bias = tensors or _cat_tensors(case, et)
    y = ops.conv1x1_cat(x1.to("cuda:0"), x2.to("cuda:0"), s2, wcat.to("cuda:0"), bias.to("cuda:0"), relu=relu, tile=tile)
    ref = F.conv2d(x1.double().permute(0, 3, 1, 2), wcat[:, :c1].double().view(cout, c1, 1, 1))
    ref = ref + F.conv2d(x2.double().permute(0, 3, 1, 2), wcat[:, c1:].double().view(cout, c2, 1, 1), stride=s2)
    ref = ref + bias.double().view(1, -1, 1, 1)
    if relu:
        ref = F.relu(ref)
    ref = ref.float()
    if et == torch.float16:
        ref = ref.clamp(-65504.0, 65504.0)                 # the fp16 conversion saturates (test_conv2d_fp16_saturates_instead_of_overflowing)
    ref = ref.to(et).float()
    got = y.float().cpu().permute(0, 3, 1, 2)
    diff = (got - ref).abs()
    ulp = ref.abs() * (2.0 ** -7 if et == torch.bfloat16 else 2.0 ** -10) + 2.0 ** -16 * max(1.0, float(ref.abs().max()))
    assert not (diff > ulp).any(), float(diff.max())
    assert float((diff > 0).float().mean()) < 0.01
    with pytest.raises(Exception):
        ops.conv1x1_cat(x1.to("cuda:0"), x2.to("cuda:0"), s2 + 1, wcat.to("cuda:0"), bias.to("cuda:0"))      # geometry mismatch
    with pytest.raises(Exception):
        ops.conv1x1_cat(x1.to("cuda:0"), x2.to("cuda:0"), s2, wcat.to("cuda:0"), bias.to("cuda:0"), tile=1)  # not a role-specialised tile
    return y


@pytest.mark.parametrize("case", FP8_CASES, ids=lambda c: "n%d_%dx%d_c%d_o%d_k%d_s%d_p%d_r%d_res%d_t%d" % tuple(int(v) for v in c))
def test_conv2d_fp8(lib_built, case):
    _run_conv2d_fp8(case)


def _fp8_tensors(case):
    """The seeded host tensors of _run_conv2d_fp8 (NHWC / OHWI e4m3): xq, wq, bias, rq or None, and the scales (sx, sw, sr, sy)."""
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res, tile = case
    g = torch.Generator().manual_seed(cin * 7 + cout + k)
    sx, sw, sr, sy = 0.05, 0.002, 0.04, 0.03
    xq = (torch.randn(n, h, w, cin, generator=g) * 1.0 / sx * 0.5).clamp(-448, 448).to(ops.FP8)
    wq = (torch.randn(cout, k, k, cin, generator=g) * (1.0 / (k * k * cin)) ** 0.5 / sw).clamp(-448, 448).to(ops.FP8)
    bias = torch.randn(cout, generator=g) * 0.1
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    rq = (torch.randn(n, ho, wo, cout, generator=g) / sr * 0.5).clamp(-448, 448).to(ops.FP8) if has_res else None
    return xq, wq, bias, rq, (sx, sw, sr, sy)


def _run_conv2d_fp8(case, tensors=None):
    """fp8 (e4m3) conv on the K = 128 scaled MFMA (BASELINE configs[4], kernel level) against a wide accumulation of the same
    quantised operands, requantised with torch's round-to-nearest-even fp8 conversion.
    ``tensors``: host tensors and scales in _fp8_tensors' order and layout instead of the seeded ones."""
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res, tile = case
    xq, wq, bias, rq, (sx, sw, sr, sy) = tensors or _fp8_tensors(case)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    y = ops.conv2d_fp8(xq.to("cuda:0"), sx, wq.to("cuda:0"), sw, bias.to("cuda:0"), sy, stride=stride, pad=pad, relu=bool(relu),
                       residual=rq.to("cuda:0") if has_res else None, sr=sr, tile=tile)
    assert y.dtype == ops.FP8 and tuple(y.shape) == (n, ho, wo, cout)
    ref_q = fp8_reference(xq, wq, bias, rq, (sx, sw, sr, sy), stride, pad, relu).clamp(-448, 448).float().to(ops.FP8).float()
    got = y.float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    diff = (got - ref_q).abs()
    # one fp8 step at most (3 mantissa bits: spacing <= |v| / 8; 2^-9 in the subnormal range), and only where the fp32 sum sits on a tie
    assert not (diff > ref_q.abs() * 0.126 + 2.0 ** -9 + 1e-7).any(), float(diff.max())
    assert float((diff > 0).float().mean()) < 0.02, float((diff > 0).float().mean())
    assert float(got.abs().max()) > 1.0                       # a real signal, not all zeros
    with pytest.raises(Exception):
        ops.conv2d_fp8(xq.to("cuda:0")[..., :64].contiguous(), sx, wq.to("cuda:0")[..., :64].contiguous(), sw, bias.to("cuda:0"), sy)   # cin % 128
    return y
