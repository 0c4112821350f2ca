"""Every persistent kernel under a capped workgroup count (option "cu_cap", process-wide; include/r50.h: "results bit-identical").

A persistent launch puts min(work items, CU budget) workgroups on the chip and each workgroup walks its items with
``item += gridDim.x``, carrying LDS rings, prefetched fragments and barrier phases from one item to the next.  On 256 CUs the small
shapes of the suite give every workgroup ONE item, and the large ones always a stride of 256.  A cap of 1, 3 or 5 workgroups turns the
same small shapes into many items per workgroup, at every stride, with a ragged last round and image borders crossed in mid-stream.

What is asserted, and nothing else: (1) the suite's own check of each kernel (tests/test_kernels_gpu.py, tests/test_network_gpu.py:
same seeded inputs, same fp64 oracle, same bars, same guard bands) passes under each cap, and (2) ``torch.equal`` against the uncapped
launch of the same call.  No tolerance of its own appears in this file.

Item counts are restated here from the launchers (csrc/r50_abi.hip) so that a capped launch is known to give some workgroup more than
one item (``_must_stream``).  Where a listed case has no more items than a cap (the smallest shapes under the larger tiles), that
launch would be the uncapped launch over again: it is left out, and each test asserts that every cap still reached a launch.
"""
import contextlib

import pytest
import torch
from tests.network_oracles import _oracle_bar  # noqa: F401

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 5)
KNOBS = ("cu_cap", "stem_strip", "tail3_bp")        # process-wide options this file touches: each must read 0 when a test ends


# ---- the knob, safely -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cap(lib_built):
    """``cap(v)`` sets the process-wide workgroup cap through a small backbone's handle (``cap.bb``); whatever a test does, the cap
    (and the other process-wide knobs) are back at 0 when the module is done."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    bb = ResNet50Backbone(seed=0, max_batch=1).to("cuda:0").eval()

    def set_cap(v):
        bb.set_option("cu_cap", int(v))

    set_cap.bb = bb
    try:
        yield set_cap
    finally:
        for k in KNOBS:
            bb.set_option(k, 0)
        bb.close()


@pytest.fixture(autouse=True)
def knobs_read_zero_when_a_test_ends(cap):
    yield
    left = {k: cap.bb.get_option(k) for k in KNOBS}
    for k in KNOBS:                                   # a failing test must not leave the rest of the GPU suite capped
        cap.bb.set_option(k, 0)
    assert all(v == 0 for v in left.values()), f"a test left process-wide knobs set: {left}"


@contextlib.contextmanager
def _capped(cap, v):
    cap(v)
    try:
        yield
    finally:
        cap(0)


@contextlib.contextmanager
def _option(bb, key, v, restore=0):
    bb.set_option(key, v)
    try:
        yield
    finally:
        bb.set_option(key, restore)


# ---- the launchers' arithmetic (csrc/r50_abi.hip), restated -------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _budget(v):                                       # cu_budget()
    return v if 0 < v < _cus() else _cus()


def _ceil(a, b):
    return (a + b - 1) // b


def _streams(items, v, per_cu=1):
    """More items than the capped grid has workgroups: some workgroup walks at least two."""
    return items > _budget(v) * per_cu


def _must_stream(items, v, what, per_cu=1):
    assert _streams(items, v, per_cu), f"{what}: {items} items on {_budget(v) * per_cu} workgroups -- the cap changes nothing here"


# igemm_bf16_kernel tiles: id -> (couts, pixels, waves over couts, waves over pixels, LDS stages); launch_igemm_t
_GENERIC = {1: (128, 128, 2, 2, 2), 2: (64, 128, 1, 4, 2), 3: (64, 256, 1, 4, 2), 5: (128, 64, 2, 2, 2), 6: (256, 128, 4, 2, 3),
            7: (128, 256, 2, 4, 3), 8: (128, 128, 2, 4, 3), 9: (256, 256, 4, 2, 2), 10: (256, 256, 2, 4, 2), 11: (256, 208, 8, 1, 2),
            12: (256, 224, 4, 2, 2)}
# igemm_ws_kernel / gemm8p_kernel tiles: id & 31 -> (couts, pixels); one workgroup per CU
_WS = {1: (128, 128), 3: (256, 128), 4: (128, 224), 8: (128, 224), 9: (64, 224), 10: (128, 208), 19: (256, 256), 20: (256, 224)}


def _igemm_items(tile, m, cout):
    """(tiles of the launch, upper bound of the resident workgroups per CU the launcher multiplies the budget with)."""
    from implementation_phd_lab_vision_amd import ops
    if tile & ops.WS:
        bc, bp = _WS[tile & 31]
        return (cout // bc) * _ceil(m, bp), 1
    assert tile & ops.PERSISTENT
    bc, bp, wc, wp, nst = _GENERIC[tile & 31]
    rows = wc * wp * 8
    lds = nst * (bc + _ceil(bp, rows) * rows) * 128
    # the launcher asks the runtime for the occupancy; LDS (160 KiB per CU) and the 32 wave slots of a CU bound it from above
    return (cout // bc) * _ceil(m, bp), max(1, min(163840 // lds, 32 // (wc * wp)))


def _xres_items(n, hw, c):                           # launch_conv3x3_xres_t: images per tile x row bands x cout tiles
    ni, bands = {14: (1, 1), 28: (1, 4), 7: (4, 1)}[hw]
    return _ceil(n, ni) * bands * (c // 128)


def _s2_items(n, hw, c):                             # launch_conv3x3_s2_t (hw = input size)
    return (_ceil(n, 4) if hw == 14 else n * (4 if hw == 56 else 1)) * (c // 128)


def _tail3_tiles(m, v, bp_override=0):               # launch_bneck_tail3 -> (pixels per tile, tiles)
    b = _budget(v)
    rounds = _ceil(_ceil(m, 112), b)
    bp = min(112, max(49, _ceil(m, rounds * b)))
    if _ceil(m, 112) > b:
        bp = 112
    if 1 <= bp_override <= 112:
        bp = bp_override
    return bp, _ceil(m, bp)


def _catchain_tiles(m, v):                           # launch_bneck_catchain -> (pixels per tile, tiles)
    b = _budget(v)
    bp = 112
    if _ceil(m, 112) <= b:
        bp = min(112, max(16, _ceil(m, b)))
    return bp, _ceil(m, bp)


def _stem_strips(n, strip):                          # launch_stem_fused
    g = strip
    if g == 0:
        g = next((c for c in (28, 14, 7, 4, 2) if n * (28 // c) >= 200), 1)
    return n * (28 // g)


class _Reached:
    """Counts the capped launches of a test per cap; ``done()`` asserts that no cap went without one."""

    def __init__(self, caps):
        self.n = {v: 0 for v in caps}

    def hit(self, v):
        self.n[v] += 1

    def done(self, caps=None):
        missing = [v for v in (caps or self.n) if self.n[v] == 0]
        assert not missing, f"no launch streamed items under cap(s) {missing}: {self.n}"


# ---- 1. op level ------------------------------------------------------------------------------------------------------------------
CONV_CAPPED = [
    (2, 14, 14, 256, 256, 3, 1, 1, True, False),
    (2, 9, 9, 128, 128, 3, 2, 1, True, False),
    (3, 9, 9, 64, 256, 1, 1, 0, False, False),
    (5, 14, 14, 512, 512, 1, 1, 0, True, True),
    (3, 12, 12, 256, 256, 1, 2, 0, True, False),
]
_CONV_IDS = lambda c: "n%d_%dx%d_c%d-%d_k%ds%dp%d_r%d_res%d" % tuple(int(v) for v in c)      # noqa: E731
_ET = pytest.mark.parametrize("et", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _conv_under_caps(cap, case, inputs, tiles_items, caps=CAPS):
    """tiles_items: [(tile id, items, per-CU bound)].  Per tile: the suite's check at cap 0, then under every cap that makes a workgroup
    walk several items the same check again and the uncapped bits."""
    from tests.test_kernels_gpu import _conv_tile_check
    reached = _Reached(caps)
    for tile, items, per_cu in tiles_items:
        y0 = _conv_tile_check(case, inputs, tile).clone()
        for v in caps:
            if not _streams(items, v, per_cu):
                continue
            _must_stream(items, v, f"conv tile {tile}", per_cu)
            with _capped(cap, v):
                y = _conv_tile_check(case, inputs, tile)
            assert torch.equal(y, y0), f"conv tile {tile}, cap {v}: {int((y != y0).sum())} elements differ from the uncapped launch"
            reached.hit(v)
    return reached


@_ET
@pytest.mark.parametrize("case", CONV_CAPPED, ids=_CONV_IDS)
def test_conv2d_persistent_and_role_specialised_tiles(cap, case, et):
    """r50_op_conv2d / _f16: t | PERSISTENT for every generic tile, the role-specialised tiles and both eight-phase GEMM tiles."""
    from implementation_phd_lab_vision_amd import ops
    from tests.test_kernels_gpu import CONV_CASES, _conv_inputs, _tiles_for
    assert case in CONV_CASES
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    inputs = _conv_inputs(case, et)
    ho, wo = inputs[5]
    tiles = [t for t in _tiles_for(cout, k, pad) if t & (ops.PERSISTENT | ops.WS)]
    assert ops.WS | 9 in tiles and ops.TILE_64x128 | ops.PERSISTENT in tiles
    reached = _conv_under_caps(cap, case, inputs, [(t,) + _igemm_items(t, n * ho * wo, cout) for t in tiles])
    # the two smallest listed cases: 50 output pixels (3x3 stride 2 on 9x9) are two tiles at the most, 108 (1x1 stride 2 on 12x12) four
    reached.done({50: (1,), 108: (1, 3)}.get(n * ho * wo, CAPS))


@_ET
def test_resident_weights_3x3(cap, et):
    """TILE_C64 (conv3x3_c64_kernel) at 3 x 56 x 56: 42 tiles."""
    from implementation_phd_lab_vision_amd import ops
    from tests.test_kernels_gpu import CONV_CASES, _conv_inputs
    case = (3, 56, 56, 64, 64, 3, 1, 1, True, False)
    assert case in CONV_CASES
    for v in CAPS:
        _must_stream(14 * case[0], v, "conv3x3_c64")
    _conv_under_caps(cap, case, _conv_inputs(case, et), [(ops.TILE_C64, 14 * case[0], 1)]).done()


@_ET
@pytest.mark.parametrize("shape", [(5, 7, 512), (3, 28, 128), (3, 14, 256)], ids=lambda v: "n%d_%dx%d_c%d" % (v[0], v[1], v[1], v[2]))
def test_input_resident_3x3(cap, shape, et):
    """TILE_XRES (conv3x3_xres_kernel): 8 / 12 / 6 tiles; against the oracle, the uncapped bits, and (bf16, as the suite has it) every
    image the bits of the image run alone."""
    from implementation_phd_lab_vision_amd import ops
    from tests.test_kernels_gpu import CONV_CASES, _conv_inputs, _run_xres_batch_invariance
    n, hw, c = shape
    case = next(cc for cc in CONV_CASES if cc[:5] == (n, hw, hw, c, c) and cc[5:8] == (3, 1, 1))
    items = _xres_items(n, hw, c)
    for v in CAPS:
        _must_stream(items, v, "conv3x3_xres")
    _conv_under_caps(cap, case, _conv_inputs(case, et), [(ops.TILE_XRES, items, 1)]).done()
    if et == torch.bfloat16:
        y0 = _run_xres_batch_invariance(shape).clone()
        for v in CAPS:
            with _capped(cap, v):
                assert torch.equal(_run_xres_batch_invariance(shape), y0), f"cap {v}"


@_ET
@pytest.mark.parametrize("shape", [(3, 56, 128), (2, 28, 256), (5, 14, 512)], ids=lambda v: "n%d_%dx%d_c%d" % (v[0], v[1], v[1], v[2]))
def test_polyphase_stride2_3x3(cap, shape, et):
    """TILE_S2 (conv3x3_s2_kernel): 12 / 4 / 8 tiles (2 x 28 x 28: four tiles, so caps 1 and 3 only)."""
    from implementation_phd_lab_vision_amd import ops
    from tests.test_kernels_gpu import CONV_CASES, _conv_inputs, _run_s2_batch_invariance
    n, hw, c = shape
    case = next(cc for cc in CONV_CASES if cc[:5] == (n, hw, hw, c, c) and cc[5:8] == (3, 2, 1))
    items = _s2_items(n, hw, c)
    caps = tuple(v for v in CAPS if _streams(items, v))
    assert caps == (CAPS if items > 5 else (1, 3))
    _conv_under_caps(cap, case, _conv_inputs(case, et), [(ops.TILE_S2, items, 1)], caps).done()
    if et == torch.bfloat16:
        y0 = _run_s2_batch_invariance(shape).clone()
        for v in caps:
            with _capped(cap, v):
                assert torch.equal(_run_s2_batch_invariance(shape), y0), f"cap {v}"


@_ET
def test_conv1x1_two_k_sources(cap, et):
    """r50_op_conv1x1_cat with the role-specialised and eight-phase tiles (2 .. 16 tiles)."""
    from tests.test_kernels_gpu import CAT_CASES, _run_conv1x1_cat
    cases = [c for c in CAT_CASES if c[8] in (64 | 1, 64 | 4, 64 | 3, 83, 84)]
    assert len(cases) == 7
    reached = _Reached(CAPS)
    for case in cases:
        n, h, _c1, _h2, _c2, _s2, cout, _relu, tile = case
        items, _ = _igemm_items(tile, n * h * h, cout)
        y0 = _run_conv1x1_cat(case, et).clone()
        for v in CAPS:
            if not _streams(items, v):
                continue
            _must_stream(items, v, f"conv1x1_cat tile {tile}")
            with _capped(cap, v):
                assert torch.equal(_run_conv1x1_cat(case, et), y0), f"{case}, cap {v}"
            reached.hit(v)
    reached.done()


def test_conv2d_fp8(cap):
    """r50_op_conv2d_fp8 with its role-specialised tiles.  The suite's fp8 cases are one to four tiles each: caps 1 and 3 split them."""
    from tests.test_kernels_gpu import FP8_CASES, _run_conv2d_fp8
    cases = [c for c in FP8_CASES if c[10] & 64]
    assert len(cases) == 6
    reached = _Reached(CAPS)
    for case in cases:
        n, h, w, _cin, cout, k, stride, pad, _relu, _res, tile = case
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        items, _ = _igemm_items(tile, n * ho * wo, cout)
        y0 = _run_conv2d_fp8(case).view(torch.uint8).clone()
        for v in CAPS:
            if not _streams(items, v):
                continue
            _must_stream(items, v, f"conv2d_fp8 tile {tile}")
            with _capped(cap, v):
                assert torch.equal(_run_conv2d_fp8(case).view(torch.uint8), y0), f"{case}, cap {v}"
            reached.hit(v)
    reached.done((1, 3))


def _pair_equal(a, b, what):
    for x, y, name in zip(a, b, ("block output", "next conv1")):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y), f"{what}: {name} differs from the uncapped launch in {int((x != y).sum())} elements"


@pytest.mark.parametrize("ds", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("shape,c1", [((3, 5, 16), 64), ((1, 56, 56), 128)], ids=lambda v: str(v).replace(" ", ""))
def test_bneck_tail_layer1(cap, shape, c1, ds):
    """bneck_tail_kernel: a workgroup of NT / 64 waves takes that many 16-pixel tiles per round (15 tiles: 4 or 2 rounds; 196: 49 or 25)."""
    from tests.test_kernels_gpu import _run_bneck_tail
    n, h, w = shape
    items = _ceil(_ceil(n * h * w, 16), 8 if ds else 4)          # TAIL_NT_DS = 512 threads, 256 otherwise
    caps = tuple(v for v in CAPS if _streams(items, v))
    assert caps == (CAPS if items > 5 else ((1, 3) if items > 3 else (1,)))
    ref = [t.clone() for t in _run_bneck_tail(shape, c1, ds)]
    for v in caps:
        _must_stream(items, v, "bneck_tail")
        with _capped(cap, v):
            _pair_equal(_run_bneck_tail(shape, c1, ds), ref, f"cap {v}")


@pytest.mark.parametrize("shape", [(3, 5, 16), (1, 28, 28)], ids=lambda v: str(v).replace(" ", ""))
def test_bneck_tail_layer2(cap, shape):
    """bneck_tail2_kernel: 15 / 49 steps of 16 pixels."""
    from tests.test_kernels_gpu import _run_bneck_tail_layer2
    n, h, w = shape
    items = _ceil(n * h * w, 16)
    ref = [t.clone() for t in _run_bneck_tail_layer2(shape)]
    for v in CAPS:
        _must_stream(items, v, "bneck_tail2")
        with _capped(cap, v):
            _pair_equal(_run_bneck_tail_layer2(shape), ref, f"cap {v}")


@pytest.mark.parametrize("shape,bp", [((3, 14, 14), 0), ((5, 14, 14), 33)], ids=lambda v: str(v).replace(" ", ""))
def test_bneck_tail_layer3_chained(cap, shape, bp, monkeypatch):
    """bneck_tail3p_kernel.  Its tile height follows the CU budget: 49 pixels (12 tiles) on the whole chip and under cap 100, full
    112-pixel tiles (6) under caps 1, 3, 5; 33 forced: 30 tiles.  Every height keeps each output pixel's summation order, so the bits are
    the uncapped ones (and, inside the suite's check, those of the two igemm launches)."""
    from tests.test_kernels_gpu import _run_bneck_tail_layer3
    monkeypatch.delenv("R50_TAIL3_BP", raising=False)           # the op hook's own override: the option is what is under test
    n, h, w = shape
    m = n * h * w
    with _option(cap.bb, "tail3_bp", bp):
        ref = [t.clone() for t in _run_bneck_tail_layer3(shape, bp)]
        for v in CAPS + (100,):
            height, tiles = _tail3_tiles(m, v, bp)
            if v != 100:                                        # cap 100 is there for the tile height it derives, not for a stream
                _must_stream(tiles, v, "bneck_tail3p")
                assert height == (bp or 112)
            with _capped(cap, v):
                _pair_equal(_run_bneck_tail_layer3(shape, bp), ref, f"cap {v} ({tiles} tiles of {height})")
    assert _tail3_tiles(588, 0) == (49, 12) and _tail3_tiles(588, 100) == (49, 12) and _tail3_tiles(588, 5) == (112, 6)


def test_layer3_last_block(cap):
    """bneck_tail3p_kernel<.., NOB> at n = 5: 20 tiles of 49 uncapped, 9 full tiles under caps 1, 3, 5."""
    from tests.test_kernels_gpu import _run_layer3_last_block
    ref = _run_layer3_last_block(5).clone()
    for v in CAPS:
        height, tiles = _tail3_tiles(980, v)
        assert (height, tiles) == (112, 9)
        _must_stream(tiles, v, "bneck_tail3p (last block)")
        with _capped(cap, v):
            assert torch.equal(_run_layer3_last_block(5), ref), f"cap {v}"


@pytest.mark.parametrize("c1", [64, 128])
def test_bneck_block1(cap, c1):
    """bneck_block1_kernel at n = 3: 42 four-row tiles."""
    from tests.test_kernels_gpu import _run_bneck_block1
    ref = [t.clone() for t in _run_bneck_block1(3, c1)]
    for v in CAPS:
        _must_stream(14 * 3, v, "bneck_block1")
        with _capped(cap, v):
            _pair_equal(_run_bneck_block1(3, c1), ref, f"cap {v}")


def test_bneck_block1_downsample(cap):
    """bneck_block1_kernel<.., DS> at n = 3: 42 tiles."""
    from tests.test_kernels_gpu import _run_bneck_block1_ds
    ref = [t.clone() for t in _run_bneck_block1_ds(3)]
    for v in CAPS:
        _must_stream(14 * 3, v, "bneck_block1 (downsample)")
        with _capped(cap, v):
            _pair_equal(_run_bneck_block1_ds(3), ref, f"cap {v}")


@pytest.mark.parametrize("chain", [False, True], ids=["last_block", "chained_conv1"])
def test_bneck_block2(cap, chain):
    """bneck_block2_kernel at n = 3: 12 seven-row tiles."""
    from tests.test_kernels_gpu import _run_bneck_block2
    ref = [None if t is None else t.clone() for t in _run_bneck_block2(3, chain)]
    for v in CAPS:
        _must_stream(4 * 3, v, "bneck_block2")
        with _capped(cap, v):
            _pair_equal(_run_bneck_block2(3, chain), ref, f"cap {v}")


def test_bneck_cat_chain(cap):
    """bneck_catchain_kernel at n = 3 (2,352 pixels).  Its tile height follows the CU budget: 147 tiles of 16 on the whole chip, 21 full
    tiles under caps 1, 3, 5 (cap 1: all of them on one workgroup), 98 tiles of 24 under cap 100."""
    from tests.test_kernels_gpu import _run_bneck_cat_chain
    m = 3 * 28 * 28
    assert _catchain_tiles(m, 0) == (16, 147) and _catchain_tiles(m, 1) == (112, 21) and _catchain_tiles(m, 100) == (24, 98)
    ref = [t.clone() for t in _run_bneck_cat_chain(3)]
    for v in CAPS + (100,):
        height, tiles = _catchain_tiles(m, v)
        if v != 100:
            _must_stream(tiles, v, "bneck_catchain")
        with _capped(cap, v):
            _pair_equal(_run_bneck_cat_chain(3), ref, f"cap {v} ({tiles} tiles of {height})")


# ---- 2. the fused stem ------------------------------------------------------------------------------------------------------------
# single-pixel impulses of frame 2: the four corners, the middle of each edge, one interior position (row, column, channel)
IMPULSES = [(0, 0, 0), (0, 223, 1), (223, 0, 2), (223, 223, 0), (0, 112, 1), (223, 112, 2), (112, 0, 0), (112, 223, 1), (100, 77, 2)]
STRIPS = (0, 1, 2, 4, 7, 14, 28)


def _impulse_frame(background, values):
    f = torch.full((3, 224, 224), background)
    for i, (r, c, ch) in enumerate(IMPULSES):
        f[ch, r, c] = values[i % len(values)]
    return f


def _untouched_pooled_pixels():
    """(56, 56) mask of the pooled pixels whose receptive field holds no impulse: pooled row p reads conv rows 2p-1 .. 2p+1, conv row c
    reads input rows 2c-3 .. 2c+3, so pooled row p reads input rows 4p-5 .. 4p+5 (columns alike)."""
    p = torch.arange(56) * 4
    free = torch.ones(56, 56, dtype=torch.bool)
    for r, c, _ch in IMPULSES:
        free &= ~(((p - r).abs() <= 5).view(56, 1) & ((p - c).abs() <= 5).view(1, 56))
    return free


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def stem_setup(request, lib_built):
    """Backbone, the three frames, the bits of the unfused path (taken once, uncapped) and the oracle's stem / pool of the same frames."""
    import torch.nn.functional as F
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from oracle.resnet50_oracle import conv_bias_act_emulated, elem_round, folded
    fmt = request.param
    sd = synthetic_state_dict(0)
    x = torch.cat([synthetic_frames(1), torch.zeros(1, 3, 224, 224), _impulse_frame(0.0, [2.0]).unsqueeze(0)])
    bb = ResNet50Backbone(state_dict=sd, max_batch=4, precision=fmt).to("cuda:0").eval()
    xd = x.to("cuda:0")
    assert bb.get_option("fused_stem") == 1 and bb.get_option("fuse_stem_c1") == 1 and bb.get_option("cu_cap") == 0
    stem = bb.layer(xd, "stem").clone()                      # (the 'stem' tap alone forces the unfused path)
    with _option(bb, "fused_stem", 0, restore=1):
        pool_u = bb.layer(xd, "pool").clone()
        t1_u = bb.layer(xd, "layer1.0.t1").clone()
    assert torch.equal(pool_u.float(), F.max_pool2d(stem.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))
    with _option(bb, "fuse_stem_c1", 0, restore=1):
        t1_plain = bb.layer(xd, "layer1.0.t1").clone()
        f_plain = bb.features(xd).clone()
    wf, bf = folded(sd, "conv1", "bn1")
    stem_ref = conv_bias_act_emulated(elem_round(x, fmt), wf, bf, 2, 3, True, fmt=fmt)
    pool_ref = F.max_pool2d(stem_ref, 3, 2, 1)
    const = torch.relu(elem_round(bf, fmt)).to(pool_u.dtype).to("cuda:0")       # a zero frame: every conv output is the folded bias
    yield dict(fmt=fmt, bb=bb, xd=xd, pool_u=pool_u, t1_u=t1_u, t1_plain=t1_plain, f_plain=f_plain, stem_ref=stem_ref,
               pool_ref=pool_ref, const=const, free=_untouched_pooled_pixels().to("cuda:0"), mant=7 if fmt == "bf16" else 10)
    bb.close()


def _stem_statements(s, what):
    """(a) the bits of the unfused path, (b) the exact constants of the zero frame and of the impulse frame away from its impulses."""
    bb, xd = s["bb"], s["xd"]
    pool = bb.layer(xd, "pool")
    t1 = bb.layer(xd, "layer1.0.t1")
    const, free = s["const"], s["free"]
    # (b) first: it names the stale row, where (a) would only count differing elements
    bad = (pool[1] != const).any(dim=-1)
    assert not bool(bad.any()), f"{what}: zero frame, pooled pixels off the bias constant at (row, col) {bad.nonzero()[:8].tolist()}"
    bad = (pool[2] != const).any(dim=-1) & free
    assert not bool(bad.any()), f"{what}: impulse frame, pooled pixels outside every receptive field off the constant at {bad.nonzero()[:8].tolist()}"
    row = t1[1, 0, 0]
    bad = (t1[1] != row).any(dim=-1)
    assert not bool(bad.any()), f"{what}: zero frame, layer1.0.t1 is not one constant row at {bad.nonzero()[:8].tolist()}"
    bad = (t1[2] != row).any(dim=-1) & free
    assert not bool(bad.any()), f"{what}: impulse frame, layer1.0.t1 off the constant row at {bad.nonzero()[:8].tolist()}"
    assert torch.equal(pool, s["pool_u"]), f"{what}: pool differs from the unfused path in {int((pool != s['pool_u']).sum())} elements"
    assert torch.equal(t1, s["t1_u"]) and torch.equal(t1, s["t1_plain"]), f"{what}: layer1.0.t1 differs from its own igemm launch"
    assert torch.equal(bb.features(xd), s["f_plain"]), f"{what}: features differ"


def test_fused_stem_strips_and_caps(cap, stem_setup):
    """stem_fused3_kernel, float frames: every strip length x caps 0, 1, 3, 5.  Three frames = 84 strips of one pair .. 3 strips of 28:
    under cap 1 one workgroup walks them all, so the loud frame's last strip is followed by the zero frame's first in the same LDS rings."""
    from tests.test_kernels_gpu import _check_bf16
    s = stem_setup
    bb = s["bb"]
    _check_bf16(s["pool_u"], s["pool_ref"], "unfused pool", s["mant"])      # what every combination below equals bit for bit
    streamed = 0
    for strip in STRIPS:
        strips = _stem_strips(3, strip)
        assert strips == (84 if strip == 0 else 3 * 28 // strip)
        _must_stream(strips, 1, f"stem strip {strip}")
        with _option(bb, "stem_strip", strip):
            for v in (0,) + CAPS:
                streamed += _streams(strips, v)
                with _capped(cap, v):
                    _stem_statements(s, f"{s['fmt']} strip {strip} cap {v}")
    assert streamed == 7 + 6 + 6       # cap 1: every strip length; caps 3 and 5: all but whole-image strips (3 strips)


@pytest.mark.parametrize("strip", [0, 28])
def test_fused_stem_against_the_oracle_under_cap_1(cap, stem_setup, strip):
    """The fused kernel's own pool (and the stem tap) within one ulp of the oracle -- in fp16 too, where the op-level stem check does not reach."""
    from tests.test_kernels_gpu import _check_bf16
    s = stem_setup
    _must_stream(_stem_strips(3, strip), 1, "stem")
    with _option(s["bb"], "stem_strip", strip), _capped(cap, 1):
        stem = s["bb"].layer(s["xd"], "stem").clone()
        pool = s["bb"].layer(s["xd"], "pool").clone()
    _check_bf16(stem, s["stem_ref"], f"{s['fmt']} stem tap", s["mant"])
    _check_bf16(pool, s["pool_ref"], f"{s['fmt']} fused pool, strip {strip}, cap 1", s["mant"])


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fused_stem_uint8_frames(cap, precision):
    """The uint8 packer of the strip kernel (table look-up, 4-byte loads) under strips and caps: features_u8 gives the bits of the
    host-normalised float frames.  Frames: random, all 0, all 255, 128 with impulses of 0 and 255."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    g = torch.Generator().manual_seed(21)
    u8 = torch.randint(0, 256, (4, 3, 224, 224), generator=g, dtype=torch.uint8)
    u8[1] = 0
    u8[2] = 255
    u8[3] = _impulse_frame(128.0, [0.0, 255.0]).to(torch.uint8)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    x = ((u8.to(torch.float32) / 255.0 - mean) / std).to("cuda:0")           # the reference's host path
    u8d = u8.to("cuda:0")
    bb = ResNet50Backbone(seed=0, max_batch=4, precision=precision).to("cuda:0").eval()
    try:
        ref = bb.features(x).clone()
        assert torch.isfinite(ref).all()
        for strip in (0, 1, 28):
            strips = _stem_strips(4, strip)
            _must_stream(strips, 1, "stem (uint8)")
            with _option(bb, "stem_strip", strip):
                for v in (0, 1, 5):
                    with _capped(cap, v):
                        a = bb.features_u8(u8d)
                        b = bb.features(x)
                    assert torch.equal(a, b), f"strip {strip} cap {v}: uint8 frames differ from host-normalised frames"
                    assert torch.equal(b, ref), f"strip {strip} cap {v}: float frames differ from strip 0, cap 0"
    finally:
        bb.close()


# ---- 3. whole network -------------------------------------------------------------------------------------------------------------
NET_CAPS = (1, 5, 32, 100)


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp8", "bf16w2", "fp32x"])
def test_network_features_do_not_depend_on_the_cap(cap, precision):
    """Five frames through the whole stack under caps 1, 5, 32, 100: the features (and, in the 16-bit modes, every named activation, so
    that a failure names the first one that differs) are the uncapped bits; under cap 5 the mode's oracle check holds as it stands."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from tests.test_network_gpu import TAPS
    x = synthetic_frames(5, seed=77).to("cuda:0")
    assert cap.bb.get_option("cu_cap") == 0                   # fp8 calibrates at construction: uncapped
    bb = ResNet50Backbone(state_dict=synthetic_state_dict(0), max_batch=8, precision=precision).to("cuda:0").eval()
    taps = TAPS if precision in ("bf16", "fp16") else []
    try:
        f0 = bb.features(x).clone()
        assert torch.isfinite(f0).all()
        t0 = {name: bb.layer(x, name).clone() for name in taps}
        for v in NET_CAPS:
            if precision != "fp32x":                          # (fp32x has a stem of its own: one workgroup per tile)
                _must_stream(_stem_strips(5, 0), v, "stem")
            with _capped(cap, v):
                for name in taps:
                    assert torch.equal(bb.layer(x, name), t0[name]), f"cap {v}: {name} is the first activation that differs"
                f = bb.features(x)
                assert torch.equal(f, f0), f"cap {v}: {int((f != f0).sum())} feature values differ"
                if v == 5:
                    _oracle_bar(precision, bb)
    finally:
        bb.close()


def test_two_lanes_under_a_cap(cap):
    """backbone.BackboneLanes with every persistent grid capped at 100 workgroups -- sharing the chip between lanes is the use the knob
    was written for: each batch's features are the bits of one uncapped backbone, whatever lane it ran on."""
    from implementation_phd_lab_vision_amd.backbone import BackboneLanes, ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    dev = torch.device("cuda", 0)
    sd = synthetic_state_dict(0)
    one = ResNet50Backbone(state_dict=sd, max_batch=8).to(dev).eval()
    two = BackboneLanes(lanes=2, state_dict=sd, max_batch=8).to(dev).eval()
    try:
        xs = [synthetic_frames(n, seed=900 + n).to(dev) for n in (8, 5, 3, 8)]
        refs = [one.features(x).clone() for x in xs]
        torch.cuda.synchronize(dev)
        _must_stream(_stem_strips(8, 0), 100, "stem")
        with _capped(cap, 100):
            tickets = [two.submit(x) for x in xs]
            assert [t.lane for t in tickets] == [0, 1, 0, 1]
            for t, r in zip(tickets, refs):
                assert torch.equal(t.wait(), r)
            torch.cuda.synchronize(dev)
    finally:
        one.close()
        two.close()
