"""The two (head, tail) pair precisions, fp32x and bf16w2, held to per-kernel bars on the MI355X.

What runs: the conv launches of both modes through the debug hooks `r50_op_conv2d_w2` / `r50_op_conv2d_split` (the ConvArgs and launcher
of the network's own convs) on small ragged shapes, with explicit tile ids where the mode has them; every bottleneck conv of both networks
on the device's own input activations; the split pool kernels; the packed weight rows; and batch composition at the large-batch tile choices.
The oracles are plain torch in fp64 (tests/pair_reference.py, oracle/resnet50_oracle.py); tests/test_pair_modes_cpu.py shows that
every one-term defect of the arithmetic lies outside the bars used here.

bf16w2 bar: `_check_bf16` of tests/test_kernels_gpu.py (one bf16 ulp + 2^-16 of scale per element, < 1 % of elements differing, rel-L2
< 1e-3) against `conv_bias_act_emulated(..., weight_terms=2)`.

fp32x bar, per launch, against the exact fp64 conv of the pair values:
* element-wise |d| <= 2^-16 |ref| + 2^-16 max(1, max|ref|) (the form of `_check_bf16` with a 16-bit significand: the pair store and
  the dropped tail.tail products stay under 2^-17 relative, the absolute term is the suite's allowance for fp32 accumulation noise;
  `_check_bf16`'s count of differing elements compares two roundings to ONE format and has no meaning against an fp64 reference);
* rel-L2 < FP32X_REL_L2_BAR = 4 x the worst value measured with the correct kernels over the op-level cases and the network's
  53 launches, and never above 2.4e-4 (a quarter of the smallest one-term defect, 9.6e-4).  The arithmetic alone predicts ~5e-6
  plus about sqrt(3K) 2^-24 of accumulation noise.
  Measured on an MI355X (profiles/pair_modes_accuracy.txt), 60 launches: the seven op-level cases 3.28e-6 .. 4.48e-6 (worst: the
  single-pixel 3x3 case), the stem 3.67e-6, the 52 bottleneck convs 2.54e-6 .. 4.31e-6 (conv3 + residual 2.5e-6 .. 2.7e-6, conv1 /
  conv2 / downsample 3.3e-6 .. 4.3e-6).  That is the arithmetic's own distance: fp32 accumulation adds nothing visible up to K = 3 x 4608.
  Worst 4.481e-6 -> FP32X_REL_L2_BAR = 4 x 4.481e-6 = 1.79e-5 (tests/pair_reference.py); the smallest one-term defect is 54 bars away.

Exact checks need no tolerance: a zero tail plane adds exact zero products to the same accumulators in the same K order, so the pair
kernels must then reproduce `r50_op_conv2d` under the same tile template value for value -- any `x_wrap` or pair-offset indexing error
breaks that outright.
"""
import functools

import pytest
import torch

from tests import pair_reference as P
from tests.kernel_cases import _out_shape, _refused_ids, _split_case, _w2_case  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = -7.0
_MEASURED = []          # (what, rel-L2) of every fp32x launch checked in this session; printed by each fp32x test before it asserts


def _same_values(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool((a.float() == b.float()).all())


def _check_fp32x(y_pair_nhwc: torch.Tensor, ref_nchw_f64: torch.Tensor, what: str) -> float:
    """The fp32x bar stated above on one launch's (N,H,W,[head | tail]) output; prints the measured distance first."""
    hd, tl = P.unpair_nhwc(y_pair_nhwc.cpu())
    got = P.pair_value(hd, tl)
    ref = ref_nchw_f64.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    diff = (got - ref).abs()
    r = P.rel_l2(got, ref)
    _MEASURED.append((what, r))
    print(f"fp32x rel-L2 {what}: {r:.3e}  max|d| {float(diff.max()):.3e}")
    tol = ref.abs() * 2.0 ** -16 + 2.0 ** -16 * max(1.0, float(ref.abs().max()))
    bad = diff > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond tolerance, max diff {float(diff.max())}"
    assert r < P.FP32X_REL_L2_BAR, f"{what}: rel-L2 {r:.3e} (bar {P.FP32X_REL_L2_BAR:.1e})"
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# op level
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_w2_conv_every_tile_matches_oracle(lib_built, case):
    """Every generic, persistent and role-specialised tile id on a weight pair with a populated tail, guard band behind the output."""
    from implementation_phd_lab_vision_amd import ops
    from tests.test_kernels_gpu import _check_bf16, _tiles_for
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xd, wd, bd, rd, ref = _w2_case(case)
    assert float(wd[..., cin:].float().abs().max()) > 0.0
    n_, ho, wo, _ = _out_shape(case)
    numel = n * ho * wo * cout
    tiles = [t for t in _tiles_for(cout, k, pad) if t not in _refused_ids()]
    assert len(tiles) >= 6
    for tile in tiles:
        buf = torch.full((numel + 512 * cout,), GUARD, dtype=torch.bfloat16, device=DEV)
        y = ops.conv2d_w2(xd, wd, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile, out=buf)
        torch.cuda.synchronize()
        _check_bf16(y, ref, f"w2 conv tile={tile}")
        assert bool((buf[numel:] == GUARD).all()), f"w2 conv tile={tile}: wrote past the end of the output"


@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_w2_conv_refuses_tiles_that_do_not_read_the_pair(lib_built, case):
    """The shape-specialised kernels walk K on their own: their ids raise before any launch and leave y untouched."""
    from implementation_phd_lab_vision_amd import _lib, ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xd, wd, bd, rd, _ref = _w2_case(case)
    _n, ho, wo, _c = _out_shape(case)
    buf = torch.full((n * ho * wo * cout,), GUARD, dtype=torch.bfloat16, device=DEV)
    for tile in _refused_ids():
        with pytest.raises(_lib.R50Error, match="status -1"):
            ops.conv2d_w2(xd, wd, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile, out=buf)
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all()), "a refused call wrote to y"


@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_w2_conv_with_one_zero_plane_equals_the_plain_conv(lib_built, case):
    """[W | 0] and [0 | W] against `r50_op_conv2d` on W under the same explicit tile id, value for value."""
    from implementation_phd_lab_vision_amd import ops
    from tests.test_kernels_gpu import _tiles_for
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xd, wd, bd, rd, _ref = _w2_case(case)
    head = wd[..., :cin].contiguous()
    zero = torch.zeros_like(head)
    w_head_only = torch.cat([head, zero], dim=3).contiguous()
    w_tail_only = torch.cat([zero, head], dim=3).contiguous()
    for tile in [t for t in _tiles_for(cout, k, pad) if t not in _refused_ids() and t != ops.TILE_AUTO]:
        plain = ops.conv2d_bf16(xd, head, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile)
        a = ops.conv2d_w2(xd, w_head_only, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile)
        b = ops.conv2d_w2(xd, w_tail_only, bd, stride=stride, pad=pad, relu=relu, residual=rd, tile=tile)
        torch.cuda.synchronize()
        assert _same_values(a, plain), f"tile {tile}: [W | 0] differs from the plain conv in {int((a.float() != plain.float()).sum())} elements"
        assert _same_values(b, plain), f"tile {tile}: [0 | W] differs from the plain conv in {int((b.float() != plain.float()).sum())} elements"


@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_split_conv_matches_oracle(lib_built, case):
    """One fp32x launch (64 x 128 tile for cout 64, 128 x 128 otherwise) with every tail plane populated, guard band behind the output."""
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xd, wd, bd, rd, ref = _split_case(case)
    _n, ho, wo, _c = _out_shape(case)
    numel = n * ho * wo * 2 * cout
    buf = torch.full((numel + 512 * 2 * cout,), GUARD, dtype=torch.bfloat16, device=DEV)
    y = ops.conv2d_split(xd, wd, bd, stride=stride, pad=pad, relu=relu, residual_pair=rd, out=buf)
    torch.cuda.synchronize()
    assert bool((buf[numel:] == GUARD).all()), "split conv wrote past the end of the output"
    assert float(y[..., cout:].float().abs().max()) > 0.0, "no tail plane was written"
    _check_fp32x(y, ref, "op " + P.case_id(case))


def test_both_split_tile_shapes_occur():
    couts = {c[4] for c in P.PAIR_CASES}
    assert any(c % 128 for c in couts) and any(c % 128 == 0 for c in couts)


@pytest.mark.parametrize("case", P.PAIR_CASES, ids=P.case_id)
def test_split_conv_with_zero_tails_equals_the_plain_conv(lib_built, case):
    """x, w and residual with every tail zero: the head plane is `r50_op_conv2d`'s output under the tile id of the same template."""
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res = case
    xd, wd, bd, rd, _ref = _split_case(case)
    xh, wh = xd[..., :cin].contiguous(), wd[..., :cin].contiguous()
    rh = rd[..., :cout].contiguous() if has_res else None
    x0 = torch.cat([xh, torch.zeros_like(xh)], dim=3).contiguous()
    w0 = torch.cat([wh, wh, torch.zeros_like(wh)], dim=3).contiguous()
    r0 = torch.cat([rh, torch.zeros_like(rh)], dim=3).contiguous() if has_res else None
    y = ops.conv2d_split(x0, w0, bd, stride=stride, pad=pad, relu=relu, residual_pair=r0)
    plain = ops.conv2d_bf16(xh, wh, bd, stride=stride, pad=pad, relu=relu, residual=rh,
                            tile=ops.TILE_64x128 if cout % 128 else ops.TILE_128x128)
    torch.cuda.synchronize()
    got = y[..., :cout]
    assert _same_values(got, plain), f"{int((got.float() != plain.float()).sum())} of {plain.numel()} head values differ"


# ------------------------------------------------------------------------------------------------------------------------------
# network level
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net_inputs():
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    return synthetic_state_dict(0), synthetic_frames(3, seed=77)       # n = 3: M is ragged at every resolution


@pytest.fixture(scope="module")
def bb_fp32x(lib_built):
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    bb = ResNet50Backbone(state_dict=_net_inputs()[0], max_batch=64, precision="fp32x").to(DEV).eval()
    yield bb
    bb.close()


@pytest.fixture(scope="module")
def bb_w2(lib_built):
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    bb = ResNet50Backbone(state_dict=_net_inputs()[0], max_batch=64, precision="bf16w2").to(DEV).eval()
    yield bb
    bb.close()


def _blocks():
    for si, (blocks, stride) in enumerate(((3, 1), (4, 2), (6, 2), (3, 2)), start=1):
        for b in range(blocks):
            yield f"layer{si}.{b}", (stride if b == 0 else 1), b == 0


def test_w2_network_every_conv_on_shared_inputs(bb_w2):
    """All 52 bottleneck convs of the bf16w2 network, each fed the device's own input activation and residual."""
    from oracle.resnet50_oracle import conv_bias_act_emulated, folded
    from tests.test_kernels_gpu import _check_bf16
    sd, x = _net_inputs()
    xd = x.to(DEV)

    def nchw(t):
        return t.float().cpu().permute(0, 3, 1, 2).contiguous()

    def emu(xin, key, bn, s, pad, relu, res=None):
        w, bias = folded(sd, key, bn)
        return conv_bias_act_emulated(xin, w, bias, s, pad, relu, residual_bf=res, weight_terms=2)

    prev, n_checked = "pool", 0
    for p, s, first in _blocks():
        x_in = nchw(bb_w2.layer(xd, prev))
        t1, t2, out = bb_w2.layer(xd, p + ".t1"), bb_w2.layer(xd, p + ".t2"), bb_w2.layer(xd, p)
        _check_bf16(t1, emu(x_in, p + ".conv1", p + ".bn1", 1, 0, True), p + ".conv1")
        _check_bf16(t2, emu(nchw(t1), p + ".conv2", p + ".bn2", s, 1, True), p + ".conv2")
        idn = x_in
        if first:
            ds = bb_w2.layer(xd, p + ".ds")
            _check_bf16(ds, emu(x_in, p + ".downsample.0", p + ".downsample.1", s, 0, False), p + ".downsample")
            idn = nchw(ds)
            n_checked += 1
        _check_bf16(out, emu(nchw(t2), p + ".conv3", p + ".bn3", 1, 0, True, res=idn), p + ".conv3")
        n_checked += 3
        prev = p
    assert n_checked == 52


def test_fp32x_network_every_conv_on_shared_inputs(bb_fp32x):
    """The fp32x stem against the fp64 7x7 conv of the split frame and split stem weights, and all 52 bottleneck convs, each fed the
    device's own (head, tail) input activation and residual."""
    from oracle.resnet50_oracle import folded
    sd, x = _net_inputs()
    xd = x.to(DEV)

    def pair(name):
        t = bb_fp32x.layer(xd, name, pair=True)
        return t, P.unpair_nhwc(t.cpu())

    def ref(xin, key, bn, s, pad, relu, res=None):
        w, bias = folded(sd, key, bn)
        return P.fp32x_conv(xin, P.split_pair(w), bias, s, pad, relu, res)

    stem, _ = pair("stem")
    _check_fp32x(stem, ref(P.split_pair(x), "conv1", "bn1", 2, 3, True), "net conv1")
    prev, n_checked = "pool", 0
    for p, s, first in _blocks():
        _, x_in = pair(prev)
        (t1, t1p), (t2, t2p), (out, _) = pair(p + ".t1"), pair(p + ".t2"), pair(p)
        _check_fp32x(t1, ref(x_in, p + ".conv1", p + ".bn1", 1, 0, True), "net " + p + ".conv1")
        _check_fp32x(t2, ref(t1p, p + ".conv2", p + ".bn2", s, 1, True), "net " + p + ".conv2")
        idn = x_in
        if first:
            ds, idn = pair(p + ".ds")
            _check_fp32x(ds, ref(x_in, p + ".downsample.0", p + ".downsample.1", s, 0, False), "net " + p + ".downsample")
            n_checked += 1
        _check_fp32x(out, ref(t2p, p + ".conv3", p + ".bn3", 1, 0, True, res=idn), "net " + p + ".conv3")
        n_checked += 3
        prev = p
    assert n_checked == 52
    worst = max(_MEASURED, key=lambda v: v[1])
    print(f"fp32x worst rel-L2 over {len(_MEASURED)} launches: {worst[1]:.3e} ({worst[0]}); bar {P.FP32X_REL_L2_BAR:.1e}")


def test_fp32x_pools_are_exact(bb_fp32x):
    """maxpool3x3s2_split_kernel: the max of the pair sums (exact in fp32), re-split -- bit for bit.  avgpool_split_kernel: the 49
    pair sums added in order in fp32, times fp32(1/49) -- bit for bit."""
    import torch.nn.functional as F
    _sd, x = _net_inputs()
    xd = x.to(DEV)
    sh, st = P.unpair_nhwc(bb_fp32x.layer(xd, "stem", pair=True).cpu())
    want_h, want_t = P.split_pair(F.max_pool2d(sh.float() + st.float(), 3, 2, 1))
    got_h, got_t = P.unpair_nhwc(bb_fp32x.layer(xd, "pool", pair=True).cpu())
    assert float(want_t.float().abs().max()) > 0.0
    assert _same_values(got_h, want_h) and _same_values(got_t, want_t)

    last = bb_fp32x.layer(xd, "layer4.2", pair=True).cpu()             # (3,7,7,[head(2048) | tail(2048)])
    v = (last[..., :2048].float() + last[..., 2048:].float()).reshape(3, 49, 2048)
    s = torch.zeros((3, 2048), dtype=torch.float32)
    for r in range(49):
        s = s + v[:, r]
    want = s * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(49.0, dtype=torch.float32))
    got = bb_fp32x.features(xd).cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} features differ, max {float((got - want).abs().max())}"


# ------------------------------------------------------------------------------------------------------------------------------
# packed weights
# ------------------------------------------------------------------------------------------------------------------------------
def _stem_image(w_folded_oihw: torch.Tensor) -> torch.Tensor:
    """The stem kernel's weight image [kh][row][8][4] bf16: row rho holds channel perm(rho), slot j = kw + 1, c < 3; zero elsewhere."""
    img = torch.zeros((7, 64, 8, 4), dtype=torch.bfloat16)
    wq = w_folded_oihw.to(torch.bfloat16)
    for rho in range(64):
        o = (rho & ~31) | (rho & 3) | (((rho >> 4) & 1) << 2) | (((rho >> 2) & 3) << 3)
        img[:, rho, 1:8, :3] = wq[o].permute(1, 2, 0)            # (c,kh,kw) -> (kh,kw,c)
    return img.reshape(-1)


@pytest.mark.parametrize("mode", ["bf16w2", "fp32x"])
def test_packed_params_equal_the_restated_layouts(bb_w2, bb_fp32x, mode):
    """For every conv key: `packed_params` (sized by the mode; fp32x's two w_head copies verified equal by the hook) against
    `split_pair` of the oracle's BN fold, bit for bit, and the biases.  "conv1" is the stem image of bf16(w) in both modes; the fp32x
    stem's tail image is not served by `r50_get_packed`, so it is not checked here (the stem tap above depends on it)."""
    from implementation_phd_lab_vision_amd.weights import conv_specs
    from oracle.resnet50_oracle import folded
    bb = bb_w2 if mode == "bf16w2" else bb_fp32x
    sd, _x = _net_inputs()
    n_keys = 0
    for key, bn, cin, cout, k, _s, _p in conv_specs():
        w, b = folded(sd, key, bn)
        if key == "conv1":
            got_w, got_b = bb.packed_params(key)
            assert torch.equal(got_w.view(torch.int16), _stem_image(w).view(torch.int16)), "conv1: stem image differs"
        else:
            got_h, got_t, got_b = bb.packed_params(key)
            hd, tl = P.split_pair(w)
            assert tuple(got_h.shape) == (cout, k, k, cin) and tuple(got_t.shape) == (cout, k, k, cin)
            assert torch.equal(got_h.view(torch.int16), hd.permute(0, 2, 3, 1).contiguous().view(torch.int16)), f"{key}: w_head differs"
            assert torch.equal(got_t.view(torch.int16), tl.permute(0, 2, 3, 1).contiguous().view(torch.int16)), f"{key}: w_tail differs"
        assert torch.equal(got_b, b.to(torch.float32)), f"{key}: folded bias differs"
        n_keys += 1
    assert n_keys == 53


# ------------------------------------------------------------------------------------------------------------------------------
# batch composition
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16w2", "fp32x"])
def test_features_do_not_depend_on_batch_composition(bb_w2, bb_fp32x, mode):
    """A frame's features are the same bits alone, in a batch of 7 and in a batch of 49 -- where bf16w2 takes the large-batch tile
    choices (N >= 48: the tuned table, persistent and role-specialised tiles, all with the X chunk index wrapping)."""
    from implementation_phd_lab_vision_amd.weights import synthetic_frames
    bb = bb_w2 if mode == "bf16w2" else bb_fp32x
    x = synthetic_frames(49, seed=77).to(DEV)
    big = bb.features(x).clone()
    assert torch.isfinite(big).all()
    assert torch.equal(bb.features(x[3:10]), big[3:10]), "frames 3:10"
    for i in (0, 17, 48):
        assert torch.equal(bb.features(x[i:i + 1]), big[i:i + 1]), f"frame {i}"
