"""Whole-network parity on the MI355X through the reference-shaped boundary
(`backbone.to(device).eval(); backbone(x)`, src/preprocess_resnet_features.py:209,296).

Tolerances:
* every conv of the network on SHARED inputs (the device's own input activation fed to the oracle's
  fused conv): within one bf16 ulp + 2^-16 of scale per element (same bar as test_kernels_gpu.py).
* free-running, vs the bf16-emulating oracle (same rounding points, fp64 accumulation): two CPU
  emulations that differ ONLY in accumulating in fp32 instead of fp64 drift apart layer by layer
  (bf16 re-rounding amplifies accumulation-order noise: 1e-5 at the stem, 6e-3 element-wise at
  layer4, 1e-3 on the pooled features).  The device must stay within 3x that measured drift per
  named activation, and within 3e-3 per-frame rel-L2 on the final features.
* vs the fp32 reference restatement (the reference's CPU numerics): per-frame rel-L2 < 1e-2 — the
  cost of bf16 itself (the reference's own GPU path runs bf16 autocast, :290-294).
"""
import pytest
import torch
from tests.network_oracles import (  # noqa: F401
    check_features_bf16, check_features_bf16w2, check_features_fp16, check_features_fp32x, check_features_fp8, oracle_bf16, oracle_bf16w2, oracle_fp16, oracle_fp32x, oracle_fp8)

pytestmark = pytest.mark.gpu

TAPS = ["stem", "pool", "layer1.0.t1", "layer1.0.t2", "layer1.0.ds", "layer1.0", "layer1.2", "layer2.0.t2",
        "layer2.0.ds", "layer2.0", "layer2.3", "layer3.0", "layer3.5", "layer4.0.t2", "layer4.0", "layer4.2"]


@pytest.fixture(scope="module")
def setup(lib_built):
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    sd, x, taps, drift, feats_emu, feats_ref = oracle_bf16()
    bb = ResNet50Backbone(state_dict=sd, max_batch=8).to("cuda:0").eval()
    return bb, x, (taps, drift, sd), feats_emu, feats_ref


def test_named_activations_match_emulated_oracle(setup):
    from oracle.resnet50_oracle import rel_l2
    bb, x, (taps, drift, _sd), _, _ = setup
    xd = x.to("cuda:0")
    for name in TAPS:
        got = bb.layer(xd, name).float().cpu().permute(0, 3, 1, 2)
        ref = taps[name].float()
        assert got.shape == ref.shape, name
        r = rel_l2(got, ref)
        assert r < max(1e-4, 3.0 * drift[name]), f"{name}: rel-L2 {r} (emulation drift {drift[name]})"


@pytest.mark.parametrize("ds_cat", [1, 0], ids=["ds_in_conv3", "ds_separate"])
def test_every_conv_on_shared_inputs(setup, ds_cat):
    """All 52 bottleneck convs, each checked in isolation: the oracle's fused conv is fed the DEVICE's
    input activation (and residual), so no drift accumulates and the 1-ulp bar applies.  ds_cat = 1 (the default): in
    layer2.0 / 3.0 / 4.0 conv3 and the downsample conv are one accumulation over two K sources, checked as such (the
    downsample conv alone is still checked through its tap); ds_cat = 0: the two launches."""
    from oracle.resnet50_oracle import conv_bias_act_emulated, conv_cat_emulated, folded
    from tests.test_kernels_gpu import _check_bf16
    bb, x, (_taps, _drift, sd), _, _ = setup
    xd = x[:2].to("cuda:0")

    def dev(name):
        return bb.layer(xd, name)                       # bf16 NHWC on the GPU

    def nchw(t):
        return t.float().cpu().permute(0, 3, 1, 2).contiguous()

    assert bb.get_option("fuse_ds_cat") == 1
    bb.set_option("fuse_ds_cat", ds_cat)
    try:
        prev = "pool"
        n_checked = 0
        for si, (blocks, stride) in enumerate(((3, 1), (4, 2), (6, 2), (3, 2)), start=1):
            for b in range(blocks):
                p = f"layer{si}.{b}"
                s = stride if b == 0 else 1
                x_in = nchw(dev(prev))
                t1, t2, out = dev(p + ".t1"), dev(p + ".t2"), dev(p)
                w, bias = folded(sd, p + ".conv1", p + ".bn1")
                _check_bf16(t1, conv_bias_act_emulated(x_in, w, bias, 1, 0, True), p + ".conv1")
                w, bias = folded(sd, p + ".conv2", p + ".bn2")
                _check_bf16(t2, conv_bias_act_emulated(nchw(t1), w, bias, s, 1, True), p + ".conv2")
                if b == 0:
                    ds = dev(p + ".ds")
                    wd, bd = folded(sd, p + ".downsample.0", p + ".downsample.1")
                    _check_bf16(ds, conv_bias_act_emulated(x_in, wd, bd, s, 0, False), p + ".downsample")
                    idn = nchw(ds)
                    n_checked += 1
                else:
                    idn = x_in
                w, bias = folded(sd, p + ".conv3", p + ".bn3")
                if b == 0 and si >= 2 and ds_cat:
                    _check_bf16(out, conv_cat_emulated(nchw(t2), w, bias, x_in, wd, bd, s), p + ".conv3+downsample")
                else:
                    _check_bf16(out, conv_bias_act_emulated(nchw(t2), w, bias, 1, 0, True, residual_bf=idn), p + ".conv3")
                n_checked += 3
                prev = p
        assert n_checked == 52
    finally:
        bb.set_option("fuse_ds_cat", 1)


def test_features_match_oracles(setup):
    bb, x, _t, feats_emu, feats_ref = setup
    check_features_bf16(bb, x, feats_emu, feats_ref)


def test_batch_split_invariance(setup):
    """Frames are independent: chunking by max_batch / micro_batch must not change a single bit."""
    bb, x, _, _, _ = setup
    from implementation_phd_lab_vision_amd.weights import synthetic_frames
    xs = synthetic_frames(11, seed=5).to("cuda:0")       # 11 > max_batch = 8: two chunks
    full = bb.features(xs).clone()
    bb.set_option("micro_batch", 3)
    part = bb.features(xs).clone()
    bb.set_option("micro_batch", 0)
    one = torch.cat([bb.features(xs[i:i + 1]) for i in range(11)])
    assert torch.equal(full, part)
    assert torch.equal(full, one)


def test_empty_and_errors(setup):
    from implementation_phd_lab_vision_amd import _lib
    bb, *_ = setup
    out = bb.features(torch.empty((0, 3, 224, 224), device="cuda:0"))
    assert tuple(out.shape) == (0, 2048)
    with pytest.raises(ValueError):
        bb.features(torch.zeros((1, 3, 32, 32), device="cuda:0"))
    with pytest.raises(_lib.R50Error):
        bb.layer(torch.zeros((1, 3, 224, 224), device="cuda:0"), "no_such_layer")


# ---------------------------------------------------------------------------------------------------
# fp32x precision: fp32-class accuracy on the bf16 matrix cores.  This is the mode that meets the
# north-star bar "features within 1e-3 rel of the reference" against the fp32 reference view
# (= the reference's CPU numerics, autocast disabled, src/preprocess_resnet_features.py:239-241).
# Tolerance: per-frame rel-L2 < 1e-3 on features, rel-L2 < 1e-3 on every named activation (measured ~1e-5).
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup_fp32x(lib_built):
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    sd, x, taps, feats_ref = oracle_fp32x()
    bb = ResNet50Backbone(state_dict=sd, max_batch=4, precision="fp32x").to("cuda:0").eval()
    return bb, x, taps, feats_ref


def test_fp32x_features_within_1e3_of_fp32_reference(setup_fp32x):
    bb, x, _taps, feats_ref = setup_fp32x
    check_features_fp32x(bb, x, feats_ref)


def test_fp32x_named_activations(setup_fp32x):
    from oracle.resnet50_oracle import rel_l2
    bb, x, taps, _ = setup_fp32x
    xd = x.to("cuda:0")
    for name in ["stem", "pool", "layer1.0", "layer1.2", "layer2.0", "layer2.3", "layer3.5", "layer4.0", "layer4.2"]:
        got = bb.layer(xd, name).cpu().permute(0, 3, 1, 2)
        ref = taps[name]
        assert got.shape == ref.shape, name
        r = rel_l2(got, ref)
        assert r < 1e-3, f"{name}: rel-L2 {r}"


def test_fused_stem_equals_unfused(setup):
    """conv1+bn1+relu+maxpool fused in one kernel must equal the three-kernel path bit for bit (same K order,
    same roundings), for every frame position incl. the image borders."""
    from implementation_phd_lab_vision_amd import ops
    bb, x, *_ = setup
    xd = x.to("cuda:0")
    assert bb.get_option("fused_stem") == 1
    fused = bb.layer(xd, "pool")                       # fused kernel (the 'stem' tap alone forces the unfused path)
    unfused = ops.maxpool_bf16(bb.layer(xd, "stem").contiguous())
    assert torch.equal(fused, unfused)
    # every strip length of the strip kernel (workgroup = G consecutive pooled-row pairs of an image, shared rows kept in LDS rings): the same bits
    try:
        for g in (1, 2, 4, 7, 14, 28):
            bb.set_option("stem_strip", g)
            assert torch.equal(bb.layer(xd, "pool"), unfused), g
    finally:
        bb.set_option("stem_strip", 0)
    # layer1.0.conv1 riding along in the strip kernel: the same bits as its own igemm launch, for every strip length
    assert bb.get_option("fuse_stem_c1") == 1
    bb.set_option("fuse_stem_c1", 0)
    t1_plain = bb.layer(xd, "layer1.0.t1").clone()
    f_plain = bb.features(xd).clone()
    bb.set_option("fuse_stem_c1", 1)
    try:
        for g in (0, 1, 2, 4, 7, 14, 28):
            bb.set_option("stem_strip", g)
            assert torch.equal(bb.layer(xd, "layer1.0.t1"), t1_plain), g
            assert torch.equal(bb.layer(xd, "pool"), unfused), g
            assert torch.equal(bb.features(xd), f_plain), g
    finally:
        bb.set_option("stem_strip", 0)
    bb.set_option("fused_stem", 0)
    try:
        assert torch.equal(bb.layer(xd, "pool"), unfused)
        f0 = bb.features(xd).clone()
    finally:
        bb.set_option("fused_stem", 1)
    assert torch.equal(bb.features(xd), f0)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_default_fusions_give_the_bits_of_plain_launches(lib_built, precision):
    """With the bottleneck bodies of layer1.1 / layer2.1-.3 in one launch each (bneck_block1 / bneck_block2), the layer1 tails and the
    chained layer3 tails, EVERY fusion on the default path reproduces the summation order of the launches it replaces: the features
    are the same bits as with one igemm launch per conv (`fuse_tail` = 0 turns all of them off).  Also with layer1.2 as two launches."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_frames
    x = synthetic_frames(5, seed=77).to("cuda:0")
    bb = ResNet50Backbone(seed=0, max_batch=5, precision=precision).to("cuda:0").eval()
    try:
        assert bb.get_option("fuse_block1") == 3 and bb.get_option("fuse_block2") == 1      # round 3: layer1.2 and layer1.0 are one launch each by default too
        assert bb.get_option("fuse_cat_chain") == 1
        f_default = bb.features(x).clone()
        bb.set_option("fuse_block1", 1)
        f_b12 = bb.features(x).clone()                                                   # the round-2 default (layer1.2 as conv2 + fused tail)
        bb.set_option("fuse_block1", 0); bb.set_option("fuse_block2", 0)
        f_tails = bb.features(x).clone()          # layer2 through bneck_tail2_kernel: its next conv1 sums K in eight slices
        bb.set_option("fuse_tail", 0)
        f_plain = bb.features(x).clone()
    finally:
        bb.close()
    assert torch.isfinite(f_plain).all()
    assert torch.equal(f_default, f_plain), f"max |diff| {float((f_default - f_plain).abs().max())}"
    assert torch.equal(f_b12, f_plain)
    assert float((f_tails - f_plain).abs().max()) < 0.05 * float(f_plain.abs().max())      # (bneck_tail2: within rounding, not bit for bit)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 5, 37])
def test_sub_sampled_layer1_output_gives_the_same_features(lib_built, precision, n):
    """layer1.2 stores only the even rows / columns of its block output (option "sub_out", the default): its two readers are layer2.0.conv1
    (computed in the same launch) and layer2.0's stride-2 downsample conv (inside bneck_catchain_kernel, which then reads the compact
    tensor).  The features must be the bits of the run that writes the full tensor; and with the chained transition tail turned off
    the full tensor must be written again (the compact form has no other reader)."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_frames
    x = synthetic_frames(n, seed=91).to("cuda:0")
    bb = ResNet50Backbone(seed=0, max_batch=n, precision=precision).to("cuda:0").eval()
    try:
        assert bb.get_option("sub_out") == 1
        f_sub = bb.features(x).clone()
        bb.set_option("sub_out", 0)
        f_full = bb.features(x).clone()
        bb.set_option("sub_out", 1)
        bb.set_option("fuse_cat_chain", 0)            # layer2.0 through the two-source igemm launch: needs (and gets) the full tensor
        f_nochain = bb.features(x).clone()
        bb.set_option("fuse_cat_chain", 1)
        tap = bb.layer(x, "layer1.2").clone()         # debug taps see full tensors
        f_again = bb.features(x).clone()
    finally:
        bb.close()
    assert torch.isfinite(f_full).all()
    assert torch.equal(f_sub, f_full), f"max |diff| {float((f_sub - f_full).abs().max())}"
    assert torch.equal(f_nochain, f_full) and torch.equal(f_again, f_full)
    assert tuple(tap.shape) == (n, 56, 56, 256)


def test_fused_bottleneck_tail_equals_unfused(setup):
    """conv3 + identity + ReLU + the next block's conv1 in one kernel.  layer1 (pixels split over the waves): bit
    for bit what the two igemm launches give.  layer2 (channels split over the waves, second conv summed in eight
    K slices): block outputs downstream of a fused conv1 may flip a bf16 ulp, so those are held to a tight rel-L2."""
    from oracle.resnet50_oracle import rel_l2
    bb, x, *_ = setup
    xd = x.to("cuda:0")
    assert bb.get_option("fuse_tail") == 1
    exact = ["layer1.0.ds", "layer1.0", "layer1.1.t1", "layer1.1", "layer1.2.t1", "layer1.2", "layer2.0.t1", "layer2.0.ds",
             "layer2.0"]
    close = ["layer2.1.t1", "layer2.1", "layer2.2.t1", "layer2.3.t1", "layer2.3", "layer3.0"]
    fused = {k: bb.layer(xd, k).clone() for k in exact + close}
    f1 = bb.features(xd).clone()
    bb.set_option("fuse_tail", 0)
    try:
        for k in exact:
            assert torch.equal(bb.layer(xd, k), fused[k]), k
        for k in close:
            r = rel_l2(bb.layer(xd, k).float(), fused[k].float())
            assert r < 2e-3, f"{k}: rel-L2 {r} between fused and unfused"
        r = rel_l2(bb.features(xd), f1)
        assert r < 2e-3, f"features: rel-L2 {r} between fused and unfused"
    finally:
        bb.set_option("fuse_tail", 1)


@pytest.mark.parametrize("precision", ["bf16", "fp32x"])
def test_uint8_frames_equal_host_normalised_frames(lib_built, precision):
    """Boundary one step upstream: uint8 resized crops in, normalisation inside the stem kernel.
    Must be bit-identical to feeding the host-normalised fp32 frames (dataset.py:148-149,242-245: /255, -mean, /std)."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    g = torch.Generator().manual_seed(21)
    u8 = torch.randint(0, 256, (5, 3, 224, 224), generator=g, dtype=torch.uint8)
    u8[0] = 0
    u8[1] = 255
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    x = (u8.to(torch.float32) / 255.0 - mean) / std                 # the reference's host path
    bb = ResNet50Backbone(seed=0, max_batch=8, precision=precision).to("cuda:0").eval()
    a = bb.features_u8(u8.to("cuda:0")).cpu()
    b = bb.features(x.to("cuda:0")).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_features_do_not_depend_on_batch_composition(lib_built):
    """A frame's features are a function of that frame alone: the same bits whether it is run alone, in a batch of 7, or
    in a batch of 49 (where the tuned large-batch tile table, the persistent kernels and ragged last tiles are in play).
    This is what lets the CLI take the temporal-reverse variant's features from variant 0 (extract_features)."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_frames
    bb = ResNet50Backbone(seed=0, max_batch=64).to("cuda:0").eval()
    x = synthetic_frames(49, seed=77).to("cuda:0")
    big = bb.features(x).clone()
    assert torch.isfinite(big).all()
    mid = bb.features(x[3:10]).clone()
    assert torch.equal(mid, big[3:10])
    for i in (0, 17, 48):
        assert torch.equal(bb.features(x[i:i + 1]), big[i:i + 1]), f"frame {i}"
    assert torch.equal(bb.features(x.flip(0)), big.flip(0))


def test_bf16w2_precision_meets_1e3_of_the_fp32_reference(lib_built):
    """bf16w2: bf16 activations, every bottleneck conv weight a bf16 (head, tail) pair, two MFMA products per conv.  The
    bf16 error of this network is weight-rounding dominated (oracle: fp32 weights + bf16 activations 8e-4, bf16 weights +
    fp32 activations 2.3e-3), so this mode lands within north_star's 1e-3 of the fp32/fp64 reference view, and tracks
    its own emulation (same rounding points) like the bf16 mode does."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from oracle import resnet50_oracle as O
    sd, x, ref, emu, taps = oracle_bf16w2()
    bb = ResNet50Backbone(state_dict=sd, max_batch=4, precision="bf16w2").to("cuda:0").eval()
    check_features_bf16w2(bb, x, ref, emu)
    # and a mid-network tap against the emulation's tap
    t = bb.layer(x.to("cuda:0"), "layer2.1").float().cpu().permute(0, 3, 1, 2)
    assert O.rel_l2(t, taps["layer2.1"]) < 2e-3


def test_fp16_precision(lib_built):
    """fp16 mode: the bf16 path with IEEE half as the 16-bit format (same kernels, MFMA f16).  11 significand bits: the
    features land ~3e-4 from the fp32/fp64 reference view -- inside north_star's 1e-3 at full speed -- and track the
    emulation with the same rounding points, taps included (fused stem, resident-weights 3x3, fused tails, plain convs)."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from oracle import resnet50_oracle as O
    sd, x, ref, emu, taps = oracle_fp16()
    bb = ResNet50Backbone(state_dict=sd, max_batch=4, precision="fp16").to("cuda:0").eval()
    xd = x.to("cuda:0")
    check_features_fp16(bb, x, ref, emu)
    for name in ["pool", "layer1.0", "layer1.1.t1", "layer1.1.t2", "layer1.2", "layer2.0", "layer2.1.t1", "layer2.3", "layer3.5", "layer4.2"]:
        t = bb.layer(xd, name)
        assert t.dtype == torch.float16
        r = O.rel_l2(t.float().cpu().permute(0, 3, 1, 2), taps[name])
        assert r < 1e-3, f"{name}: rel-L2 {r} vs the fp16 emulation"
    # uint8 boundary in fp16 mode: same bits as host-normalised frames
    g = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (2, 3, 224, 224), generator=g, dtype=torch.uint8)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    xn = (u8.to(torch.float32) / 255.0 - mean) / std
    assert torch.equal(bb.features_u8(u8.to("cuda:0")).cpu(), bb.features(xn.to("cuda:0")).cpu())


# ---- fp8 network mode (R50_PREC_FP8, BASELINE configs[4]) ---------------------------------------------------------------
@pytest.fixture(scope="module")
def setup_fp8(lib_built):
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    sd = synthetic_state_dict(0)
    bb = ResNet50Backbone(state_dict=sd, max_batch=8, precision="fp8").to("cuda:0").eval()      # calibrates on 8 synthetic frames
    return bb, sd, synthetic_frames(4, seed=1234)


def test_fp8_weights_are_torchs_e4m3_of_the_folded_weights(setup_fp8):
    """The host-side fp32 -> e4m3 conversion of r50_load_weights (round to nearest even, saturating) against torch's."""
    import ctypes as C
    from implementation_phd_lab_vision_amd import _lib
    from oracle import resnet50_oracle as O
    bb, sd, _ = setup_fp8
    lib = _lib.load_library()
    for key, bn in (("layer2.0.conv1", "layer2.0.bn1"), ("layer3.4.conv2", "layer3.4.bn2"), ("layer4.0.downsample.0", "layer4.0.downsample.1")):
        w, _b = O.folded(sd, key, bn)
        wq, _scale = O.fp8_weight(w)
        want = wq.permute(0, 2, 3, 1).contiguous().to(torch.float8_e4m3fn).view(torch.uint8).flatten()
        got = torch.empty(want.numel(), dtype=torch.uint8)
        n = C.c_int64()
        _lib.check(lib.r50_get_packed(bb._handle, key.encode(), 0, got.data_ptr(), got.numel(), C.byref(n)), bb._handle, "r50_get_packed")
        assert n.value == want.numel()
        # +0 and -0 both occur for tiny weights of either sign; compare values
        assert torch.equal(got.view(torch.float8_e4m3fn).float(), want.view(torch.float8_e4m3fn).float()), key


def test_fp8_features_match_the_fp8_emulation(setup_fp8):
    from oracle import resnet50_oracle as O
    bb, sd, x = setup_fp8
    _sd, _x, emu, ref = oracle_fp8(tuple(bb.fp8_scales))
    f = check_features_fp8(bb, x, emu, ref)
    # conv3 and the downsample conv as two launches (downsample tensor formed and rounded): its own emulation
    bb.set_option("fuse_ds_cat", 0)
    try:
        f2 = bb(x.to("cuda:0")).flatten(1).cpu()
    finally:
        bb.set_option("fuse_ds_cat", 1)
    emu2 = O.forward_fp8_emulated(sd, x, bb.fp8_scales, fused_ds=False)
    assert float(O.per_row_rel_l2(f2, emu2).max()) < 2.5e-2
    assert not torch.equal(f2, f)


def test_fp8_mode_is_batch_independent_and_needs_scales(setup_fp8):
    from implementation_phd_lab_vision_amd import _lib
    from implementation_phd_lab_vision_amd.weights import synthetic_frames
    bb, sd, _ = setup_fp8
    xs = synthetic_frames(7, seed=9).to("cuda:0")
    full = bb.features(xs).clone()
    one = torch.cat([bb.features(xs[i:i + 1]) for i in range(7)])
    assert torch.equal(full, one)
    with pytest.raises(_lib.R50Error):
        bb.layer(xs, "layer3.0")                      # e4m3 tensors beyond layer1: no 16-bit tap
    assert bb.layer(xs, "layer1.2").shape == (7, 56, 56, 256)
    with pytest.raises(ValueError):
        bb.set_fp8_scales([1.0] * 5)


def test_layer3_chained_tail_is_bit_identical_to_separate_launches(setup):
    """layer3.1-.4: conv3 + identity + ReLU chained with the next block's conv1 in one launch (bneck_tail3p_kernel) -- same features,
    bit for bit, as the two igemm launches per block it replaces; and the taps it produces match too."""
    bb, x, *_ = setup
    xd = x.to("cuda:0")
    assert bb.get_option("fuse_tail3") == 1
    fused = bb.features(xd).clone()
    taps_f = {n: bb.layer(xd, n).clone() for n in ("layer3.1", "layer3.2.t1", "layer3.4", "layer3.5.t1", "layer3.5")}
    bb.set_option("fuse_tail3", 0)
    try:
        plain = bb.features(xd).clone()
        for n, t in taps_f.items():
            assert torch.equal(t, bb.layer(xd, n)), n
    finally:
        bb.set_option("fuse_tail3", 1)
    assert torch.equal(fused, plain)


def test_fp8_handover_in_the_conv_epilogue_is_bit_identical(setup_fp8):
    """fp8 mode: layer1's 16-bit output is quantised to e4m3 inside layer1.2.conv3's epilogue (same rounding sequence: 16-bit result,
    then x 1/scale, then e4m3) -- same features as with the separate quantisation pass, at batch sizes on both sides of the tile rule."""
    from implementation_phd_lab_vision_amd.weights import synthetic_frames
    bb, _sd, _x = setup_fp8
    assert bb.get_option("fuse_fp8_handover") == 1
    for n in (3, 8):
        xs = synthetic_frames(n, seed=40 + n).to("cuda:0")
        fused = bb.features(xs).clone()
        bb.set_option("fuse_fp8_handover", 0)
        try:
            plain = bb.features(xs).clone()
        finally:
            bb.set_option("fuse_fp8_handover", 1)
        assert torch.equal(fused, plain), n


def test_backbone_lanes_give_the_bits_of_one_backbone():
    """backbone.BackboneLanes: two backbone copies on their own streams, batches dealt round robin -- the features of every batch are the
    bits of a single backbone's, whatever lane it ran on and whatever else was in flight; the one-batch surface (``features``,
    ``__call__``) is ordered with the current stream like ``ResNet50Backbone``'s."""
    import torch
    from implementation_phd_lab_vision_amd.backbone import BackboneLanes, ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    dev = torch.device("cuda", 0)
    sd = synthetic_state_dict(0)
    one = ResNet50Backbone(state_dict=sd, max_batch=24).to(dev).eval()
    two = BackboneLanes(lanes=2, state_dict=sd, max_batch=24).to(dev).eval()
    try:
        xs = [synthetic_frames(n, seed=900 + n).to(dev) for n in (24, 5, 17, 24, 9)]
        refs = [one.features(x).clone() for x in xs]
        torch.cuda.synchronize(dev)
        # whether the two streams share a hardware queue is the runtime's business (DESIGN: one stream pair in eight): a diagnostic, never a failure
        print("lanes' streams overlap:", BackboneLanes._overlap(two._streams[0], two._streams[1], dev))
        assert two.tune(xs[1]) == 1.0 and "too few" in two.tune_mode and two.active_lanes == 2        # 5 frames: nothing to measure, nothing changed
        # workload check of the lanes' streams (may swap them): ratios are informational, results unaffected; drop_below = 0: keep both lanes
        gain = two.tune(xs[0], steps=3, tries=2, drop_below=0.0, min_frames=1)
        assert 0.2 < gain < 5.0 and len(two.tune_log) >= 1 and two.active_lanes == 2
        tickets = [two.submit(x) for x in xs]              # five batches queued before the first result is looked at
        assert [t.lane for t in tickets] == [0, 1, 0, 1, 0]
        for t, r in zip(tickets, refs):
            assert torch.equal(t.wait(), r)
        # a workload the lanes do not pay for (tune measured < 1): submit falls back to lane 0, same bits
        two._active, two.tune_mode = BackboneLanes.lane_plan([0.97], 2)
        assert two.active_lanes == 1 and "fallback" in two.tune_mode
        tickets = [two.submit(x) for x in xs[:3]]
        assert [t.lane for t in tickets] == [0, 0, 0]
        for t, r in zip(tickets, refs):
            assert torch.equal(t.wait(), r)
        # out = None with a caller's event: the lane also waits for the allocation point of `out` on the current stream
        ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream(dev))
        junk = [torch.zeros(5, 2048, device=dev) + k for k in range(8)]; del junk
        assert torch.equal(two.submit(xs[1], after=ev).wait(), refs[1])
        two._active, two.tune_mode = BackboneLanes.lane_plan([1.05], 2)
        assert two.active_lanes == 2
        # producer on the current stream, consumer on the current stream: no explicit events needed with features()
        x = xs[2] * 1.0
        y = two.features(x)
        assert torch.equal(y, refs[2])
        assert two(xs[1]).shape == (5, 2048, 1, 1)
        two.set_option("tail3_bp", 98)                     # options go to every lane
        assert two.lane0.get_option("tail3_bp") == 98
        two.set_option("tail3_bp", 0)
        # the lanes read ONE copy of the weights (r50_share_weights): lane 1 survives lane 0's handle, and a third backbone can join
        # neither the owner (it has a sharer) nor the sharer may take new weights: their buffers are read by the other lane's launches
        for bb in two._bbs:
            with pytest.raises(Exception, match="shares its weight buffers"):
                bb._load_weights()
        w0, _ = two._bbs[0].packed_params("layer3.1.conv2")
        w1, _ = two._bbs[1].packed_params("layer3.1.conv2")
        assert torch.equal(w0, w1)
        two._bbs[0].close()
        assert torch.equal(two._bbs[1].features(xs[1]), refs[1])
        with pytest.raises(Exception):
            ResNet50Backbone(state_dict=sd, max_batch=8, precision="fp16").to(dev, share_from=two._bbs[1])      # other precision
    finally:
        one.close()
        two.close()


def test_layer2_0_chained_transition_tail_is_bit_identical(setup):
    """layer2.0: conv3 + downsample + ReLU (one two-source conv) chained with layer2.1.conv1 in one launch (bneck_catchain_kernel, option
    fuse_cat_chain, default on) -- same features bit for bit as the two igemm launches it replaces; the block output tap too."""
    bb, x, *_ = setup
    xd = x.to("cuda:0")
    assert bb.get_option("fuse_cat_chain") == 1
    fused = bb.features(xd).clone()
    bb.set_option("fuse_cat_chain", 0)
    try:
        plain = bb.features(xd).clone()
    finally:
        bb.set_option("fuse_cat_chain", 1)
    assert torch.equal(fused, plain)


def test_layer1_0_body_in_one_launch_is_bit_identical(setup):
    """fuse_block1 = 3 (default): layer1.0 from its conv2 on is one launch of the bottleneck-body kernel with the downsample conv as the identity;
    same features bit for bit as with conv3x3_c64 + the fused downsample tail (fuse_block1 = 2) and as layer by layer (0)."""
    bb, x, *_ = setup
    xd = x.to("cuda:0")
    assert bb.get_option("fuse_block1") == 3
    ref = bb.features(xd).clone()
    try:
        for v in (2, 0):
            bb.set_option("fuse_block1", v)
            assert torch.equal(bb.features(xd), ref), v
    finally:
        bb.set_option("fuse_block1", 3)
