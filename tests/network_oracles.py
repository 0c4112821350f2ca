"""The CPU oracles of each precision's network fixture and the features check that goes with each: tests/test_network_gpu.py's, which
the network rows of tests/rows/r50.py and tests/test_work_distribution_gpu.py hold their own handles to as well."""
import functools

import torch


# The CPU oracles of each precision's fixture: computed once per session and shared (read-only) by every test module that needs them.
@functools.lru_cache(maxsize=None)
def oracle_bf16():
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from oracle import resnet50_oracle as O
    sd = synthetic_state_dict(0)
    x = synthetic_frames(4, seed=1234)
    taps = {}
    feats_emu = O.forward_bf16_emulated(sd, x, taps=taps, fused_ds=True)
    taps32 = {}
    O.forward_bf16_emulated(sd, x, taps=taps32, acc_dtype=torch.float32, fused_ds=True)
    drift = {k: O.rel_l2(taps32[k], taps[k]) for k in taps}
    feats_ref = O.forward_reference(sd, x).flatten(1)
    return sd, x, taps, drift, feats_emu, feats_ref


def check_features_bf16(bb, x, feats_emu, feats_ref):
    from oracle.resnet50_oracle import per_row_rel_l2
    out = bb(x.to("cuda:0"))
    assert tuple(out.shape) == (4, 2048, 1, 1) and out.dtype == torch.float32 and out.is_cuda, f"{tuple(out.shape)} {out.dtype} on {out.device}"
    f = out.flatten(1).cpu()
    assert torch.isfinite(f).all(), f"{int((~torch.isfinite(f)).sum())} of {f.numel()} features are not finite"
    r_emu = per_row_rel_l2(f, feats_emu)
    r_ref = per_row_rel_l2(f, feats_ref)
    assert float(r_emu.max()) < 3e-3, r_emu
    assert float(r_ref.max()) < 1e-2, r_ref


@functools.lru_cache(maxsize=None)
def oracle_fp32x():
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from oracle import resnet50_oracle as O
    sd = synthetic_state_dict(0)
    x = synthetic_frames(3, seed=77)
    taps = {}
    feats_ref = O.forward_reference(sd, x, dtype=torch.float64, taps=taps).flatten(1)
    return sd, x, taps, feats_ref


def check_features_fp32x(bb, x, feats_ref):
    from oracle.resnet50_oracle import per_row_rel_l2
    f = bb(x.to("cuda:0")).flatten(1).cpu()
    assert torch.isfinite(f).all(), f"{int((~torch.isfinite(f)).sum())} of {f.numel()} features are not finite"
    r = per_row_rel_l2(f, feats_ref)
    assert float(r.max()) < 1e-3, r


@functools.lru_cache(maxsize=None)
def oracle_bf16w2():
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from oracle import resnet50_oracle as O
    sd = synthetic_state_dict(0)
    x = synthetic_frames(3, seed=11)
    ref = O.forward_reference(sd, x, dtype=torch.float64).float()
    taps = {}
    emu = O.forward_bf16_emulated(sd, x, taps=taps, weight_terms=2)
    return sd, x, ref, emu, taps


def check_features_bf16w2(bb, x, ref, emu):
    from oracle import resnet50_oracle as O
    got = bb.features(x.to("cuda:0")).cpu()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} of {got.numel()} features are not finite"
    r_ref = O.per_row_rel_l2(got, ref)
    r_emu = O.per_row_rel_l2(got, emu)
    assert float(r_ref.max()) < 1e-3, f"bf16w2 vs fp64 reference: {r_ref.tolist()}"
    assert float(r_emu.max()) < 1e-3, f"bf16w2 vs its emulation: {r_emu.tolist()}"


@functools.lru_cache(maxsize=None)
def oracle_fp16():
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from oracle import resnet50_oracle as O
    sd = synthetic_state_dict(0)
    x = synthetic_frames(3, seed=12)
    ref = O.forward_reference(sd, x, dtype=torch.float64).float()
    taps = {}
    emu = O.forward_bf16_emulated(sd, x, taps=taps, fmt="fp16", fused_ds=True)
    return sd, x, ref, emu, taps


def check_features_fp16(bb, x, ref, emu):
    from oracle import resnet50_oracle as O
    got = bb.features(x.to("cuda:0")).cpu()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} of {got.numel()} features are not finite"
    r_ref, r_emu = O.per_row_rel_l2(got, ref), O.per_row_rel_l2(got, emu)
    assert float(r_ref.max()) < 1e-3, f"fp16 vs fp64 reference: {r_ref.tolist()}"
    assert float(r_ref.max()) < 5e-4, f"fp16 should sit well inside the tolerance: {r_ref.tolist()}"
    assert float(r_emu.max()) < 3e-4, f"fp16 vs its emulation: {r_emu.tolist()}"


@functools.lru_cache(maxsize=None)
def oracle_fp8(scales):
    """fp8 emulation (for one tuple of activation scales) and fp32 reference features of the fp8 fixture's frames."""
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from oracle import resnet50_oracle as O
    sd = synthetic_state_dict(0)
    x = synthetic_frames(4, seed=1234)
    return sd, x, O.forward_fp8_emulated(sd, x, list(scales)), O.forward_reference(sd, x).flatten(1)


def check_features_fp8(bb, x, emu, ref):
    from oracle import resnet50_oracle as O
    assert len(bb.fp8_scales) == 43 and all(s > 0 for s in bb.fp8_scales), f"{len(bb.fp8_scales)} fp8 scales: {bb.fp8_scales}"
    f = bb(x.to("cuda:0")).flatten(1).cpu()
    assert tuple(f.shape) == (4, 2048) and torch.isfinite(f).all(), f"{tuple(f.shape)}, {int((~torch.isfinite(f)).sum())} features not finite"
    r_emu = O.per_row_rel_l2(f, emu)
    r_ref = O.per_row_rel_l2(f, ref)
    e_ref = O.per_row_rel_l2(emu, ref)
    # one e4m3 step is 6 %: a sum that lands on the other side of a rounding tie moves an activation by that much, and 39 chained
    # convs spread such flips; the device must stay as close to the emulation as the emulation's own error scale allows
    assert float(r_emu.max()) < 2.5e-2, r_emu
    assert float(r_ref.max()) < 1.5 * float(e_ref.max()) + 1e-2, (r_ref, e_ref)
    return f


def _oracle_bar(precision, bb):
    """That precision's features check of tests/test_network_gpu.py, on its fixture's frames and with its limits."""
    if precision == "bf16":
        _sd, x, _taps, _drift, feats_emu, feats_ref = oracle_bf16()
        check_features_bf16(bb, x, feats_emu, feats_ref)
    elif precision == "fp16":
        _sd, x, ref, emu, _taps = oracle_fp16()
        check_features_fp16(bb, x, ref, emu)
    elif precision == "bf16w2":
        _sd, x, ref, emu, _taps = oracle_bf16w2()
        check_features_bf16w2(bb, x, ref, emu)
    elif precision == "fp32x":
        _sd, x, _taps, feats_ref = oracle_fp32x()
        check_features_fp32x(bb, x, feats_ref)
    else:
        _sd, x, emu, ref = oracle_fp8(tuple(bb.fp8_scales))
        check_features_fp8(bb, x, emu, ref)
