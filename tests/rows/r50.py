"""The guard-band rows of include/r50.h: ``ROWS``.  What a row is and how the harnesses run it: tests/guard_bands.py and
tests/rows/__init__.py; what the table covers and what it cannot see: tests/test_guard_bands_gpu.py."""
import ctypes
import functools

import torch

from tests import guard_bands as G
from tests import pair_reference as P
from tests.guard_bands import BF, DEV, F32, F64, HF, I32, U8, Row, lib, ok, ptr, stream
from tests.kernel_cases import (CAT_CASES, CONV_CASES, FP8_CASES, HEAD_GEMMS, _assert_matches, _case_inputs, _cast_source, _clip, _conv_inputs,
                                _gn_inputs, _lerp_fp32, _out_shape, _refused_ids, _split_case, _tail3_inputs, _tiles_for, _ulps, _w2_case)
from tests.network_oracles import _oracle_bar
from tests.sequence_cases import T, _metric_case, _poses, _stitch_clips

ET = {0: BF, 1: HF}
EPS = 1e-5

# Entry points of include/r50.h without a row below.  The only acceptable reason: the call takes no device operand.
NOT_GUARDED = {
    "r50_stem_scratch_bytes": "size query: no device operand",
    "r50_op_nn_search_workspace": "size query: no device operand",
}

ROWS = []


def _add(family, rid, ops, make, launch, check=None, scrub=None):
    ROWS.append(Row(family, rid, (ops,) if isinstance(ops, str) else tuple(ops), make, launch, check, scrub))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, shape, dtype=F32, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _conv_reach(w, cin, cout, k, pad, es=2, xmul=1, ymul=1, tile_rows=256):
    x_back = (pad * w + pad) * cin * xmul * es
    soff = ((k - 1) * w + (k - 1)) * cin * xmul * es
    tile = tile_rows * max(cin * xmul, cout * ymul) * es
    return max(x_back, soff, tile)


def _case_id(c):
    return "n%d_%dx%d_c%d-%d_k%ds%dp%d_r%d_res%d" % tuple(int(v) for v in c[:10])


# ------------------------------------------------------------------------------------------------------------------------------
# igemm: bf16 and fp16 over every tile id of _tiles_for; the shape-specialised conv kernels
# ------------------------------------------------------------------------------------------------------------------------------
IGEMM_CASES = [c for c in CONV_CASES if c[:8] in {
    (3, 5, 5, 64, 256, 1, 1, 0), (2, 8, 8, 256, 512, 1, 2, 0), (3, 7, 7, 64, 64, 3, 1, 1), (2, 9, 9, 128, 128, 3, 2, 1),
    (1, 1, 1, 64, 64, 3, 1, 1), (3, 5, 9, 128, 256, 3, 1, 1), (3, 9, 9, 64, 256, 1, 1, 0)}]
assert len(IGEMM_CASES) == 7, f"{len(IGEMM_CASES)} of the seven igemm shapes are in CONV_CASES"


def _conv_launch(case, tiles, et):
    def launch(a, pay):
        from implementation_phd_lab_vision_amd import ops
        n, h, w, cin, cout, k, stride, pad, relu, has_res = case
        xd, wd, bd, rd, _ref, (ho, wo) = pay
        a.reach(_conv_reach(w, cin, cout, k, pad))
        x, wt, b = a.inp("x", xd), a.inp("w", wd), a.inp("bias", bd)
        r = a.inp("residual", rd) if has_res else None
        for tile in tiles:
            y = a.out(f"y[tile {tile}]", (n, ho, wo, cout), et)
            ops.conv2d_bf16(x, wt, b, stride=stride, pad=pad, relu=relu, residual=r, tile=tile, out=y)
    return launch


for _et, _nm in ((BF, "bf16"), (HF, "fp16")):
    for _c in IGEMM_CASES:
        _add("igemm", f"conv2d_{_nm}-{_case_id(_c)}", "r50_op_conv2d" if _et == BF else "r50_op_conv2d_f16",
             functools.partial(_conv_inputs, _c, _et), _conv_launch(_c, _tiles_for(_c[4], _c[5], _c[7]), _et))

SPECIAL = {80: [(1, 56, 56, 64, 64, 3, 1, 1)], 81: [(5, 7, 7, 512, 512, 3, 1, 1), (3, 28, 28, 128, 128, 3, 1, 1), (3, 14, 14, 256, 256, 3, 1, 1)],
           82: [(3, 56, 56, 128, 128, 3, 2, 1), (1, 28, 28, 256, 256, 3, 2, 1), (5, 14, 14, 512, 512, 3, 2, 1)]}
for _tile, _heads in SPECIAL.items():
    for _hd in _heads:
        _c = [c for c in CONV_CASES if c[:8] == _hd][-1]
        _add("special_conv", f"tile{_tile}-{_case_id(_c)}", "r50_op_conv2d", functools.partial(_conv_inputs, _c, BF), _conv_launch(_c, [_tile], BF))

# the head's GEMMs (r50_op_conv2d(_f16) with n = rows, h = w = 1): ragged rows, K padded to 64 / 1088
HEAD_ROWS = [s for s in HEAD_GEMMS if s[:3] in {(32, 1088, 1024), (32, 3072, 1024), (1024, 64, 3072)}]
assert len(HEAD_ROWS) == 3, f"{len(HEAD_ROWS)} of the three head shapes are in HEAD_GEMMS"


def _head_gemm_make(shape, et):
    rows, k, cout, relu, has_res, kind = shape[:6]
    g = _gen(rows + 3 * k + 7 * cout + et)
    x, w = _rn(g, (rows, k), ET[et]), _rn(g, (cout, k), ET[et], (2.0 / k) ** 0.5)
    if kind == "dw":
        x[:, shape[6]:] = 0
        w[:, shape[6]:] = 0
    bias = _rn(g, (cout,), F32, 0.1) if kind == "fwd" else torch.zeros(cout)
    return x, w, bias, (_rn(g, (rows, cout), ET[et]) if has_res else None)


def _head_gemm_launch(shape, et):
    def launch(a, pay):
        from implementation_phd_lab_vision_amd import ops
        rows, k, cout, relu, has_res = shape[:5]
        x, w, bias, res = pay
        a.reach(_conv_reach(1, k, cout, 1, 0))
        xd, wd, bd = a.inp("x", x.view(rows, 1, 1, k)), a.inp("w", w.view(cout, 1, 1, k)), a.inp("bias", bias)
        rd = a.inp("residual", res.view(rows, 1, 1, cout)) if has_res else None
        for tile in _tiles_for(cout, 1, 0):
            y = a.out(f"y[tile {tile}]", (rows, 1, 1, cout), ET[et])
            ops.conv2d_bf16(xd, wd, bd, relu=relu, residual=rd, tile=tile, out=y)
    return launch


for _et in (1, 0):
    for _sh in HEAD_ROWS:
        _add("head_gemm", "%s-%s_m%d_k%d_n%d" % ("fp16" if _et else "bf16", _sh[5], _sh[0], _sh[1], _sh[2]),
             "r50_op_conv2d_f16" if _et else "r50_op_conv2d", functools.partial(_head_gemm_make, _sh, _et), _head_gemm_launch(_sh, _et))


# ------------------------------------------------------------------------------------------------------------------------------
# pair precisions, fp8, two K sources
# ------------------------------------------------------------------------------------------------------------------------------
# The four smallest rows of PAIR_CASES, each with a ragged last tile: M = 75 (1x1, residual), M = 1 (3x3, every tap but the centre is padding:
# the strongest halo case), M = 50 (3x3 stride 2), M = 135 (3x3, halo rows cross image borders, residual).  The other rows are the large-K ones.
PAIR_ROWS = list(P.PAIR_CASES[:4])


def _w2_launch(case):
    def launch(a, pay):
        from implementation_phd_lab_vision_amd import ops
        n, h, w, cin, cout, k, stride, pad, relu, has_res = case
        xd, wd, bd, rd, _ref = pay
        a.reach(_conv_reach(w, 2 * cin, cout, k, pad))
        x, wt, b = a.inp("x", xd), a.inp("w_pair", wd), a.inp("bias", bd)
        r = a.inp("residual", rd) if has_res else None
        for tile in [t for t in _tiles_for(cout, k, pad) if t not in _refused_ids()]:
            y = a.out(f"y[tile {tile}]", _out_shape(case), BF)
            ops.conv2d_w2(x, wt, b, stride=stride, pad=pad, relu=relu, residual=r, tile=tile, out=y)
    return launch


def _split_launch(case):
    def launch(a, pay):
        from implementation_phd_lab_vision_amd import ops
        n, h, w, cin, cout, k, stride, pad, relu, has_res = case
        xd, wd, bd, rd, _ref = pay
        a.reach(_conv_reach(w, cin, cout, k, pad, xmul=3, ymul=2))
        x, wt, b = a.inp("x_pair", xd), a.inp("w_trip", wd), a.inp("bias", bd)
        r = a.inp("residual_pair", rd) if has_res else None
        n_, ho, wo, _ = _out_shape(case)
        y = a.out("y_pair", (n_, ho, wo, 2 * cout), BF)
        ops.conv2d_split(x, wt, b, stride=stride, pad=pad, relu=relu, residual_pair=r, out=y)
    return launch


for _c in PAIR_ROWS:
    _add("pair_fp8_cat", f"conv2d_w2-{_case_id(_c)}", "r50_op_conv2d_w2", functools.partial(_w2_case, _c), _w2_launch(_c))
    _add("pair_fp8_cat", f"conv2d_split-{_case_id(_c)}", "r50_op_conv2d_split", functools.partial(_split_case, _c), _split_launch(_c))

FP8_ROWS = [FP8_CASES[1], FP8_CASES[3], FP8_CASES[4]]     # M = 75 (residual), 147 (3x3), 50 (3x3 stride 2): the ragged rows


def _fp8_make(case):
    from implementation_phd_lab_vision_amd import ops
    n, h, w, cin, cout, k, stride, pad, relu, has_res, tile = case
    g = _gen(cin * 7 + cout + k)
    sx, sw, sr = 0.05, 0.002, 0.04
    xq = (torch.randn(n, h, w, cin, generator=g) / sx * 0.5).clamp(-448, 448).to(ops.FP8)
    wq = (torch.randn(cout, k, k, cin, generator=g) * (1.0 / (k * k * cin)) ** 0.5 / sw).clamp(-448, 448).to(ops.FP8)
    bias = torch.randn(cout, generator=g) * 0.1 / (sx * sw)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    rq = (torch.randn(n, ho, wo, cout, generator=g) / sr * 0.5).clamp(-448, 448).to(ops.FP8) if has_res else None
    return xq, wq, bias, rq, (ho, wo)


def _fp8_launch(case):
    def launch(a, pay):
        from implementation_phd_lab_vision_amd import ops
        n, h, w, cin, cout, k, stride, pad, relu, has_res, tile = case
        xq, wq, bias, rq, (ho, wo) = pay
        sx, sw, sr, sy = 0.05, 0.002, 0.04, 0.03
        a.reach(_conv_reach(w, cin, cout, k, pad, es=1))
        x, wt, b = a.inp("x", xq), a.inp("w", wq), a.inp("bias_scaled", bias)
        r = a.inp("residual", rq) if has_res else None
        for t in (0, tile):
            y = a.out(f"y[tile {t}]", (n, ho, wo, cout), ops.FP8)
            ok(lib().r50_op_conv2d_fp8(ptr(x), n, h, w, cin, ptr(wt), ptr(b), ptr(r), ptr(y), cout, k, stride, pad, int(relu),
                                         sx * sw / sy, sr / sy, t, stream()), "r50_op_conv2d_fp8")
    return launch


for _c in FP8_ROWS:
    _add("pair_fp8_cat", "conv2d_fp8-" + _case_id(_c) + "_t%d" % _c[10], "r50_op_conv2d_fp8", functools.partial(_fp8_make, _c), _fp8_launch(_c))

CAT_ROWS = [CAT_CASES[0], CAT_CASES[1], CAT_CASES[3], CAT_CASES[7]]       # stride2 = 2 (M = 32, 147), stride2 = 1, the eight-phase tile


def _cat_make(case, et):
    n, h, c1, h2, c2, s2, cout, relu, tile = case
    g = _gen(h * 131 + c2)
    return (_rn(g, (n, h, h, c1), et), _rn(g, (n, h2, h2, c2), et), _rn(g, (cout, c1 + c2), et, (1.0 / (c1 + c2)) ** 0.5),
            _rn(g, (cout,), F32, 0.1))


def _cat_launch(case, et):
    def launch(a, pay):
        n, h, c1, h2, c2, s2, cout, relu, tile = case
        a.reach(max(_conv_reach(h, c1, cout, 1, 0), _conv_reach(h2, c2, cout, 1, 0), s2 * h2 * c2 * 2))
        x1, x2, wc, b = (a.inp(nm, t) for nm, t in zip(("x1", "x2", "wcat", "bias"), pay))
        y = a.out("y", (n, h, h, cout), et)
        ok(lib().r50_op_conv1x1_cat(ptr(x1), n, h, h, c1, ptr(x2), h2, h2, c2, s2, ptr(wc), ptr(b), ptr(y), cout, int(relu), tile,
                                      1 if et == HF else 0, stream()), "r50_op_conv1x1_cat")
    return launch


for _et, _nm in ((BF, "bf16"), (HF, "fp16")):
    for _c in CAT_ROWS:
        _add("pair_fp8_cat", "conv1x1_cat_%s-n%d_%d_c%d_src%d_c%d_s%d_o%d_t%d" % ((_nm,) + _c[:7] + (_c[8],)), "r50_op_conv1x1_cat",
             functools.partial(_cat_make, _c, _et), _cat_launch(_c, _et))


# ------------------------------------------------------------------------------------------------------------------------------
# fused bodies and tails
# ------------------------------------------------------------------------------------------------------------------------------
def _tail_make(shape, cmid, c1, ds, seed):
    n, h, w = shape
    g = _gen(seed)
    cout = 4 * cmid
    pay = {"y2": _rn(g, (n, h, w, cmid), BF), "w3": _rn(g, (cout, cmid), BF, (2.0 / cmid) ** 0.5), "b3": _rn(g, (cout,), F32, 0.1)}
    if c1:
        pay["w1"], pay["b1"] = _rn(g, (c1, cout), BF, (2.0 / cout) ** 0.5), _rn(g, (c1,), F32, 0.1)
    if ds:
        pay["identity"] = _rn(g, (n, h, w, cmid), BF)
        pay["wd"], pay["bd"] = _rn(g, (cout, cmid), BF, (1.0 / cmid) ** 0.5), _rn(g, (cout,), F32, 0.1)
    else:
        pay["identity"] = _rn(g, (n, h, w, cout), BF)
    return pay


def _tail3_make(shape, c1, seed):
    """The layer3 tails' payloads from tests/test_kernels_gpu.py's own builder (NCHW / (cout, cin, 1, 1) there, NHWC / (cout, cin) here)."""
    n, h, w = shape
    y2, w3, b3, idn, w1, b1 = _tail3_inputs(n, h, w, seed)
    pay = {"y2": y2.permute(0, 2, 3, 1).contiguous(), "w3": w3.view(1024, 256).contiguous(), "b3": b3, "identity": idn.permute(0, 2, 3, 1).contiguous()}
    if c1:
        pay["w1"], pay["b1"] = w1.view(256, 1024).contiguous(), b1
    return pay


def _tail_launch(shape, cmid, c1, bp=None):
    def launch(a, pay):
        import os
        n, h, w = shape
        m, cout = n * h * w, 4 * cmid
        a.reach(256 * cout * 2)
        d = {k: a.inp(k, v) for k, v in pay.items()}
        out = a.out("out", (n, h, w, cout), BF)
        y1n = a.out("y1n", (n, h, w, c1), BF) if c1 else None
        old = os.environ.get("R50_TAIL3_BP")
        if bp:
            os.environ["R50_TAIL3_BP"] = str(bp)
        else:
            os.environ.pop("R50_TAIL3_BP", None)
        try:
            rc = lib().r50_op_bneck_tail(ptr(d["y2"]), m, cmid, ptr(d["w3"]), ptr(d["b3"]), ptr(d["identity"]), ptr(d.get("wd")), ptr(d.get("bd")),
                                          ptr(out), ptr(d.get("w1")), c1, ptr(d.get("b1")), ptr(y1n), stream())
        finally:
            os.environ.pop("R50_TAIL3_BP", None)
            if old is not None:
                os.environ["R50_TAIL3_BP"] = old
        ok(rc, "r50_op_bneck_tail")
    return launch


for _shape in ((2, 7, 9), (3, 5, 16)):
    _sid = "%dx%dx%d" % _shape
    for _ds in (False, True):
        _add("fused", f"bneck_tail-layer1-{_sid}-{'downsample' if _ds else 'identity'}", "r50_op_bneck_tail",
             functools.partial(_tail_make, _shape, 64, 64, _ds, 1000 + sum(_shape)), _tail_launch(_shape, 64, 64))
    _add("fused", f"bneck_tail-layer2-{_sid}", "r50_op_bneck_tail", functools.partial(_tail_make, _shape, 128, 128, False, 2000 + sum(_shape)),
         _tail_launch(_shape, 128, 128))
for _shape, _bp in (((2, 7, 9), 0), ((3, 14, 14), 98)):
    _add("fused", "bneck_tail-layer3-%dx%dx%d-bp%d" % (_shape + (_bp,)), "r50_op_bneck_tail",
         functools.partial(_tail3_make, _shape, 256, 3000 + _shape[0] * _shape[1] * _shape[2] + _bp), _tail_launch(_shape, 256, 256, _bp))
for _n in (1, 5):
    _add("fused", f"bneck_tail-layer3.5-n{_n}", "r50_op_bneck_tail", functools.partial(_tail3_make, (_n, 14, 14), 0, 4100 + _n),
         _tail_launch((_n, 14, 14), 256, 0))


def _body_make(n, hw, cmid, c1, seed, ds=False):
    g = _gen(seed)
    cout = 4 * cmid
    pay = {"t1": _rn(g, (n, hw, hw, cmid), BF).clamp_(min=0), "w2": _rn(g, (cmid, 3, 3, cmid), BF, (2.0 / (9 * cmid)) ** 0.5),
           "b2": _rn(g, (cmid,), F32, 0.1), "w3": _rn(g, (cout, cmid), BF, (2.0 / cmid) ** 0.5), "b3": _rn(g, (cout,), F32, 0.1)}
    if ds:
        pay["x"] = _rn(g, (n, hw, hw, cmid), BF).clamp_(min=0)
        pay["wd"], pay["bd"] = _rn(g, (cout, cmid), BF, (1.0 / cmid) ** 0.5), _rn(g, (cout,), F32, 0.1)
    else:
        pay["identity"] = _rn(g, (n, hw, hw, cout), BF).clamp_(min=0)
    if c1:
        pay["w1"], pay["b1"] = _rn(g, (c1, cout), BF, (2.0 / cout) ** 0.5), _rn(g, (c1,), F32, 0.1)
    return pay


def _body_launch(kind, n, hw, cmid, c1):
    def launch(a, pay):
        cout = 4 * cmid
        a.reach(max(_conv_reach(hw, cmid, cmid, 3, 1), 256 * cout * 2))
        d = {k: a.inp(k, v) for k, v in pay.items()}
        out = a.out("out", (n, hw, hw, cout), BF)
        y1n = a.out("y1n", (n, hw, hw, c1), BF) if c1 else None
        L = lib()
        if kind == "block1":
            rc = L.r50_op_bneck_block1(ptr(d["t1"]), n, ptr(d["w2"]), ptr(d["b2"]), ptr(d["w3"]), ptr(d["b3"]), ptr(d["identity"]), ptr(out),
                                       ptr(d["w1"]), c1, ptr(d["b1"]), ptr(y1n), stream())
        elif kind == "block1_ds":
            rc = L.r50_op_bneck_block1_ds(ptr(d["t1"]), n, ptr(d["w2"]), ptr(d["b2"]), ptr(d["w3"]), ptr(d["b3"]), ptr(d["x"]), ptr(d["wd"]),
                                          ptr(d["bd"]), ptr(out), ptr(d["w1"]), ptr(d["b1"]), ptr(y1n), stream())
        else:
            rc = L.r50_op_bneck_block2(ptr(d["t1"]), n, ptr(d["w2"]), ptr(d["b2"]), ptr(d["w3"]), ptr(d["b3"]), ptr(d["identity"]), ptr(out),
                                       ptr(d.get("w1")), ptr(d.get("b1")), ptr(y1n), stream())
        ok(rc, "r50_op_bneck_" + kind)
    return launch


for _n in (1, 3):
    for _c1 in (64, 128):
        _add("fused", f"bneck_block1-n{_n}-c1_{_c1}", "r50_op_bneck_block1", functools.partial(_body_make, _n, 56, 64, _c1, 5100 + _n + _c1),
             _body_launch("block1", _n, 56, 64, _c1))
    _add("fused", f"bneck_block1_ds-n{_n}", "r50_op_bneck_block1_ds", functools.partial(_body_make, _n, 56, 64, 64, 5300 + _n, True),
         _body_launch("block1_ds", _n, 56, 64, 64))
    for _chain in (False, True):
        _add("fused", f"bneck_block2-n{_n}-{'chained_conv1' if _chain else 'last_block'}", "r50_op_bneck_block2",
             functools.partial(_body_make, _n, 28, 128, 128 if _chain else 0, 4100 + _n), _body_launch("block2", _n, 28, 128, 128 if _chain else 0))


def _catchain_make(n):
    g = _gen(5100 + n)
    return {"t2": _rn(g, (n, 28, 28, 128), BF), "x": _rn(g, (n, 56, 56, 256), BF), "wcat": _rn(g, (512, 384), BF, (1.0 / 384) ** 0.5),
            "bcat": _rn(g, (512,), F32, 0.1), "w1": _rn(g, (128, 512), BF, (2.0 / 512) ** 0.5), "b1": _rn(g, (128,), F32, 0.1)}


def _catchain_launch(n):
    def launch(a, pay):
        a.reach(max(256 * 512 * 2, 2 * 56 * 256 * 2))
        d = {k: a.inp(k, v) for k, v in pay.items()}
        out, y1n = a.out("out", (n, 28, 28, 512), BF), a.out("y1n", (n, 28, 28, 128), BF)
        ok(lib().r50_op_bneck_cat_chain(ptr(d["t2"]), ptr(d["x"]), n, 28, ptr(d["wcat"]), ptr(d["bcat"]), ptr(out), ptr(d["w1"]), ptr(d["b1"]),
                                          ptr(y1n), stream()), "r50_op_bneck_cat_chain")
    return launch


for _n in (1, 3):
    _add("fused", f"bneck_cat_chain-n{_n}", "r50_op_bneck_cat_chain", functools.partial(_catchain_make, _n), _catchain_launch(_n))


# ------------------------------------------------------------------------------------------------------------------------------
# stem, pools, network
# ------------------------------------------------------------------------------------------------------------------------------
def _stem_make(n):
    from implementation_phd_lab_vision_amd.weights import synthetic_frames, synthetic_state_dict
    from oracle.resnet50_oracle import folded
    wf, bf = folded(synthetic_state_dict(0), "conv1", "bn1")
    return synthetic_frames(n, seed=7), wf.to(F32).contiguous(), bf.to(F32)


def _stem_launch(n):
    def launch(a, pay):
        x, wf, bf = pay
        a.reach(max(2 * 7 * 224 * 4, 256 * 64 * 2))            # seven fp32 input rows of a 7x7 s2 window pair; one tile of output rows
        xd, bd = a.inp("x", x), a.inp("bias", bf)
        scratch = a.ws("scratch", (int(lib().r50_stem_scratch_bytes(n)),), U8)
        y = a.out("y", (n, 112, 112, 64), BF)
        ok(lib().r50_op_stem(ptr(xd), n, wf.data_ptr(), ptr(bd), ptr(scratch), ptr(y), stream()), "r50_op_stem")
    return launch


for _n in (1, 3):
    _add("stem_pools_network", f"stem-n{_n}", "r50_op_stem", functools.partial(_stem_make, _n), _stem_launch(_n))


def _pool_launch(kind, shape):
    def launch(a, x):
        n, h, w, c = shape
        a.reach(3 * w * c * 2)
        xd = a.inp("x", x)
        if kind == "max":
            y = a.out("y", (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), BF)
            ok(lib().r50_op_maxpool(ptr(xd), n, h, w, c, ptr(y), stream()), "r50_op_maxpool")
        else:
            y = a.out("y", (n, c), F32)
            ok(lib().r50_op_avgpool(ptr(xd), n, h * w, c, ptr(y), stream()), "r50_op_avgpool")
    return launch


for _sh in ((1, 7, 9, 8), (3, 5, 5, 72)):
    _add("stem_pools_network", "maxpool-%dx%dx%dx%d" % _sh, "r50_op_maxpool", functools.partial(lambda s: _rn(_gen(11), s, BF), _sh),
         _pool_launch("max", _sh))
for _sh in ((1, 3, 3, 8), (4, 7, 7, 2048)):
    _add("stem_pools_network", "avgpool-%dx%dx%dx%d" % _sh, "r50_op_avgpool", functools.partial(lambda s: _rn(_gen(13), s, BF), _sh),
         _pool_launch("avg", _sh))


NET_N = (1, 3)           # frames per call; max_batch = 4


def _net_make(precision):
    """A handle, uint8 frames (a black and a white frame among them) and the reference's host path of the same frames, (u8 / 255 - mean) / std."""
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_state_dict
    bb = ResNet50Backbone(state_dict=synthetic_state_dict(0), max_batch=4, precision=precision).to(DEV).eval()
    u8 = torch.randint(0, 256, (max(NET_N), 3, 224, 224), generator=_gen(21), dtype=U8)
    u8[1], u8[2] = 0, 255
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    other = torch.rand((max(NET_N), 3, 224, 224), generator=_gen(22)).to(DEV)       # another batch, for ``_net_scrub``
    return bb, (u8.to(F32) / 255.0 - mean) / std, u8, other


def _net_launch(a, pay):
    bb, x, u8, other = pay
    a.reach(2 * 7 * 224 * 4)            # the stem's window: seven fp32 input rows, two strips deep
    for n in NET_N:                     # n = 1: the uint8 packer and the stem with a single frame between the bands
        xd, ud = a.inp(f"x[n {n}]", x[:n]), a.inp(f"x_u8[n {n}]", u8[:n])
        fo, uo = a.out(f"features[n {n}]", (n, 2048), F32), a.out(f"features_u8[n {n}]", (n, 2048), F32)
        if n != NET_N[0]:
            a.between_calls(lambda: bb.features(other))
        bb.features(xd, out=fo)
        a.between_calls(lambda: bb.features(other))      # the four calls run the same frames through the same buffers
        bb.features_u8(ud, out=uo)


def _net_scrub(pay):
    """Another batch through the handle: its activation buffers then hold that batch's values, not the last run's.  (tests/stream_order.py's ``run_row_late``
    runs this between its two runs: a branch of r50_forward that read a buffer before the caller's stream had written it would otherwise
    find there what the same frames left a moment ago; ``_net_launch`` asks for the same between its own calls.)"""
    bb, _x, _u8, other = pay
    bb.features(other)
    torch.cuda.synchronize()


def _net_check(precision):
    def check(plain, pay):
        """The row's own results: uint8 frames give the bits of the host-normalised frames (tests/test_network_gpu.py's uint8 statement), and
        the frame run alone gives the bits it has in the batch of three.  max_batch = 4 is this table's own, so the handle also goes through
        that precision's oracle check of tests/test_network_gpu.py (its frames, its limits; the oracles are computed once per session)."""
        r = plain.results
        for n in NET_N:
            assert torch.isfinite(r[f"features[n {n}]"]).all(), f"n {n}: features that are not finite"
            assert torch.equal(r[f"features_u8[n {n}]"], r[f"features[n {n}]"]), f"n {n}: uint8 frames differ from host-normalised frames"
        assert torch.equal(r["features[n 1]"][0], r["features[n 3]"][0]), "frame 0 alone differs from frame 0 in the batch"
        _oracle_bar(precision, pay[0])
    return check


for _prec in ("bf16", "fp16", "fp8", "bf16w2", "fp32x"):
    _add("stem_pools_network", f"features-features_u8-{_prec}-n1-n3-max_batch4", ("r50_forward", "r50_forward_u8"), functools.partial(_net_make, _prec),
         _net_launch, _net_check(_prec), _net_scrub)


# ------------------------------------------------------------------------------------------------------------------------------
# frame ops (uint8: a stray read under a zero weight stays invisible; these rows see nonzero-weight reads and every write)
# ------------------------------------------------------------------------------------------------------------------------------
def _frames_make(t, h, w, seed):
    return torch.randint(0, 256, (t, h, w, 3), generator=_gen(seed), dtype=U8)


def _crop_launch(h, w, top, left, side, mode):
    def launch(a, fr):
        a.reach(2 * w * 3)
        f = a.inp("frames", fr)
        for flags in (0, 3):
            out = a.out(f"out[flags {flags}]", (2, 3, 224, 224), U8)
            ok(lib().r50_op_crop_resize_u8(ptr(f), 2, h, w, top, left, side, side, ptr(out), 224, mode, flags, stream()), "r50_op_crop_resize_u8")
    return launch


for _cs in ((1002, 1000, 0, 0, 1000), (1000, 1002, 776, 778, 224), (64, 64, 10, 11, 1)):       # rows of tests/test_frames_gpu.py's CASES
    for _mode in (0, 1):
        _add("frames", "crop_resize_u8-%dx%d_box%d_%d_%d-" % _cs + ("fixed" if _mode else "float"), "r50_op_crop_resize_u8",
             functools.partial(_frames_make, 2, _cs[0], _cs[1], _cs[0] * 7 + _cs[4]), _crop_launch(*_cs, _mode))


def _resize_launch(a, pay):
    fr, idx, buf = pay
    n, h, w, _ = fr.shape
    a.reach(2 * w * 3)
    f, i = a.inp("frames", fr), a.inp("src_idx", idx)
    b = a.inout("out_buffer", buf)                       # (3 clips, t, 33, 33, 3): the call fills clip 1 and leaves clips 0 and 2 alone
    ok(lib().r50_op_resize_frames_u8(ptr(f), n, h, w, ptr(i), idx.numel(), b[1].data_ptr(), 33, stream()), "r50_op_resize_frames_u8")


# the shape of test_resize_kernel_writes_only_its_slice: src_idx names frame 0 and frame n - 1
_add("frames", "resize_frames_u8-first_and_last_frame-clip_slice", "r50_op_resize_frames_u8",
     lambda: (torch.randint(0, 256, (6, 50, 70, 3), dtype=U8, generator=_gen(3)), torch.tensor([5, 2, 2, 0, 4], dtype=I32),
              torch.randint(0, 256, (3, 5, 33, 33, 3), generator=_gen(6), dtype=U8)), _resize_launch)


def _jitter_make():
    from oracle import colorjitter_oracle as cj
    p = cj.sample_params(_gen(100))
    p["fn_idx"] = [2, 0, 3, 1]
    return _clip(0, t=2, h=64, w=48), p


def _jitter_launch(a, pay):
    u8, p = pay
    a.reach(256 * 16)
    f = a.inp("frames_u8", u8)
    order = (ctypes.c_int * 4)(*p["fn_idx"])
    for norm in (0, 1):
        out = a.out(f"out[normalize {norm}]", (2, 3, 64, 48), F32)
        means = a.ws(f"scratch_means[{norm}]", (2,), F32)
        ok(lib().r50_op_color_jitter_u8(ptr(f), 2, 64 * 48, order, p["brightness"], p["contrast"], p["saturation"], p["hue"], norm, ptr(out),
                                          ptr(means), stream()), "r50_op_color_jitter_u8")


def _jitter_check(plain, pay):
    """tests/test_colorjitter_gpu.py's bars: 5e-6 of the oracle in [0, 1], 3e-5 after Normalize (5e-6 / std)."""
    from oracle import colorjitter_oracle as cj
    u8, p = pay
    d0 = float((plain.results["out[normalize 0]"].cpu() - cj.color_jitter(u8.float() / 255, p)).abs().max())
    d1 = float((plain.results["out[normalize 1]"].cpu() - cj.color_jitter_variant_u8(u8, p)).abs().max())
    assert d0 < 5e-6, f"max |d| {d0:.3g} from the oracle in [0, 1], bar 5e-6"
    assert d1 < 3e-5, f"max |d| {d1:.3g} from the oracle after Normalize, bar 3e-5"


_add("frames", "color_jitter_u8-t2", "r50_op_color_jitter_u8", _jitter_make, _jitter_launch, _jitter_check)


def _draw_make(name, with_bg):
    from tests import render_reference as rr
    bg, pts, style = rr.parity_inputs(name)
    return torch.from_numpy(pts), torch.from_numpy(style), torch.from_numpy(bg) if with_bg else None


def _draw_launch(name):
    def launch(a, pay):
        from tests import render_reference as rr
        pts, style, bg = pay
        f, h, w, layers, _seed = rr.PARITY_CASES[name]
        a.reach(4 * w * 3)
        p, s = a.inp("pts", pts), a.inp("style", style)
        b = a.inp("bg", bg) if bg is not None else None
        out = a.out("out", (f, h, w, 3), U8)
        flat = [v for e in rr.H36M_EDGES for v in e]
        ok(lib().r50_op_draw_skeletons_u8(ptr(b), 0x0A80FE, ptr(p), ptr(s), (ctypes.c_int * len(flat))(*flat), len(flat) // 2, f, h, w, layers, 17,
                                            rr.PARITY_HALF_WIDTH, rr.PARITY_JOINT_RADIUS, ptr(out), stream()), "r50_op_draw_skeletons_u8")
    return launch


def _draw_check(name):
    def check(plain, pay):
        """bg = NULL at the parity shapes: tests/test_render_gpu.py's bar against the same oracle."""
        from tests import render_reference as rr
        pts, style, _bg = pay
        f, h, w, layers, _seed = rr.PARITY_CASES[name]
        ref = rr.draw_reference(None, 0x0A80FE, pts.numpy(), style.numpy(), rr.H36M_EDGES, rr.PARITY_HALF_WIDTH, rr.PARITY_JOINT_RADIUS, hw=(h, w))
        _assert_matches(plain.results["out"].cpu().numpy(), ref, layers, f"{name}, bg NULL")
    return check


for _name in ("byte_37x53", "vec_32x64"):              # w % 4 != 0: the per-byte path; w % 4 == 0: the 12-byte path; joints outside the image
    _add("frames", f"draw_skeletons_u8-{_name}-bg", "r50_op_draw_skeletons_u8", functools.partial(_draw_make, _name, True), _draw_launch(_name))
    _add("frames", f"draw_skeletons_u8-{_name}-uniform", "r50_op_draw_skeletons_u8", functools.partial(_draw_make, _name, False), _draw_launch(_name),
         _draw_check(_name))


# ------------------------------------------------------------------------------------------------------------------------------
# head
# ------------------------------------------------------------------------------------------------------------------------------
N_TWO_GRIDS = 256 * 8192 + 1001
# Reach of a linear element-wise kernel (casts, row ops, ReLU / dropout backward, grad_accum, AdamW, the flag checks): a lane's address is
# a function of its global index alone and a lane moves at most 16 bytes, so a wrong tail predicate or grid-stride step lands at most one
# workgroup step off the operand: 256 lanes x 16 bytes.
EW = 256 * 16


def _tensors(pay):
    if isinstance(pay, torch.Tensor):
        yield pay
    elif isinstance(pay, dict):
        yield from _tensors(list(pay.values()))
    elif isinstance(pay, (list, tuple)):
        for v in pay:
            yield from _tensors(v)


def INDEXED(pay):
    """Reach of a kernel that finds its rows through a scalar offset or a device table (i0, s0, t0, frame 0 of a clip, `starts`, `src`,
    `offsets`, `perm`, `nn_row`, `group`): an index that is wrong but still an index of that operand -- the last window taken one past the end,
    the clamp at frame 0 taken one before it -- lands within one operand's length of it.  So: the bytes of the row's largest input."""
    return max(t.numel() * t.element_size() for t in _tensors(pay))


# The losses and the evaluation ops all index that way (gt at i0 .. i0 + p, frame s0 of every clip, contributor and window tables).
FAMILY_REACH = {"head": EW, "losses": INDEXED, "evaluation": INDEXED}


def _simple(family, rid, ops, make, body, reach=None, check=None):
    """reach: bytes, or a function of the payloads; None = the family's (FAMILY_REACH, with the reason there)."""
    reach = FAMILY_REACH[family] if reach is None else reach

    def launch(a, pay):
        a.reach(reach(pay) if callable(reach) else reach)
        body(a, pay, lib())
    _add(family, rid, ops, make, launch, check)


def _gn_bm_make(et, shape):
    from tests import head_kernels_reference as R
    b, t, c, groups = shape
    x, gamma, beta, g = _gn_inputs(et, 0, shape)
    amb = R.gn_relu_ambiguous(x, groups, gamma, beta, EPS, 2.0 ** -10)
    dr = R.zero_taps_of(torch.randn(b, t, 3 * c, generator=g), amb).to(ET[et])
    return {"x": x, "gamma": gamma, "beta": beta, "dr": dr, "add": torch.randn(b, t, c, generator=g).to(ET[et])}


def _gn_bm_check(et, shape):
    def check(plain, pay):
        """tests/test_head_kernels_gpu.py's GroupNorm bars (forward and backward against fp64) at this row's shape."""
        from tests import head_kernels_reference as R
        b, t, c, groups = shape
        x, gamma, beta, dr, add = (pay[k] for k in ("x", "gamma", "beta", "dr", "add"))
        ref, abs_term = R.gn_forward_bar(x, groups, gamma, beta, EPS)
        R.assert_within_rounding(plain.results["out"].cpu().view(b, t, 3 * c), ref, et, abs_term, "gn_relu_causal3")
        dx64, pg64, pb64 = R.gn_backward(x.double(), dr.double(), groups, gamma.double(), beta.double(), EPS)
        dx32, pg32, pb32 = R.gn_backward(x.float(), dr.float(), groups, gamma.float(), beta.float(), EPS)
        want = dx64 + add.double()
        R.assert_within_rounding(plain.results["dx"].cpu(), want, et, R.bar_from(dx32 + add.float(), want), "gn bwd dx")
        for name, p64, p32 in (("dgamma_part", pg64, pg32), ("dbeta_part", pb64, pb32)):
            d = float((plain.results[name].cpu().double() - p64).abs().max())
            assert d <= R.bar_from(p32, p64), f"gn bwd {name}: max |d| {d:.3g}"
    return check


TM = (4, 19, 256, 32)           # b, t, c, groups of test_tm_bwd_partial_emission_against_autograd


def _gn_tm_make(et, t0):
    b, t, c, _ = TM
    g = _gen(40 + et + 7 * t0)
    return {"x": (torch.randn(t, b, c, generator=g) * 2 + 0.3).to(ET[et]), "gamma": 1 + 0.1 * torch.randn(c, generator=g),
            "beta": 0.1 * torch.randn(c, generator=g), "add": torch.randn(t * b, c, generator=g).to(ET[et]),
            "dr": torch.randn((t - t0) * b, 3 * c, generator=g).to(ET[et])}


def _gn_tm_check(et, t0):
    def check(plain, pay):
        """Forward: the batch-major kernel's bits (tests/test_rollout_gpu.py).  Backward: fp64 autograd of the emitted rows under the bars of
        test_tm_bwd_partial_emission_against_autograd."""
        import torch.nn.functional as F
        b, t, c, groups = TM
        L = lib()
        x, gamma, beta = pay["x"], pay["gamma"], pay["beta"]
        x_bm = x.transpose(0, 1).contiguous().to(DEV)
        gd, bd = gamma.to(DEV), beta.to(DEV)
        ref = torch.empty((b * t, 3 * c), dtype=ET[et], device=DEV)
        ok(L.r50_op_gn_relu_causal3(ptr(x_bm), b, t, c, groups, ptr(gd), ptr(bd), EPS, ptr(ref), et, stream()), "gn")
        got = plain.results["out"].view(t - t0, b, 3 * c).transpose(0, 1)
        assert torch.equal(G.bits(got), G.bits(ref.view(b, t, 3 * c)[:, t0:])), "time-major rows differ from the batch-major kernel's"
        dr, add = pay["dr"], pay["add"]
        xd = x.double().permute(1, 2, 0).clone().requires_grad_(True)        # (b, c, t)
        y = F.relu(F.group_norm(xd, groups, gamma.double(), beta.double(), eps=EPS))
        idx = torch.arange(t)
        rows = torch.cat([y[:, :, (idx - 2).clamp_min(0)], y[:, :, (idx - 1).clamp_min(0)], y], dim=1)
        (rows[:, :, t0:].permute(2, 0, 1).reshape((t - t0) * b, 3 * c) * dr.double()).sum().backward()
        want = xd.grad.permute(2, 0, 1).reshape(t * b, c) + add.double()
        torch.testing.assert_close(plain.results["dx"].cpu().double(), want, rtol=2 ** -10 if et else 2 ** -7, atol=1e-4 * float(want.abs().max()))
        xh = F.group_norm(xd.detach(), groups, eps=EPS)
        yv = (xh * gamma.double().view(1, c, 1) + beta.double().view(1, c, 1)).clone().requires_grad_(True)
        r = torch.cat([F.relu(yv)[:, :, (idx - 2).clamp_min(0)], F.relu(yv)[:, :, (idx - 1).clamp_min(0)], F.relu(yv)], dim=1)
        (r[:, :, t0:].permute(2, 0, 1).reshape((t - t0) * b, 3 * c) * dr.double()).sum().backward()
        pg, pb = (yv.grad * xh).sum(-1), yv.grad.sum(-1)
        torch.testing.assert_close(plain.results["dgamma_part"].cpu().double(), pg, rtol=1e-4, atol=1e-4 * float(pg.abs().max()))
        torch.testing.assert_close(plain.results["dbeta_part"].cpu().double(), pb, rtol=1e-4, atol=1e-4 * float(pb.abs().max()))
    return check


def _flags_check(plain, pay):
    """n = 5001: tests/test_clip_ema_gpu.py's one-ulp bars of the norm and the coefficient; check_finite sees an inf at the last index."""
    import numpy as np
    gf = pay[0]
    x64 = gf.numpy().astype(np.float64)
    norm64 = np.sqrt(np.sum(x64 * x64))
    coef64 = min(1.0, 1.0 / (norm64 + 1e-6))
    clip2 = plain.results["clip2"].cpu().numpy()
    assert _ulps(clip2[1], np.float32(norm64)) <= 1.0 and _ulps(clip2[0], np.float32(coef64)) <= 1.0, \
        f"clip2 {clip2.tolist()} against coefficient {coef64} and norm {norm64}"
    st = plain.results["stats4"].tolist()
    assert st[0] == 1.0 and st[1] == float(coef64 < 1.0) and st[2] == st[3] and _ulps(st[2], np.float32(norm64)) <= 1.0, \
        f"stats4 {st} against coefficient {coef64} and norm {norm64}"
    bad = gf.clone()
    bad[-1] = float("inf")
    bd, found = bad.to(DEV), torch.zeros(1, dtype=I32, device=DEV)
    ok(lib().r50_op_check_finite(ptr(bd), bad.numel(), ptr(found), stream()), "check_finite")
    assert int(found) == 1, f"check_finite left the flag at {int(found)} with an inf at the last index"


def _flag_is_down(found, nm, fill):
    assert int(found) == 0, f"{nm}: the flag went up on finite data (fill {fill})"


ADAM = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
ADAM_STEP = 10_000


def _adam_check(et):
    def check(plain, pay):
        """n = 5001: tests/test_clip_ema_gpu.py's statement -- p, m, v, p16 are r50_op_adamw's bits on g * clip[0], ema is the fp32 lerp."""
        n = 5001
        p, m, v, g = (pay[k].to(DEV) for k in ("p", "m", "v", "g"))
        gc = g * pay["clip"].to(DEV)[0]
        p16, found = torch.empty(n, dtype=ET[et], device=DEV), torch.zeros(1, dtype=I32, device=DEV)
        ok(lib().r50_op_adamw(ptr(p), ptr(m), ptr(v), ptr(gc), ptr(p16), n, *ADAM, ADAM_STEP, ptr(found), et, stream()), "adamw")
        for name, want in (("p", p), ("m", m), ("v", v)):
            assert torch.equal(plain.results[name + "[clip_ema]"], want), f"{name}[clip_ema] is not r50_op_adamw's {name} on g * clip[0]"
        assert torch.equal(G.bits(plain.results["p16[clip_ema]"]), G.bits(p16)), "p16[clip_ema] is not r50_op_adamw's p16 on g * clip[0]"
        assert torch.equal(plain.results["ema[clip_ema]"], _lerp_fp32(pay["ema"].to(DEV), p, 0.1)), "ema[clip_ema] is not the fp32 lerp"
    return check


for _et in (1, 0):
    _nm = "fp16" if _et else "bf16"
    for _rows, _c, _cp in ((33, 33, 34), (1, 1, 2)):
        def _cast(a, x, L, rows=_rows, c=_c, cp=_cp, et=_et):
            dst = a.out("dst", (rows, cp), ET[et])
            ok(L.r50_op_cast_rows(ptr(a.inp("src", x)), rows, c, ptr(dst), cp, et, stream()), "cast_rows")
        _simple("head", f"cast_rows-{_nm}-r{_rows}_c{_c}_cp{_cp}", "r50_op_cast_rows",
                functools.partial(lambda r, c: _rn(_gen(r * 7 + c), (r, c), F32, 3.0), _rows, _c), _cast)

    def _concat(a, pay, L, et=_et):
        phi, y = pay
        dst = a.out("dst", (40, 1088), ET[et])
        ok(L.r50_op_concat_pad(ptr(a.inp("phi", phi)), 1024, ptr(a.inp("y", y)), 51, 40, ptr(dst), 1088, et, stream()), "concat_pad")
    _simple("head", f"concat_pad-{_nm}", "r50_op_concat_pad",
            functools.partial(lambda et: (_rn(_gen(11 + et), (40, 1024), ET[et]), _rn(_gen(12), (40, 51))), _et), _concat)

    def _addrows(a, pay, L, et=_et):
        y, dy = pay
        ok(L.r50_op_add_rows(ptr(a.inout("y", y)), 51, ptr(a.inp("dy", dy)), 64, 40, et, stream()), "add_rows")
    _simple("head", f"add_rows-{_nm}", "r50_op_add_rows",
            functools.partial(lambda et: (_rn(_gen(13), (40, 51)), _rn(_gen(14 + et), (40, 64), ET[et], 0.1)), _et), _addrows)

    def _ew3(a, pay, L, et=_et):
        n = N_TWO_GRIDS
        dy, act, mask, h, dst = pay
        ok(L.r50_op_relu_bwd(ptr(a.inout("dy", dy)), ptr(a.inp("act", act)), 1.0 / 0.9, n, et, stream()), "relu_bwd")
        hd = a.inout("x", h)
        ok(L.r50_op_mask_scale(ptr(hd), ptr(a.inp("mask", mask)), 1.0 / 0.9, n, et, stream()), "mask_scale")
        ok(L.r50_op_grad_accum(ptr(hd), 0.25, ptr(a.out("dst[accumulate 0]", (n,), F32)), n, 0, et, stream()), "grad_accum")
        ok(L.r50_op_grad_accum(ptr(hd), 0.25, ptr(a.inout("dst[accumulate 1]", dst)), n, 1, et, stream()), "grad_accum")

    def _ew3_make(et=_et):
        g, n = _gen(21 + et), N_TWO_GRIDS
        act = _rn(g, (n,), ET[et])
        act[::97] = 0.0
        return _rn(g, (n,), ET[et], 4.0), act, (torch.rand(n, generator=g) > 0.1).to(U8), _rn(g, (n,), ET[et], 4.0), _rn(g, (n,))
    _simple("head", f"relu_bwd-mask_scale-grad_accum-{_nm}", ("r50_op_relu_bwd", "r50_op_mask_scale", "r50_op_grad_accum"), _ew3_make, _ew3)

    for _acc in (0, 1):
        def _colsum(a, pay, L, et=_et, acc=_acc):
            x, xf, o0, xs = pay
            rows, cols, ld = 10240, 51, 115

            def target(nm):
                return a.inout(nm, o0) if acc else a.out(nm, (cols,), F32)
            xd = a.inp("x", x)
            ok(L.r50_op_colsum(ptr(xd), rows, cols, ld, 0.37, ptr(target("out")), acc, et, stream()), "colsum")
            ok(L.r50_op_colsum_split(ptr(xd), rows, cols, ld, 0.37, ptr(a.ws("part", (16 * cols,), F32)), ptr(target("out_split")), acc, et, stream()),
                "colsum_split")
            ok(L.r50_op_colsum_f32(ptr(a.inp("x_f32", xf)), rows, cols, 2.0, ptr(target("out_f32")), acc, stream()), "colsum_f32")
            ok(L.r50_op_colsum_split(ptr(a.inp("x_small", xs)), 17, cols, 64, 1.0 / 256, ptr(a.ws("part_small", (16 * cols,), F32)),
                                      ptr(target("out_split_small")), acc, et, stream()), "colsum_split")        # (17, 51, 64): its own test's ragged case

        def _colsum_check(plain, pay):
            assert torch.equal(plain.results["out_split"], plain.results["out"]), "colsum_split is not colsum's bits"
        _simple("head", f"colsum-colsum_f32-colsum_split-{_nm}-cols51-accumulate{_acc}", ("r50_op_colsum", "r50_op_colsum_f32", "r50_op_colsum_split"),
                functools.partial(lambda et: (_rn(_gen(31 + et), (10240, 115), ET[et], 2.0), _rn(_gen(32), (10240, 51)), _rn(_gen(33), (51,)),
                                              _rn(_gen(34 + et), (17, 64), ET[et], 3.0)), _et),
                _colsum, reach=640 * 115 * 2, check=_colsum_check)          # one row group of colsum: 640 rows of ld elements

    def _tr(a, pay, L):
        for i, (rows, cols) in enumerate(((15, 64), (64, 51))):         # ld = 64: padding columns after 15 rows, none after 64
            src, dst0 = pay[i]
            ok(L.r50_op_transpose16(ptr(a.inp(f"src[{i}]", src)), rows, cols, ptr(a.inout(f"dst[{i}]", dst0)), 64, stream()), "transpose16")
    _simple("head", f"transpose16-{_nm}", "r50_op_transpose16",
            functools.partial(lambda et: [(_rn(_gen(41 + et + r), (r, c), ET[et]), _rn(_gen(42 + r), (c, 64), ET[et])) for r, c in ((15, 64), (64, 51))], _et),
            _tr, reach=64 * 64 * 2)             # one 64 x 64 tile of 16-bit elements

    for _shape in ((2, 3, 256, 32), (3, 1, 1024, 32)):
        def _gn(a, pay, L, et=_et, shape=_shape):
            b, t, c, groups = shape
            d = {k: a.inp(k, v) for k, v in pay.items()}
            out = a.out("out", (b * t, 3 * c), ET[et])
            ok(L.r50_op_gn_relu_causal3(ptr(d["x"]), b, t, c, groups, ptr(d["gamma"]), ptr(d["beta"]), EPS, ptr(out), et, stream()), "gn")
            dx, dg, db = a.out("dx", (b, t, c), ET[et]), a.out("dgamma_part", (b, c), F32), a.out("dbeta_part", (b, c), F32)
            ok(L.r50_op_gn_relu_causal3_bwd(ptr(d["dr"]), ptr(d["x"]), b, t, c, groups, ptr(d["gamma"]), ptr(d["beta"]), EPS, ptr(d["add"]), ptr(dx),
                                             ptr(dg), ptr(db), et, stream()), "gn bwd")
        _simple("head", "gn_relu_causal3-fwd-bwd-%s-b%dt%dc%dg%d" % ((_nm,) + _shape), ("r50_op_gn_relu_causal3", "r50_op_gn_relu_causal3_bwd"),
                functools.partial(_gn_bm_make, _et, _shape), _gn,
                reach=_shape[1] * 3 * _shape[2] * 2, check=_gn_bm_check(_et, _shape))      # one sample's causal rows: t rows of 3c elements

    for _t0 in (0, 9, 18):
        def _gntm(a, pay, L, et=_et, t0=_t0):
            b, t, c, groups = TM
            d = {k: a.inp(k, v) for k, v in pay.items()}
            out = a.out("out", ((t - t0) * b, 3 * c), ET[et])
            ok(L.r50_op_gn_relu_causal3_tm(ptr(d["x"]), b, t, t0, c, groups, ptr(d["gamma"]), ptr(d["beta"]), EPS, ptr(out), et, stream()), "gn_tm")
            dx, dg, db = a.out("dx", (t * b, c), ET[et]), a.out("dgamma_part", (b, c), F32), a.out("dbeta_part", (b, c), F32)
            ok(L.r50_op_gn_relu_causal3_tm_bwd(ptr(d["dr"]), ptr(d["x"]), b, t, t0, c, groups, ptr(d["gamma"]), ptr(d["beta"]), EPS, ptr(d["add"]),
                                                ptr(dx), ptr(dg), ptr(db), et, stream()), "gn_tm bwd")
        _simple("head", f"gn_relu_causal3_tm-fwd-bwd-{_nm}-b4t19-t0_{_t0}", ("r50_op_gn_relu_causal3_tm", "r50_op_gn_relu_causal3_tm_bwd"),
                functools.partial(_gn_tm_make, _et, _t0), _gntm, reach=19 * 4 * 3 * 256 * 2, check=_gn_tm_check(_et, _t0))    # t0 off by a whole sequence: t * b rows of 3c

    def _flags_make(et=_et):
        g = _gen(5 + et)
        return _rn(g, (5001,)), _rn(g, (5001,), ET[et])

    def _flags(a, pay, L, et=_et):
        gf, x16 = pay
        n = 5001
        gd = a.inp("g", gf)
        for nm, call in (("found[check_finite]", lambda f: L.r50_op_check_finite(ptr(gd), n, ptr(f), stream())),
                         ("found[check_overflow16]", lambda f, x=a.inp("x16", x16): L.r50_op_check_overflow16(ptr(x), n, ptr(f), et, stream()))):
            found = a.inout(nm, torch.zeros(1, dtype=I32))
            ok(call(found), nm)
            a.host_check(functools.partial(_flag_is_down, found, nm, a.fill))                         # the NaN band right behind the data
        found = a.inout("found[grad_norm]", torch.zeros(1, dtype=I32))
        clip2, stats4 = a.out("clip2", (2,), F32), a.inout("stats4", torch.zeros(4, dtype=F64))
        ok(L.r50_op_grad_norm(ptr(gd), n, 1.0, ptr(a.ws("part", (2,), F64)), 2, ptr(found), ptr(clip2), ptr(stats4), stream()), "grad_norm")
        a.host_check(functools.partial(_flag_is_down, found, "found[grad_norm]", a.fill))
    _simple("head", f"check_finite-check_overflow16-grad_norm-{_nm}-n5001", ("r50_op_check_finite", "r50_op_check_overflow16", "r50_op_grad_norm"),
            _flags_make, _flags, reach=4096 * 4, check=_flags_check)        # grad_norm: one workgroup's slice, at most 4096 floats

    def _adam_make(et=_et):
        g, n = _gen(77 + et), 5001
        return {"p": _rn(g, (n,)), "m": _rn(g, (n,), F32, 1e-2), "v": torch.rand(n, generator=g) * 1e-4, "g": _rn(g, (n,), F32, 1e-2),
                "ema": _rn(g, (n,)), "clip": torch.tensor([0.37, 123.0]), "found": torch.zeros(1, dtype=I32)}

    def _adam(a, pay, L, et=_et):
        n = 5001
        gd, fd, cl = a.inp("g", pay["g"]), a.inp("found_inf", pay["found"]), a.inp("clip", pay["clip"])
        p, m, v = (a.inout(k, pay[k]) for k in ("p", "m", "v"))
        ok(L.r50_op_adamw(ptr(p), ptr(m), ptr(v), ptr(gd), ptr(a.out("p16", (n,), ET[et])), n, *ADAM, ADAM_STEP, ptr(fd), et, stream()), "adamw")
        p2, m2, v2, ema = (a.inout(k + "[clip_ema]", pay[k]) for k in ("p", "m", "v", "ema"))
        ok(L.r50_op_adamw_clip_ema(ptr(p2), ptr(m2), ptr(v2), ptr(gd), ptr(a.out("p16[clip_ema]", (n,), ET[et])), n, *ADAM, ADAM_STEP, ptr(fd), ptr(cl),
                                    ptr(ema), 0.1, et, stream()), "adamw_clip_ema")
    _simple("head", f"adamw-adamw_clip_ema-{_nm}-n5001", ("r50_op_adamw", "r50_op_adamw_clip_ema"), _adam_make, _adam, check=_adam_check(_et))


def _mse(a, pay, L):
    y, gt = pay
    n = y.numel()
    ok(L.r50_op_mse_loss_grad(ptr(a.inp("y", y)), ptr(a.inp("gt", gt)), n, 1024.0, ptr(a.out("dy", (n,), F32)), ptr(a.out("loss2", (2,), F32)), stream()),
        "mse_loss_grad")


# one workgroup of 256 threads, each over ceil(joints / 256) consecutive joints of 12 bytes: a thread off by one lands one such chunk away
_simple("head", "mse_loss_grad-b256t40", "r50_op_mse_loss_grad", lambda: (_rn(_gen(17), (256 * 40 * 51,)), _rn(_gen(18), (256 * 40 * 51,))), _mse,
        reach=lambda pay: -(-(pay[0].numel() // 3) // 256) * 12)


# ------------------------------------------------------------------------------------------------------------------------------
# losses (the small rows of each op's own kernel test)
# ------------------------------------------------------------------------------------------------------------------------------
for _b, _t, _j in ((3, 5, 17), (1, 2, 1)):
    def _fut(a, pay, L, b=_b, t=_t, j=_j):
        y, gt = pay
        ok(L.r50_op_future_pose_loss_grad(ptr(a.inp("y_hat", y)), ptr(a.inp("gt", gt)), b, t, j, 64.0, ptr(a.out("dy", (b * t, j, 3), F32)),
                                           ptr(a.out("loss2", (2,), F32)), stream()), "future_pose_loss_grad")
    _simple("losses", f"future_pose_loss_grad-b{_b}t{_t}j{_j}", "r50_op_future_pose_loss_grad",
            functools.partial(lambda b, t, j: (_rn(_gen(b + t), (b * t, j, 3)), _rn(_gen(b + t + 1), (b * t, j, 3))), _b, _t, _j), _fut)

for _et in (1, 0):
    _nm = "fp16" if _et else "bf16"
    for _b, _t, _d, _lam, _ls in ((1, 3, 8, 1.0, 8.0), (2, 2, 64, 1.0, 1.0)):
        def _arl(a, pay, L, b=_b, t=_t, d=_d, lam=_lam, ls=_ls, et=_et):
            ar, phi, dphi = pay
            ok(L.r50_op_ar_latent_grad(ptr(a.inp("ar", ar)), ptr(a.inp("phi", phi)), ptr(a.inp("dphi_hat", dphi)), b, t, d, lam, ls,
                                        ptr(a.out("dar", (b, t, d), ET[et])), ptr(a.out("loss_lat", (1,), F32)), ptr(a.ws("row_part", (b * t,), F32)),
                                        et, stream()), "ar_latent_grad")
        _simple("losses", f"ar_latent_grad-{_nm}-b{_b}t{_t}d{_d}", "r50_op_ar_latent_grad",
                functools.partial(lambda b, t, d, et: (_rn(_gen(d), (b, t, d), ET[et]), _rn(_gen(d + 1), (b, t, d), ET[et]),
                                                       _rn(_gen(d + 2), (b, t, d), F32, 1.0 / (b * (t - 1) * d))), _b, _t, _d, _et), _arl)
    for _b, _k, _tg, _i0, _d, _lam, _ls in ((3, 1, 2, 1, 64, 1.0, 1.0), (2, 3, 7, 4, 8, 0.0, 4.0)):
        def _rl(a, pay, L, b=_b, k=_k, tg=_tg, i0=_i0, d=_d, lam=_lam, ls=_ls, et=_et):
            fut, phi, dfut = pay
            ok(L.r50_op_rollout_latent_grad(ptr(a.inp("fut", fut)), ptr(a.inp("phi", phi)), b, k, tg, i0, d, lam, ls, ptr(a.inout("dfut", dfut)),
                                             ptr(a.out("loss_lat", (1,), F32)), ptr(a.ws("row_part", (k * b,), F32)), et, stream()), "rollout_latent_grad")
        _simple("losses", f"rollout_latent_grad-{_nm}-b{_b}k{_k}t{_tg}i{_i0}d{_d}", "r50_op_rollout_latent_grad",
                functools.partial(lambda b, k, tg, d, et: (_rn(_gen(d + k), (k * b, d), ET[et]), _rn(_gen(d + k + 1), (b, tg, d), ET[et]),
                                                           _rn(_gen(d + k + 2), (k * b, d))), _b, _k, _tg, _d, _et), _rl)

for _b, _k, _tg, _i0, _j in ((3, 1, 2, 1, 17), (2, 3, 7, 4, 5)):          # i0 + k == t_gt: the last horizon is the last frame of gt
    def _rp(a, pay, L, b=_b, k=_k, tg=_tg, i0=_i0, j=_j):
        pred, gt = pay
        ok(L.r50_op_rollout_pose_loss_grad(ptr(a.inp("pred", pred)), ptr(a.inp("gt", gt)), b, k, tg, i0, j, 64.0, ptr(a.out("dy", (k * b, j, 3), F32)),
                                            ptr(a.out("loss2", (2,), F32)), stream()), "rollout_pose_loss_grad")
    _simple("losses", f"rollout_pose_loss_grad-b{_b}k{_k}t{_tg}i{_i0}j{_j}", "r50_op_rollout_pose_loss_grad",
            functools.partial(lambda b, k, tg, j: (_rn(_gen(j + k), (k * b, j, 3)), _rn(_gen(j + k + 1), (b, tg, j, 3))), _b, _k, _tg, _j), _rp)


def _joint(a, pay, L):
    y, gt = pay
    b, t, j = 1, 2, 17
    ok(L.r50_op_joint_pose_loss_grad(ptr(a.inp("y", y)), ptr(a.inp("gt", gt)), b, t, j, 0.5, 1024.0, ptr(a.out("dy", (2, b, t, j, 3), F32)),
                                      ptr(a.out("out4", (4,), F32)), stream()), "joint_pose_loss_grad")


_simple("losses", "joint_pose_loss_grad-b1t2j17", "r50_op_joint_pose_loss_grad", lambda: (_rn(_gen(61), (2, 1, 2, 17, 3)), _rn(_gen(62), (1, 2, 17, 3))),
        _joint)


def _geo_make():
    from tests.helpers import GOLDEN
    gold = torch.load(GOLDEN / "geo_golden.pt", map_location="cpu", weights_only=True)
    c = next(c for c in gold["op"] if c["name"] == "plain")            # (3, 5, 17): the smallest fixture case that admits s0 = 1 with a velocity term
    return c["pred"], c["joints3d"], c["joints2d"], c["K"], [int(v) for e in gold["edges"] for v in e]


def _geo(a, pay, L):
    y, g3, g2, K, flat = pay
    b, t, j, _ = y.shape
    ok(L.r50_op_geo_pose_loss_grad(ptr(a.inp("y", y)), ptr(a.inp("gt3d", g3)), ptr(a.inp("gt2d", g2)), ptr(a.inp("K", K)), b, t, 1, j,
                                    (ctypes.c_int * len(flat))(*flat), len(flat) // 2, 1e-4, 0.7, 1.3, 1e-6, 0.5, 4.0,
                                    ptr(a.out("dy", (b * t, j, 3), F32)), ptr(a.ws("part", (8 * b,), F64)), ptr(a.out("out8", (8,), F32)), stream()),
        "geo_pose_loss_grad")


_simple("losses", "geo_pose_loss_grad-plain_b3t5j17-s0_1", "r50_op_geo_pose_loss_grad", _geo_make, _geo)


# ------------------------------------------------------------------------------------------------------------------------------
# evaluation (the smallest rows of each op's own test, built by that test's builders)
# ------------------------------------------------------------------------------------------------------------------------------
def _pm_make():
    g = _gen(5)
    p = torch.randn(7, 17, 3, generator=g)
    return p, p + 0.1 * torch.randn(7, 17, 3, generator=g)


def _pm(a, pay, L):
    pred, gt = pay
    ok(L.r50_op_pose_metrics(ptr(a.inp("pred", pred)), ptr(a.inp("gt", gt)), 7, 17, ptr(a.inout("acc", torch.zeros(3, dtype=F64))), stream()), "pose_metrics")


_simple("evaluation", "pose_metrics-rows7j17", "r50_op_pose_metrics", _pm_make, _pm)


def _hm_make():
    b, t, j, i0, p = 5, 12, 17, 3, 7
    g = _gen(1)
    gt = torch.randn(b, t, j, 3, generator=g)
    return (gt[:, i0:i0 + p] + 0.05 * torch.randn(b, p, j, 3, generator=g) * torch.arange(1, p + 1).view(1, p, 1, 1)).contiguous(), gt


def _hm(a, pay, L):
    pred, gt = pay
    ok(L.r50_op_horizon_metrics(ptr(a.inp("pred", pred)), ptr(a.inp("gt", gt)), 5, 7, 12, 3, 17, ptr(a.inout("acc", torch.zeros(15, dtype=F64))), stream()),
        "horizon_metrics")


_simple("evaluation", "horizon_metrics-b5p7t12i3", "r50_op_horizon_metrics", _hm_make, _hm)


def _detail_make(case):
    from tests import detail_reference as dr
    pred, gt, group = dr.case_inputs(case)
    return torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy()), torch.tensor(group.tolist(), dtype=I32)


for _case in ((5, 3, 7, 2, 17, 4, 0, 31), (7, 4, 4, 0, 1, 2, 0, 2)):           # rows of detail_reference.CASES, the first seven fields also protocols'
    def _pp(a, pay, L, case=_case):
        from tests import detail_reference as dr
        b, p, t_gt, i0, j, ng, root, n_thr = case
        pred, gt, group = pay
        args = (ptr(a.inp("pred", pred)), ptr(a.inp("gt", gt)), ptr(a.inp("group", group)), b, p, t_gt, i0, j, root, ng)
        ok(L.r50_op_pose_protocols(*args, ptr(a.inout("acc", torch.zeros(2 * ng * p + ng, dtype=F64))), stream()), "pose_protocols")
        ok(L.r50_op_pose_detail_metrics(*args, n_thr, dr.THR_MAX, ptr(a.inout("acc_detail", torch.zeros(dr.acc_size(ng, p, j), dtype=F64))), stream()),
            "pose_detail_metrics")
    _simple("evaluation", "pose_protocols-pose_detail_metrics-" + "-".join(str(v) for v in _case), ("r50_op_pose_protocols", "r50_op_pose_detail_metrics"),
            functools.partial(_detail_make, _case), _pp)


def _dtw_make(case):
    _plain, fitted, gt, group = _case_inputs(case)
    return torch.tensor(fitted), torch.tensor(gt), torch.tensor(group.tolist(), dtype=I32)


for _case in ((4, 5, 3, 3, 0, 17, 2, 0, 2), (5, 7, 7, 9, 2, 17, 4, 0, -1)):     # rows of tests/test_dtw_gpu.py's CASES
    def _dtw(a, pay, L, case=_case):
        b, p, q, t_gt, i0, j, ng, root, band = case
        pred, gt, group = pay
        clip_out = a.out("clip_out", (b, 2, 2 + 3 * p), F64)
        path_out = a.out("path_out", (b, 2, p + q - 1, 2), I32, defined=False)       # -1 past L is the op's own value, and the 0xFF pattern
        ok(L.r50_op_dtw_protocols(ptr(a.inp("pred", pred)), ptr(a.inp("gt", gt)), ptr(a.inp("group", group)), b, p, t_gt, i0, q, j, root, band, ng,
                                   ptr(clip_out), ptr(path_out), ptr(a.inout("acc", torch.zeros(ng * 2 * (1 + 2 * p) + ng, dtype=F64))), stream()),
            "dtw_protocols")
    _simple("evaluation", "dtw_protocols-" + "-".join(str(v) for v in _case), "r50_op_dtw_protocols", functools.partial(_dtw_make, _case), _dtw,
            reach=lambda pay: max(INDEXED(pay), 64 * 64 * 8))        # and one 64 x 64 fp64 cost matrix, the op's LDS limit


def _stitch_make():
    from tests import stitch_reference as ref
    clips = _stitch_clips()
    table = ref.table(clips, T)
    pred, gt = _poses(clips, 17, 27)
    return (torch.from_numpy(pred), torch.from_numpy(gt), torch.as_tensor(table["offsets"], dtype=I32), torch.as_tensor(table["src"], dtype=I32))


def _stitch(a, pay, L):
    pred, gt, offsets, src = pay
    n, t, j, _ = pred.shape
    frames = offsets.numel() - 1
    pd, gd, od, sd = a.inp("pred", pred), a.inp("gt", gt), a.inp("offsets", offsets), a.inp("src", src)
    for mode, ramp in ((0, 1), (1, 5), (2, 1)):
        outs = [a.out(f"{nm}[mode {mode}]", s, F32) for nm, s in (("fused", (frames, j, 3)), ("gt_out", (frames, j, 3)), ("spread", (frames,)),
                                                                  ("gt_gap", (frames,)))]
        ok(L.r50_op_stitch_poses(ptr(pd), ptr(gd), n * t, j, ptr(od), ptr(sd), frames, t, mode, ramp, *(ptr(o) for o in outs), stream()), "stitch_poses")


_simple("evaluation", "stitch_poses-23clips_t8_j17", "r50_op_stitch_poses", _stitch_make, _stitch)


def _seq_make():
    case = _metric_case([1, 2, 3, 300, 1, 393], [0, 1, 3, 1, 3, 0], 17, seed=21, gap_in=(3, 140))
    return {k: torch.from_numpy(v) for k, v in case.items()}


def _seq(a, pay, L):
    d = {k: a.inp(k, v) for k, v in pay.items()}
    frames = pay["seq"].numel()
    for nb in (3, 7):
        part = a.out(f"part[{nb} blocks]", (nb * 4 * 8,), F64)
        ok(L.r50_op_sequence_metrics(ptr(d["fused"]), ptr(d["gt"]), ptr(d["spread"]), ptr(d["offsets"]), ptr(d["seq"]), ptr(d["idx"]), ptr(d["group"]),
                                      frames, 17, 0, 4, ptr(part), nb, stream()), "sequence_metrics")


_simple("evaluation", "sequence_metrics-f700_g4", "r50_op_sequence_metrics", _seq_make, _seq)


GATHER = (7, 2048, 2731, 3)              # src_rows, c, b, t of test_gather_window_rows_stride_loop_runs_more_than_once


def _gather_make(et):
    rows, c, b, t = GATHER
    g = _gen(5)
    src = _cast_source(ET[et], rows, c, g)
    starts = torch.randint(0, 5, (b,), generator=g, dtype=I32)
    starts[0], starts[-1] = 4, 0                          # 4 + 3 == 7: that window's last row is the last row of src
    return src, starts


def _merge_make():
    from implementation_phd_lab_vision_amd import predict
    g = _gen(17)
    return torch.randn(5, 17, 3, generator=g), torch.randn(5, 17, 3, generator=g), torch.from_numpy(predict.flip_perm(17)).to(I32)


def _merge(a, pay, L):
    x, y, perm = pay
    ok(L.r50_op_merge_mirrored_poses(ptr(a.inp("a", x)), ptr(a.inp("b_mirrored", y)), 5, 17, ptr(a.inp("perm", perm)), ptr(a.out("out", (5, 17, 3), F32)),
                                      stream()), "merge_mirrored_poses")


_simple("evaluation", "merge_mirrored_poses-rows5j17", "r50_op_merge_mirrored_poses", _merge_make, _merge)

for _et in (1, 0):
    _nm = "fp16" if _et else "bf16"

    def _gather(a, pay, L, et=_et):
        src, starts = pay
        rows, c, b, t = GATHER
        ok(L.r50_op_gather_window_rows(ptr(a.inp("src", src)), rows, c, ptr(a.inp("starts", starts)), b, t, ptr(a.out("dst", (b * t, c), ET[et])), et, stream()),
            "gather_window_rows")

    def _gather_check(plain, pay, et=_et):
        """tests/test_predict_gpu.py's statement: the bits of r50_op_cast_rows on the gathered fp32 rows."""
        src, starts = pay
        rows, c, b, t = GATHER
        idx = (starts.long()[:, None] + torch.arange(t)[None]).reshape(-1)
        picked = src[idx].contiguous().to(DEV)
        want = torch.empty((b * t, c), dtype=ET[et], device=DEV)
        ok(lib().r50_op_cast_rows(ptr(picked), b * t, c, ptr(want), c, et, stream()), "cast_rows")
        assert torch.equal(G.bits(plain.results["dst"]), G.bits(want)), "dst is not r50_op_cast_rows' bits on the gathered rows"
    _simple("evaluation", f"gather_window_rows-{_nm}-last_window_ends_at_src_rows", "r50_op_gather_window_rows", functools.partial(_gather_make, _et),
            _gather, check=_gather_check)

    for _n, _nq, _k in ((1000, 48, 4), (1, 17, 1)):          # rows of test_search_values_against_the_oracle / test_search_shapes
        if _n == 1000 and _et == 0:
            continue

        def _nn_make(et=_et, n=_n, nq=_nq):
            from tests import baselines_reference as br
            return br.rows16((nq, 64), 1, "fp16" if et else "bf16"), br.rows16((n, 64), 0, "fp16" if et else "bf16")

        def _nn(a, pay, L, et=_et, n=_n, nq=_nq, k=_k):
            q, x = pay
            d = 64
            qd, xd = a.inp("q", q), a.inp("x", x)
            xn = a.out("x_norm2", (n,), F32)
            ok(L.r50_op_row_norm2(ptr(xd), n, d, et, ptr(xn), stream()), "row_norm2")
            nbytes = int(L.r50_op_nn_search_workspace(nq, n, k))
            assert nbytes > 0, f"r50_op_nn_search_workspace({nq}, {n}, {k}) gave {nbytes}"
            ws = a.ws("workspace", (nbytes,), U8)
            ok(L.r50_op_nn_search(ptr(qd), nq, ptr(xd), n, d, et, ptr(xn), k, ptr(a.out("idx_out", (nq, k), I32)), ptr(a.out("dist2_out", (nq, k), F32)),
                                   ptr(ws), nbytes, stream()), "nn_search")
        _simple("evaluation", f"row_norm2-nn_search-{_nm}-d64_n{_n}_nq{_nq}_k{_k}", ("r50_op_row_norm2", "r50_op_nn_search"), _nn_make, _nn,
                reach=max(32 * 64 * 2, 256 * 64 * 2, 4 * 1000))    # one staged chunk of 32 database rows; one block of 256 queries; x_norm2


def _base_make():
    from tests import baselines_reference as br
    b, k, j, n_db, t_db = 5, 3, 17, 9, 30
    return (br.grid_poses((b, j, 3), 1 + b), br.grid_poses((b, j, 3), 2 + j), torch.randint(0, n_db, (b, k), generator=_gen(25 + k), dtype=I32),
            br.grid_poses((n_db, t_db, j, 3), 3 + k))


def _base(a, pay, L):
    a1, a0, nn_row, dbj = pay
    b, k, n_db, t_db, j, il, pl = 5, 3, 9, 30, 17, 3, 25
    outs = [a.out(nm, (b, pl, j, 3), F32) for nm in ("const_pose", "const_vel", "nn")]
    ok(L.r50_op_baseline_forecasts(ptr(a.inp("a1", a1)), ptr(a.inp("a0", a0)), ptr(a.inp("nn_row", nn_row)), ptr(a.inp("dbj", dbj)), n_db, b, k, t_db, j, 2,
                                    il, pl, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream()), "baseline_forecasts")


_simple("evaluation", "baseline_forecasts-b5k3j17p25", "r50_op_baseline_forecasts", _base_make, _base)
