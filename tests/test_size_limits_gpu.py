"""Every backbone op exactly at the size limit include/r50.h states for it, and one image (or pixel) beyond -- the cases of
tests/size_limits.py on an MI355X.

At the limit (``n = n_max``): the operands are drawn on the device (``G.guarded_random``, seeded, no period) between two ``G.BAND`` bands,
once per fill; one launch through the raw entry point; then

  * the bands of every operand are intact and no output element still holds the fill;
  * WINDOWS of the result -- the first two units, the units on either side of byte offset 2^30 (and 2^32 where the operand reaches it) of
    the largest operand, and the last units, enough of them to hold the final ragged tile -- are held to the op's own reference at the op's
    own bar (the oracle and ``_check_bf16`` / ``_check_fp16`` / ``_check_fp32x`` / the fp8 and two-source bars of tests/test_kernels_gpu.py,
    ``torch.equal`` for the max pool; the fused bottleneck kernels through their own runners of tests/test_kernels_gpu.py, which hold a
    launch on the window's operands to the oracle and to the unfused launches, and whose output the window must then equal bit for
    bit).  A unit is an image, or a pixel row of r50_op_bneck_tail.  Every window is a slice of the big operands, copied to the host;
  * everything BETWEEN the windows: the same op with the same tile id on the parts of the batch (two halves; the stem four quarters, its
    output being too large for a half-size scratch under the memory cap), each a view into the same operands, into a scratch output;
    the big run must equal the parts bit for bit, compared on the device.  Rows with tile id 0 whose tile depends on the batch
    (r50_op_conv2d, r50_op_conv1x1_cat) are held to their windows only.

One step beyond (``n = n_max + 1``): the operands really allocated at that size, the call must return R50_ERR_INVALID, name the op, the
quantity and the bound, leave the stream idle and the pattern in the outputs untouched.  Nothing is ever launched on storage smaller than
what the call describes.  No test holds more than 8 GiB of device memory (asserted on the allocator's peak, counted from what the process held when the test began).
"""
import time

import pytest
import torch

from tests import guard_bands as G
from tests import size_limits as S

pytestmark = pytest.mark.gpu

BF, HF, F32, U8 = torch.bfloat16, torch.float16, torch.float32, torch.uint8
FP8 = torch.float8_e4m3fn
DEV = G.DEV
SEED = 20240611
FP8_SCALES = (0.05, 0.002, 0.04, 0.03)          # sx, sw, sr, sy of tests/test_kernels_gpu.py's fp8 cases
CMP_CHUNK = 1 << 26
QUANTITY = {"x": "x bytes", "x_back": "x bytes", "y": "y bytes", "x2": "x2 bytes", "out": "out bytes", "M": "pixels"}


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality of two contiguous device tensors, a chunk at a time (no temporary of the operands' size)."""
    assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
    fa, fb = a.view(-1).view(U8), b.view(-1).view(U8)
    for i in range(0, fa.numel(), 2 * CMP_CHUNK):
        if not torch.equal(fa[i: i + 2 * CMP_CHUNK], fb[i: i + 2 * CMP_CHUNK]):
            return False
    return True


def _count_fill(t: torch.Tensor, fill: int) -> int:
    flat = t.view(-1)
    return sum(G.holds_fill(flat[i: i + CMP_CHUNK], fill) for i in range(0, flat.numel(), CMP_CHUNK))


def _windows(n: int, unit_bytes: int, width: int, tail: int):
    """[a, b) unit ranges: the first `width`; the unit that holds byte offset 2^30 (and 2^32, where the operand reaches it) of the largest
    operand with its neighbours on either side (for pixel rows: `width` rows around it); the last `tail`.  Overlapping ranges are merged."""
    out = [(0, min(width, n)), (max(0, n - tail), n)]
    for off in (1 << 30, 1 << 32):
        k = off // unit_bytes
        lo, hi = k - max(1, width // 2), k + max(2, width // 2)
        if lo > width and hi < n - tail:
            out.append((lo, hi))
    out = sorted(set(out))
    merged = [out[0]]
    for a, b in out[1:]:
        if a <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(b, merged[-1][1]))
        else:
            merged.append((a, b))
    return merged


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _rows_nchw(t):
    """(R, C) pixel rows -> the (1, C, R, 1) NCHW tensor the tail runners of tests/test_kernels_gpu.py take."""
    return t.view(1, t.shape[0], 1, t.shape[1]).permute(0, 3, 1, 2).contiguous()


def _host_gen(case):
    return torch.Generator().manual_seed(SEED + sum(ord(c) for c in case.id))


def _rand(shape, g, scale=1.0):
    return torch.randn(shape, generator=g) * scale


class Family:
    """One runner: which operands a case has, how the raw entry point is called on (views of) them, and what a window is held to."""
    width = 2                   # units per window
    parts = 2                   # the batch is re-run in this many parts

    def tail(self, case):       # units in the last window: two images, or enough to hold a 256-pixel tile
        return 2

    def weights(self, case):    # name -> host tensor as the device receives it, plus whatever the reference needs under other names
        raise NotImplementedError

    def device_weights(self, case, hw):   # the names of `weights` that travel to the device
        raise NotImplementedError

    def inputs(self, case):     # name -> (per-unit shape, dtype, scale, limit)
        raise NotImplementedError

    def outputs(self, case):    # name -> (per-unit shape, dtype)
        raise NotImplementedError

    def workspace(self, case, n):
        return {}

    def post_generate(self, case, I, gen):
        pass

    def compares_parts(self, case):
        return True

    def call(self, case, n, I, W, O, ws):
        raise NotImplementedError

    def reference(self, case, Iw, hw):
        """Whatever `check` needs that depends on the window's inputs alone: computed once per window, shared by both fills."""
        raise NotImplementedError

    def check(self, case, ref, Ow, what):
        raise NotImplementedError


# ---- convolutions -------------------------------------------------------------------------------------------------------------------
class Conv(Family):
    def _p(self, case):
        h, w, cin, cout, k, stride, pad, relu, res = case.shape
        ho, wo = S.out_hw(h, w, k, stride, pad)
        return h, w, cin, cout, k, stride, pad, relu, res, ho, wo

    def tail(self, case):
        *_, ho, wo = self._p(case)
        return max(2, -(-256 // (ho * wo)) + 1)

    def _et(self, case):
        return {"r50_op_conv2d_f16": HF, "r50_op_conv2d_fp8": FP8}.get(case.op, BF)

    def weights(self, case):
        from tests import pair_reference as P
        h, w, cin, cout, k, stride, pad, relu, res, ho, wo = self._p(case)
        g = _host_gen(case)
        bias = _rand(cout, g, 0.1)
        if case.op == "r50_op_conv2d_fp8":
            sx, sw, sr, sy = FP8_SCALES
            wq = (_rand((cout, k, k, cin), g, (1.0 / (k * k * cin)) ** 0.5 / sw)).clamp(-448, 448).to(FP8)
            return {"w": wq, "bias": (bias / (sx * sw)).contiguous(), "bias_real": bias}
        wt = _rand((cout, cin, k, k), g, (2.0 / (cin * k * k)) ** 0.5)
        if case.op == "r50_op_conv2d_w2":
            return {"w": P.pack_ohwi_w2(wt), "bias": bias, "wt": wt}
        if case.op == "r50_op_conv2d_split":
            return {"w": P.pack_ohwi_split(wt), "bias": bias, "wt": wt}
        wq = wt.to(self._et(case))
        return {"w": wq.permute(0, 2, 3, 1).contiguous(), "bias": bias, "wt": wq.float()}

    def device_weights(self, case, hw):
        return ("w", "bias")

    def inputs(self, case):
        h, w, cin, cout, k, stride, pad, relu, res, ho, wo = self._p(case)
        et = self._et(case)
        mul = 2 if case.op == "r50_op_conv2d_split" else 1
        scale, limit = (0.5 / FP8_SCALES[0], 448.0) if et == FP8 else (1.0, None)
        d = {"x": ((h, w, mul * cin), et, scale, limit)}
        if res:
            d["res"] = ((ho, wo, mul * cout), et, (0.5 / FP8_SCALES[2]) if et == FP8 else 1.0, limit)
        return d

    def outputs(self, case):
        h, w, cin, cout, k, stride, pad, relu, res, ho, wo = self._p(case)
        return {"y": ((ho, wo, (2 if case.op == "r50_op_conv2d_split" else 1) * cout), self._et(case))}

    def post_generate(self, case, I, gen):
        """fp32x operands are (head, tail) pairs: the tail planes become at most half a bf16 step of their heads."""
        if case.op != "r50_op_conv2d_split":
            return
        for t in I.values():
            c = t.shape[-1] // 2
            step = max(1, G.RANDOM_CHUNK // (t[0].numel()))
            for i in range(0, t.shape[0], step):
                blk = t[i: i + step]
                u = torch.rand(blk[..., :c].shape, generator=gen, device=t.device, dtype=F32) * 2 - 1
                blk[..., c:] = (blk[..., :c].float() * u * 2.0 ** -9).to(BF)

    def compares_parts(self, case):
        return not (case.tile == 0 and case.op == "r50_op_conv2d")       # the automatic tile depends on the batch

    def call(self, case, n, I, W, O, ws):
        h, w, cin, cout, k, stride, pad, relu, res, ho, wo = self._p(case)
        L, s = G.lib(), G.stream()
        head = (I["x"].data_ptr(), n, h, w, cin, W["w"].data_ptr(), W["bias"].data_ptr(), G.ptr(I.get("res")), O["y"].data_ptr(), cout, k,
                stride, pad, int(relu))
        if case.op == "r50_op_conv2d_split":
            return L.r50_op_conv2d_split(*head, s)
        if case.op == "r50_op_conv2d_fp8":
            sx, sw, sr, sy = FP8_SCALES
            return L.r50_op_conv2d_fp8(*head, float(sx * sw / sy), float(sr / sy), case.tile, s)
        return getattr(L, case.op)(*head, case.tile, s)

    def reference(self, case, Iw, hw):
        from oracle.resnet50_oracle import conv_bias_act_emulated
        from tests import pair_reference as P
        from tests.kernel_cases import fp8_reference
        h, w, cin, cout, k, stride, pad, relu, res, ho, wo = self._p(case)
        x, r = Iw["x"], Iw.get("res")
        if case.op == "r50_op_conv2d_fp8":
            return fp8_reference(x, hw["w"], hw["bias_real"], r, FP8_SCALES, stride, pad, relu).clamp(-448, 448).float().to(FP8).float()
        if case.op == "r50_op_conv2d_split":
            pair = lambda t: tuple(_nchw(p) for p in (t[..., :t.shape[-1] // 2], t[..., t.shape[-1] // 2:]))     # noqa: E731
            return P.fp32x_conv(pair(x), P.split_pair(hw["wt"]), hw["bias"], stride, pad, relu, pair(r) if res else None)
        return conv_bias_act_emulated(_nchw(x).float(), hw["wt"], hw["bias"], stride, pad, relu,
                                      residual_bf=_nchw(r).float() if res else None,
                                      weight_terms=2 if case.op == "r50_op_conv2d_w2" else 1,
                                      fmt="fp16" if case.op == "r50_op_conv2d_f16" else "bf16")

    def check(self, case, ref, Ow, what):
        from tests.test_kernels_gpu import _check_bf16, _check_fp16
        y = Ow["y"]
        if case.op == "r50_op_conv2d_fp8":            # the bar of tests/test_kernels_gpu.py::_run_conv2d_fp8
            got = _nchw(y.float().cpu())
            assert torch.isfinite(got).all(), what
            diff = (got - ref).abs()
            assert not (diff > ref.abs() * 0.126 + 2.0 ** -9 + 1e-7).any(), f"{what}: {float(diff.max())}"
            assert float((diff > 0).float().mean()) < 0.02, f"{what}: {float((diff > 0).float().mean())}"
            assert float(got.abs().max()) > 1.0, what
        elif case.op == "r50_op_conv2d_split":
            from tests.test_pair_modes_gpu import _check_fp32x
            _check_fp32x(y, ref, what)
        elif case.op == "r50_op_conv2d_f16":
            _check_fp16(y, ref, what)
        else:
            _check_bf16(y, ref, what)


class Cat(Family):
    def tail(self, case):
        return -(-256 // (case.shape[0] ** 2)) + 1

    def weights(self, case):
        h, c1, h2, c2, s2, cout = case.shape
        g = _host_gen(case)
        return {"wcat": _rand((cout, c1 + c2), g, (1.0 / (c1 + c2)) ** 0.5).to(BF), "bias": _rand(cout, g, 0.1)}

    def device_weights(self, case, hw):
        return ("wcat", "bias")

    def inputs(self, case):
        h, c1, h2, c2, s2, cout = case.shape
        return {"x1": ((h, h, c1), BF, 1.0, None), "x2": ((h2, h2, c2), BF, 1.0, None)}

    def outputs(self, case):
        h, c1, h2, c2, s2, cout = case.shape
        return {"y": ((h, h, cout), BF)}

    def compares_parts(self, case):
        return case.tile != 0

    def call(self, case, n, I, W, O, ws):
        h, c1, h2, c2, s2, cout = case.shape
        return G.lib().r50_op_conv1x1_cat(I["x1"].data_ptr(), n, h, h, c1, I["x2"].data_ptr(), h2, h2, c2, s2, W["wcat"].data_ptr(),
                                          W["bias"].data_ptr(), O["y"].data_ptr(), cout, 1, case.tile, 0, G.stream())

    def reference(self, case, Iw, hw):
        import torch.nn.functional as F
        h, c1, h2, c2, s2, cout = case.shape
        wcat = hw["wcat"]
        ref = F.conv2d(_nchw(Iw["x1"].double()), wcat[:, :c1].double().view(cout, c1, 1, 1))
        ref = ref + F.conv2d(_nchw(Iw["x2"].double()), wcat[:, c1:].double().view(cout, c2, 1, 1), stride=s2)
        return F.relu(ref + hw["bias"].double().view(1, -1, 1, 1)).float().to(BF).float()

    def check(self, case, ref, Ow, what):            # the bar of tests/test_kernels_gpu.py::_run_conv1x1_cat
        got = _nchw(Ow["y"].float().cpu())
        diff = (got - ref).abs()
        ulp = ref.abs() * 2.0 ** -7 + 2.0 ** -16 * max(1.0, float(ref.abs().max()))
        assert not (diff > ulp).any(), f"{what}: {float(diff.max())}"
        assert float((diff > 0).float().mean()) < 0.01, what


# ---- the fused bottleneck kernels: held to their own runners of tests/test_kernels_gpu.py --------------------------------------------
class Fused(Family):
    """`reference` runs the family's runner on the window's operands (it asserts the oracle's bar and the equality with the unfused
    launches) and keeps its outputs; `check` asks the big run's window for the same bits."""

    def check(self, case, ref, Ow, what):
        assert len(ref) == len(Ow), f"{what}: the runner returned {len(ref)} outputs for {list(Ow)}"
        for (name, t), r in zip(Ow.items(), ref):
            assert r is not None and _bits_equal(t.contiguous().view(-1), r.contiguous().view(-1)), \
                f"{what}: `{name}` of the run at the limit differs from the same window run on its own"


class Tail(Fused):
    width = 128

    def tail(self, case):
        return 256

    def weights(self, case):
        cmid, c1, ds = case.shape
        g = _host_gen(case)
        d = {"w3": _rand((4 * cmid, cmid, 1, 1), g, (2.0 / cmid) ** 0.5).to(BF), "b3": _rand(4 * cmid, g, 0.1)}
        cw = c1 or 256
        d["w1"] = _rand((cw, 4 * cmid, 1, 1), g, (2.0 / (4 * cmid)) ** 0.5).to(BF)
        d["b1"] = _rand(cw, g, 0.1)
        if ds:
            d["wd"] = _rand((4 * cmid, cmid, 1, 1), g, (1.0 / cmid) ** 0.5).to(BF)
            d["bd"] = _rand(4 * cmid, g, 0.1)
        return d

    def device_weights(self, case, hw):
        cmid, c1, ds = case.shape
        return tuple(k for k in hw if c1 or k not in ("w1", "b1"))

    def inputs(self, case):
        cmid, c1, ds = case.shape
        return {"y2": ((cmid,), BF, 1.0, None), "idn": ((cmid if ds else 4 * cmid,), BF, 1.0, None)}

    def outputs(self, case):
        cmid, c1, ds = case.shape
        d = {"out": ((4 * cmid,), BF)}
        if c1:
            d["y1n"] = ((c1,), BF)
        return d

    def call(self, case, m, I, W, O, ws):
        cmid, c1, ds = case.shape
        return G.lib().r50_op_bneck_tail(I["y2"].data_ptr(), m, cmid, W["w3"].data_ptr(), W["b3"].data_ptr(), I["idn"].data_ptr(),
                                         G.ptr(W.get("wd")), G.ptr(W.get("bd")), O["out"].data_ptr(), G.ptr(W.get("w1")), c1,
                                         G.ptr(W.get("b1")), G.ptr(O.get("y1n")), G.stream())

    def reference(self, case, Iw, hw):
        from tests import test_kernels_gpu as K
        cmid, c1, ds = case.shape
        y2, idn = _rows_nchw(Iw["y2"]), _rows_nchw(Iw["idn"])
        shape = (1, y2.shape[2], 1)
        if cmid == 64:
            rest = (idn, hw["wd"], hw["bd"]) if ds else (idn,)
            return K._run_bneck_tail(shape, c1, ds, tensors=(y2, hw["w3"], hw["b3"], hw["w1"], hw["b1"]) + rest)
        if cmid == 128:
            return K._run_bneck_tail_layer2(shape, tensors=(y2, hw["w3"], hw["b3"], idn, hw["w1"], hw["b1"]))
        if c1:
            return K._run_bneck_tail_layer3(shape, 0, tensors=(y2, hw["w3"], hw["b3"], idn, hw["w1"], hw["b1"]))
        return (K._run_layer3_last_block(1, tensors=(y2, hw["w3"], hw["b3"], idn, None, None)),)


class Block1(Fused):
    def weights(self, case):
        c1, ds = case.shape
        g = _host_gen(case)
        d = {"w2": _rand((64, 3, 3, 64), g, (2.0 / 576) ** 0.5).to(BF), "w3": _rand((256, 1, 1, 64), g, (2.0 / 64) ** 0.5).to(BF),
             "w1": _rand((c1, 1, 1, 256), g, (2.0 / 256) ** 0.5).to(BF), "b2": _rand(64, g, 0.1), "b3": _rand(256, g, 0.1),
             "b1": _rand(c1, g, 0.1)}
        if ds:
            d["wd"] = _rand((256, 1, 1, 64), g, (1.0 / 64) ** 0.5).to(BF)
            d["bd"] = _rand(256, g, 0.1)
        return d

    def device_weights(self, case, hw):
        return tuple(hw)

    def inputs(self, case):
        c1, ds = case.shape
        return {"t1": ((56, 56, 64), BF, 1.0, None), "idn": ((56, 56, 64 if ds else 256), BF, 1.0, None)}

    def outputs(self, case):
        c1, ds = case.shape
        return {"out": ((56, 56, 256), BF), "y1n": ((56, 56, c1), BF)}

    def call(self, case, n, I, W, O, ws):
        c1, ds = case.shape
        L, s = G.lib(), G.stream()
        p = {k: v.data_ptr() for k, v in W.items()}
        if ds:
            return L.r50_op_bneck_block1_ds(I["t1"].data_ptr(), n, p["w2"], p["b2"], p["w3"], p["b3"], I["idn"].data_ptr(), p["wd"], p["bd"],
                                            O["out"].data_ptr(), p["w1"], p["b1"], O["y1n"].data_ptr(), s)
        return L.r50_op_bneck_block1(I["t1"].data_ptr(), n, p["w2"], p["b2"], p["w3"], p["b3"], I["idn"].data_ptr(), O["out"].data_ptr(),
                                     p["w1"], c1, p["b1"], O["y1n"].data_ptr(), s)

    def reference(self, case, Iw, hw):
        from tests import test_kernels_gpu as K
        c1, ds = case.shape
        n = Iw["t1"].shape[0]
        if ds:
            return K._run_bneck_block1_ds(n, tensors=(Iw["t1"], Iw["idn"], hw["w2"], hw["w3"], hw["wd"], hw["w1"], hw["b2"], hw["b3"],
                                                      hw["bd"], hw["b1"]))
        return K._run_bneck_block1(n, c1, tensors=(Iw["t1"], Iw["idn"], hw["w2"], hw["w3"], hw["w1"], hw["b2"], hw["b3"], hw["b1"]))


class Block2(Fused):
    def weights(self, case):
        g = _host_gen(case)
        return {"w2": _rand((128, 3, 3, 128), g, (2.0 / 1152) ** 0.5).to(BF), "w3": _rand((512, 1, 1, 128), g, (2.0 / 128) ** 0.5).to(BF),
                "w1": _rand((128, 1, 1, 512), g, (2.0 / 512) ** 0.5).to(BF), "b2": _rand(128, g, 0.1), "b3": _rand(512, g, 0.1),
                "b1": _rand(128, g, 0.1)}

    def device_weights(self, case, hw):
        return tuple(hw)

    def inputs(self, case):
        return {"t1": ((28, 28, 128), BF, 1.0, None), "idn": ((28, 28, 512), BF, 1.0, None)}

    def outputs(self, case):
        return {"out": ((28, 28, 512), BF), "y1n": ((28, 28, 128), BF)}

    def call(self, case, n, I, W, O, ws):
        p = {k: v.data_ptr() for k, v in W.items()}
        return G.lib().r50_op_bneck_block2(I["t1"].data_ptr(), n, p["w2"], p["b2"], p["w3"], p["b3"], I["idn"].data_ptr(), O["out"].data_ptr(),
                                           p["w1"], p["b1"], O["y1n"].data_ptr(), G.stream())

    def reference(self, case, Iw, hw):
        from tests import test_kernels_gpu as K
        return K._run_bneck_block2(Iw["t1"].shape[0], True, tensors=(Iw["t1"], Iw["idn"], hw["w2"], hw["w3"], hw["w1"], hw["b2"], hw["b3"],
                                                                  hw["b1"]))


class CatChain(Fused):
    width = 3                   # three images per window: the runner holds up to three to the oracle as well

    def tail(self, case):
        return 3

    def weights(self, case):
        g = _host_gen(case)
        w3 = _rand((512, 128, 1, 1), g, (1.0 / 128) ** 0.5).to(BF)
        wd = _rand((512, 256, 1, 1), g, (1.0 / 256) ** 0.5).to(BF)
        w1 = _rand((128, 512, 1, 1), g, (2.0 / 512) ** 0.5).to(BF)
        return {"wcat": torch.cat([w3.view(512, 128), wd.view(512, 256)], dim=1).contiguous(), "bcat": _rand(512, g, 0.1),
                "w1": w1.view(128, 512).contiguous(), "b1": _rand(128, g, 0.1), "w3_oihw": w3, "wd_oihw": wd, "w1_oihw": w1}

    def device_weights(self, case, hw):
        return ("wcat", "bcat", "w1", "b1")

    def inputs(self, case):
        return {"t2": ((28, 28, 128), BF, 1.0, None), "x": ((56, 56, 256), BF, 1.0, None)}

    def outputs(self, case):
        return {"out": ((28, 28, 512), BF), "y1n": ((28, 28, 128), BF)}

    def call(self, case, n, I, W, O, ws):
        return G.lib().r50_op_bneck_cat_chain(I["t2"].data_ptr(), I["x"].data_ptr(), n, 28, W["wcat"].data_ptr(), W["bcat"].data_ptr(),
                                              O["out"].data_ptr(), W["w1"].data_ptr(), W["b1"].data_ptr(), O["y1n"].data_ptr(), G.stream())

    def reference(self, case, Iw, hw):
        from tests import test_kernels_gpu as K
        n = Iw["t2"].shape[0]
        assert n <= 3
        return K._run_bneck_cat_chain(n, tensors=(_nchw(Iw["t2"]), _nchw(Iw["x"]), hw["w3_oihw"], hw["wd_oihw"], hw["bcat"], hw["w1_oihw"],
                                                  hw["b1"]))


# ---- the stem and the pools ------------------------------------------------------------------------------------------------------------
class MaxPool(Family):
    def weights(self, case):
        return {}

    def device_weights(self, case, hw):
        return ()

    def inputs(self, case):
        return {"x": (case.shape, BF, 1.0, None)}

    def outputs(self, case):
        h, w, c = case.shape
        return {"y": (((h - 1) // 2 + 1, (w - 1) // 2 + 1, c), BF)}

    def call(self, case, n, I, W, O, ws):
        h, w, c = case.shape
        return G.lib().r50_op_maxpool(I["x"].data_ptr(), n, h, w, c, O["y"].data_ptr(), G.stream())

    def reference(self, case, Iw, hw):
        import torch.nn.functional as F
        return F.max_pool2d(_nchw(Iw["x"].float()), 3, 2, 1).permute(0, 2, 3, 1).contiguous()

    def check(self, case, ref, Ow, what):
        assert torch.equal(Ow["y"].float().cpu(), ref), what


class AvgPool(Family):
    def weights(self, case):
        return {}

    def device_weights(self, case, hw):
        return ()

    def inputs(self, case):
        return {"x": (case.shape, BF, 1.0, None)}

    def outputs(self, case):
        return {"y": ((case.shape[1],), F32)}

    def call(self, case, n, I, W, O, ws):
        hw_, c = case.shape
        return G.lib().r50_op_avgpool(I["x"].data_ptr(), n, hw_, c, O["y"].data_ptr(), G.stream())

    def reference(self, case, Iw, hw):
        return Iw["x"].double().mean(dim=1)

    def check(self, case, ref, Ow, what):
        y = Ow["y"].cpu().double()
        assert torch.allclose(y, ref, rtol=1e-5, atol=1e-6), f"{what}: {float((y - ref).abs().max())}"


class Stem(Family):
    parts = 4                   # a half-size scratch for y would put the case over the memory cap

    def weights(self, case):
        from implementation_phd_lab_vision_amd.weights import synthetic_state_dict
        from oracle.resnet50_oracle import folded
        wf, bf = folded(synthetic_state_dict(0), "conv1", "bn1")
        self._w_host = wf.contiguous()              # a HOST operand of the entry point: kept alive here for `call`
        return {"w_host": self._w_host, "bias": bf}

    def device_weights(self, case, hw):
        return ("bias",)

    def inputs(self, case):
        return {"x": ((3, 224, 224), F32, 1.0, None)}

    def outputs(self, case):
        return {"y": ((112, 112, 64), BF)}

    def workspace(self, case, n):
        return {"scratch": ((int(G.lib().r50_stem_scratch_bytes(n)),), U8)}

    def call(self, case, n, I, W, O, ws):
        return G.lib().r50_op_stem(I["x"].data_ptr(), n, self._w_host.data_ptr(), W["bias"].data_ptr(), ws["scratch"].data_ptr(),
                                   O["y"].data_ptr(), G.stream())

    def reference(self, case, Iw, hw):
        from oracle.resnet50_oracle import bf16_round, conv_bias_act_emulated
        return conv_bias_act_emulated(bf16_round(Iw["x"]), hw["w_host"], hw["bias"], 2, 3, True)

    def check(self, case, ref, Ow, what):
        from tests.test_kernels_gpu import _check_bf16
        _check_bf16(Ow["y"], ref, what)


FAMILIES = {"conv": Conv(), "cat": Cat(), "tail": Tail(), "block1": Block1(), "block2": Block2(), "cat_chain": CatChain(),
            "maxpool": MaxPool(), "avgpool": AvgPool(), "stem": Stem()}


# ---- the two tests -----------------------------------------------------------------------------------------------------------------
def _unit_bytes(spec):
    def nb(shape, dtype):
        numel = 1
        for v in shape:
            numel *= v
        return numel * torch.empty((), dtype=dtype).element_size()
    return max(nb(s[0], s[1]) for s in spec.values())


def _free():
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _start_of_memory_count() -> int:
    """Frees what can be freed and restarts the allocator's peak count.  Returns the bytes that are still allocated: tensors that earlier
    tests of the process keep alive (cached cases, session fixtures).  They are not this test's: what a test holds at once is the peak
    from here on minus this figure."""
    _free()
    torch.cuda.reset_peak_memory_stats()
    return torch.cuda.memory_allocated()


def _place_weights(fam, case, hw, fill):
    return {k: G.guarded(hw[k], fill, device=DEV) for k in fam.device_weights(case, hw)}


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    monkeypatch.delenv("R50_OP_ET", raising=False)
    monkeypatch.delenv("R50_TAIL3_BP", raising=False)
    yield
    _free()


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_at_the_limit(lib_built, case):
    fam = FAMILIES[case.family]
    n = case.n_at
    assert S.rule(case.terms(), n)
    held_before = _start_of_memory_count()
    t0 = time.perf_counter()
    hw = fam.weights(case)
    in_spec, out_spec = fam.inputs(case), fam.outputs(case)
    wins = _windows(n, max(_unit_bytes(in_spec), _unit_bytes(out_spec)), fam.width, fam.tail(case))
    refs = {}
    for fill in G.FILLS:
        _run_under_fill(case, fam, n, fill, hw, in_spec, out_spec, wins, refs)     # in a frame of its own: nothing of it outlives the call
        _free()
    peak = torch.cuda.max_memory_allocated() - held_before
    print(f"{case.id}: n {n}, {len(wins)} windows {wins}, {time.perf_counter() - t0:.1f} s, peak {peak / 2 ** 30:.2f} GiB "
          f"(beside {held_before / 2 ** 30:.2f} GiB that earlier tests of the process still hold)")
    assert peak <= S.MEMORY_CAP, f"{case.id}: the test held {peak} bytes of device memory at once"


def _run_under_fill(case, fam, n, fill, hw, in_spec, out_spec, wins, refs):
    what = f"{case.id} n {n} fill {fill:#x}"
    gen = torch.Generator(device=DEV).manual_seed(SEED)          # the same operands under both fills
    I = {k: G.guarded_random((n,) + tuple(shp), dt, fill, gen, scale, limit, device=DEV) for k, (shp, dt, scale, limit) in in_spec.items()}
    fam.post_generate(case, I, gen)
    W = _place_weights(fam, case, hw, fill)
    O = {k: G.guarded_empty((n,) + tuple(shp), dt, fill, device=DEV) for k, (shp, dt) in out_spec.items()}
    ws = {k: G.guarded_empty(shp, dt, fill, device=DEV) for k, (shp, dt) in fam.workspace(case, n).items()}
    operands = [(k, v) for d in (I, W, O, ws) for k, v in d.items()]
    torch.cuda.synchronize()
    G.ok(fam.call(case, n, I, W, O, ws), what)
    torch.cuda.synchronize()
    G.assert_bands_intact(operands, fill, what)
    for k, t in O.items():
        if G._checks_fill(t, fill):
            left = _count_fill(t, fill)
            assert left == 0, f"{what}: {left} of {t.numel()} elements of `{k}` still hold the fill pattern"
    for a, b in wins:
        if (a, b) not in refs:
            refs[(a, b)] = fam.reference(case, {k: v[a:b].cpu() for k, v in I.items()}, hw)
        fam.check(case, refs[(a, b)], {k: v[a:b] for k, v in O.items()}, f"{what} units [{a}, {b})")
    if fam.compares_parts(case):
        step = -(-n // fam.parts)
        Sc = {k: G.guarded_empty((step,) + tuple(shp), dt, fill, device=DEV) for k, (shp, dt) in out_spec.items()}
        for a in range(0, n, step):
            b = min(n, a + step)
            G.ok(fam.call(case, b - a, {k: v[a:b] for k, v in I.items()}, W, {k: v[:b - a] for k, v in Sc.items()}, ws), what)
            torch.cuda.synchronize()
            for k in O:
                assert _bits_equal(O[k][a:b], Sc[k][:b - a]), \
                    f"{what}: `{k}` of units [{a}, {b}) differs between the run at the limit and the run of that part alone"
        G.assert_bands_intact(list(Sc.items()) + operands, fill, what + " parts")


@pytest.mark.parametrize("case", [c for c in S.CASES if c.beyond], ids=lambda c: c.id)
def test_one_step_beyond_is_refused(lib_built, case):
    fam = FAMILIES[case.family]
    n = case.n_max + 1
    assert not S.rule(case.terms(), n)
    fill = G.FILL_BIG
    held_before = _start_of_memory_count()
    hw = fam.weights(case)
    # really allocated at the size the call describes, and filled: a library that fails to refuse computes on valid memory
    I = {k: G.guarded_empty((n,) + tuple(shp), dt, fill, device=DEV) for k, (shp, dt, _s, _l) in fam.inputs(case).items()}
    W = _place_weights(fam, case, hw, fill)
    O = {k: G.guarded_empty((n,) + tuple(shp), dt, fill, device=DEV) for k, (shp, dt) in fam.outputs(case).items()}
    ws = {k: G.guarded_empty(shp, dt, fill, device=DEV) for k, (shp, dt) in fam.workspace(case, n).items()}
    torch.cuda.synchronize()
    rc = fam.call(case, n, I, W, O, ws)
    idle = torch.cuda.current_stream().query()
    msg = G.lib().r50_last_error(None)
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    torch.cuda.synchronize()
    assert rc == -1, f"{case.id}: n_max + 1 = {n} returned {rc} ({msg})"
    assert idle, f"{case.id}: the refused call left work on the stream"
    assert case.op in msg and QUANTITY[case.limited_by] in msg and "2^31" in msg, f"{case.id}: the refusal reads `{msg}`"
    for k, t in O.items():
        assert _count_fill(t, fill) == t.numel(), f"{case.id}: the refused call wrote to `{k}`"
    G.assert_bands_intact([(k, v) for d in (I, W, O, ws) for k, v in d.items()], fill, case.id)
    assert torch.cuda.max_memory_allocated() - held_before <= S.MEMORY_CAP
    del I, W, O, ws
