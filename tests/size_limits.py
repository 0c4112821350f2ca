"""Size limits of the backbone ops -- the rules of include/r50.h ("Size limits:" in each entry point's comment) restated in Python integers, and
the case list of tests/test_size_limits_gpu.py.  Nothing here touches the device at import.

Every rule is a list of terms ``a * n + c < bound`` in the one argument that grows (the image count n, or the pixel count m of
r50_op_bneck_tail), written from the header's text, not from the launcher.  ``n_max`` is the closed form (the smallest over the terms of
``(bound - 1 - c) // a``); tests/test_size_limits_cpu.py evaluates the terms themselves at ``n_max`` and ``n_max + 1``.

A limit that lies above what fits the 8 GiB a test may hold (the stem and the two pools, whose kernels address in 64 bits) is marked
``limited_by = "cap"``: the case then runs at ``n_run``, the smallest n at which its largest 16-bit tensor crosses 2^31 elements and 2^32
bytes, and has no one-step-beyond form (its operands could not be allocated).
"""
from typing import Callable, List, NamedTuple, Optional, Tuple

P30, P31, P63 = 1 << 30, 1 << 31, 1 << 63
MEMORY_CAP = 8 << 30


class Term(NamedTuple):
    name: str           # the operand (or count) the term bounds: what `limited_by` names and what the refusal message must mention
    a: int              # per image (or pixel)
    c: int              # constant part
    bound: int          # exclusive

    def value(self, n: int) -> int:
        return self.a * n + self.c

    def holds(self, n: int) -> bool:
        return self.value(n) < self.bound

    def n_max(self) -> int:
        return (self.bound - 1 - self.c) // self.a


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


# ---- the rules, one function per entry point family; each quotes the header sentence it restates
def conv_terms(h, w, cin, cout, k, stride, pad, op="r50_op_conv2d") -> List[Term]:
    """r50_op_conv2d / _f16: n*ho*wo <= 2^30; n*h*w*cin*2 + (pad*w+pad)*cin*2 < 2^31; n*ho*wo*cout*2 < 2^31; cout*k*k*cin*2 < 2^31.
    _w2: the weight term is cout*k*k*2*cin*2.  _split: n*h*w*2*cin*2 + (pad*w+pad)*2*cin*2, n*ho*wo*2*cout*2, cout*k*k*3*cin*2.
    _fp8: n*h*w*cin + (pad*w+pad)*cin, n*ho*wo*cout*2, cout*k*k*cin."""
    ho, wo = out_hw(h, w, k, stride, pad)
    back = pad * w + pad
    if op in ("r50_op_conv2d", "r50_op_conv2d_f16"):
        x, xb, y, wt = h * w * cin * 2, back * cin * 2, ho * wo * cout * 2, cout * k * k * cin * 2
    elif op == "r50_op_conv2d_w2":
        x, xb, y, wt = h * w * cin * 2, back * cin * 2, ho * wo * cout * 2, cout * k * k * 2 * cin * 2
    elif op == "r50_op_conv2d_split":
        x, xb, y, wt = h * w * 2 * cin * 2, back * 2 * cin * 2, ho * wo * 2 * cout * 2, cout * k * k * 3 * cin * 2
    elif op == "r50_op_conv2d_fp8":
        x, xb, y, wt = h * w * cin, back * cin, ho * wo * cout * 2, cout * k * k * cin
    else:
        raise KeyError(op)
    assert wt < P31, "the weight term does not grow with n: a case must satisfy it"
    return [Term("M", ho * wo, 0, P30 + 1), Term("x", x, xb, P31), Term("y", y, 0, P31)]


def cat_terms(h, c1, h2, c2, cout) -> List[Term]:
    """r50_op_conv1x1_cat: n*h*w <= 2^30; n*h*w*c1*2 < 2^31; n*h2*w2*c2*2 < 2^31; n*h*w*cout*2 < 2^31; cout*(c1+c2)*2 < 2^31."""
    assert cout * (c1 + c2) * 2 < P31
    return [Term("M", h * h, 0, P30 + 1), Term("x", h * h * c1 * 2, 0, P31), Term("x2", h2 * h2 * c2 * 2, 0, P31),
            Term("y", h * h * cout * 2, 0, P31)]


def tail_terms(cmid) -> List[Term]:
    """r50_op_bneck_tail: m*4*cmid*2 < 2^31 (m*512, m*1024, m*2048 for cmid 64, 128, 256), in every form."""
    return [Term("out", 4 * cmid * 2, 0, P31)]


def block1_terms() -> List[Term]:
    """r50_op_bneck_block1 / _ds: n*56*56*256*2 < 2^31."""
    return [Term("out", 56 * 56 * 256 * 2, 0, P31)]


def block2_terms() -> List[Term]:
    """r50_op_bneck_block2: n*28*28*512*2 < 2^31."""
    return [Term("out", 28 * 28 * 512 * 2, 0, P31)]


def cat_chain_terms(ow=28) -> List[Term]:
    """r50_op_bneck_cat_chain: n*(2*ow)*(2*ow)*256*2 < 2^31 and n*ow*ow*512*2 < 2^31."""
    return [Term("x", (2 * ow) * (2 * ow) * 256 * 2, 0, P31), Term("out", ow * ow * 512 * 2, 0, P31)]


def stem_terms() -> List[Term]:
    """r50_op_stem: n*28 < 2^31."""
    return [Term("workgroups", 28, 0, P31)]


def maxpool_terms(h, w, c) -> List[Term]:
    """r50_op_maxpool: n*h*w*c*2 < 2^63."""
    return [Term("x", h * w * c * 2, 0, P63)]


def avgpool_terms(hw, c) -> List[Term]:
    """r50_op_avgpool: n*(c/8) + 255 < 2^31 and n*hw*c*2 < 2^63."""
    return [Term("threads", c // 8, 255, P31), Term("x", hw * c * 2, 0, P63)]


def rule(terms: List[Term], n: int) -> bool:
    return all(t.holds(n) for t in terms)


def n_max(terms: List[Term]) -> int:
    return min(t.n_max() for t in terms)


def decisive(terms: List[Term]) -> List[str]:
    """The names of the terms that fail one step beyond n_max."""
    n = n_max(terms) + 1
    return [t.name for t in terms if not t.holds(n)]


def crossing_n(elements_per_image: int) -> int:
    """The smallest n at which a 16-bit tensor of that many elements per image has crossed 2^31 elements (and so 2^32 bytes)."""
    return P31 // elements_per_image + 1


# ---- the cases
class SizeCase(NamedTuple):
    id: str
    op: str                         # the entry point of include/r50.h
    family: str                     # which runner of tests/test_size_limits_gpu.py
    shape: Tuple                    # the fixed shape arguments, per family (see the runner)
    tile: int                       # tile id (convolutions), else 0
    limited_by: str                 # "x", "y", "x_back", "M", "x2", "out" -- or "cap" (see the module docstring)
    terms: Callable[[], List[Term]]
    n_run: Optional[int] = None     # "cap" cases only
    beyond: bool = True             # False: the same (op, shape) is refused in another case -- the refusal comes before the tile is looked at

    @property
    def n_max(self) -> int:
        return n_max(self.terms())

    @property
    def n_at(self) -> int:
        return self.n_max if self.n_run is None else self.n_run


# tile ids of implementation_phd_lab_vision_amd/ops.py, restated so that this module imports nothing that loads the library
T_AUTO, T_128x128, T_64x128, T_64x256, T_128x128_P3, T_256x256 = 0, 1, 2, 3, 8, 9
PERSISTENT, WS, T_C64, T_XRES, T_S2, T_G8, T_G8_224 = 32, 64, 80, 81, 82, 83, 84


def _conv(id, op, shape, tile, limited_by, beyond=True):
    """shape: h, w, cin, cout, k, stride, pad, relu, residual"""
    h, w, cin, cout, k, stride, pad = shape[:7]
    return SizeCase(id, op, "conv", shape, tile, limited_by, lambda: conv_terms(h, w, cin, cout, k, stride, pad, op), beyond=beyond)


X64 = (56, 56, 64, 64, 1, 1, 0, True, False)            # x at the limit: 401,408 bytes per image in, as many out
X128 = (56, 56, 128, 128, 1, 1, 0, True, False)         # the same for the tiles that need cout % 128 == 0 (x and y tie)
Y256 = (56, 56, 64, 256, 1, 1, 0, True, True)           # y (and the residual) at the limit
XB512 = (7, 7, 512, 512, 3, 1, 1, True, False)          # x_back decisive: 42,799 images fit without it
C64 = (56, 56, 64, 64, 3, 1, 1, True, False)
S2 = (56, 56, 128, 128, 3, 2, 1, True, False)
FP8 = (56, 56, 128, 64, 1, 1, 0, True, False)           # the smallest cin / cout the fp8 path admits

CASES: List[SizeCase] = [
    _conv("conv_x_64x128", "r50_op_conv2d", X64, T_64x128, "x"),
    _conv("conv_x_64x256_persistent", "r50_op_conv2d", X64, T_64x256 | PERSISTENT, "x", beyond=False),
    _conv("conv_x_ws9", "r50_op_conv2d", X64, WS | 9, "x", beyond=False),
    _conv("conv_x_auto", "r50_op_conv2d", X64, T_AUTO, "x", beyond=False),
    _conv("conv_x_128x128_p3", "r50_op_conv2d", X128, T_128x128_P3, "x"),
    _conv("conv_x_ws1", "r50_op_conv2d", X128, WS | 1, "x", beyond=False),
    _conv("conv_y_g8", "r50_op_conv2d", Y256, T_G8, "y"),
    _conv("conv_y_g8_224", "r50_op_conv2d", Y256, T_G8_224, "y", beyond=False),
    _conv("conv_y_ws3", "r50_op_conv2d", Y256, WS | 3, "y", beyond=False),
    _conv("conv_y_256x256_persistent", "r50_op_conv2d", Y256, T_256x256 | PERSISTENT, "y", beyond=False),
    _conv("conv_xback_128x128", "r50_op_conv2d", XB512, T_128x128, "x_back"),
    _conv("conv_xback_xres", "r50_op_conv2d", XB512, T_XRES, "x_back", beyond=False),
    _conv("conv_c64", "r50_op_conv2d", C64, T_C64, "x"),
    _conv("conv_s2", "r50_op_conv2d", S2, T_S2, "x"),
    _conv("conv_s2_generic", "r50_op_conv2d", S2, T_128x128, "x", beyond=False),
    _conv("conv_f16", "r50_op_conv2d_f16", X64, T_64x128, "x"),
    _conv("conv_w2", "r50_op_conv2d_w2", X64, T_64x128, "x"),
    _conv("conv_split", "r50_op_conv2d_split", X64, T_AUTO, "x"),
    _conv("conv_fp8", "r50_op_conv2d_fp8", FP8, WS | 9, "x"),
    # layer2.0 family: x1 (n,4,4,128), x2 (n,8,8,256) at stride 2, cout 512: x2 is the largest tensor and decides
    SizeCase("cat_auto", "r50_op_conv1x1_cat", "cat", (4, 128, 8, 256, 2, 512), T_AUTO, "x2", lambda: cat_terms(4, 128, 8, 256, 512)),
    SizeCase("cat_g8", "r50_op_conv1x1_cat", "cat", (4, 128, 8, 256, 2, 512), T_G8, "x2", lambda: cat_terms(4, 128, 8, 256, 512), beyond=False),
    # shape: cmid, c1, downsample.  Every m_max is 2^k - 1: no multiple of 16 or 112, the last tile is ragged against the limit
    SizeCase("tail_c64_c1_64", "r50_op_bneck_tail", "tail", (64, 64, False), 0, "out", lambda: tail_terms(64)),
    SizeCase("tail_c64_c1_128", "r50_op_bneck_tail", "tail", (64, 128, False), 0, "out", lambda: tail_terms(64)),
    SizeCase("tail_c64_downsample", "r50_op_bneck_tail", "tail", (64, 64, True), 0, "out", lambda: tail_terms(64)),
    SizeCase("tail_c128", "r50_op_bneck_tail", "tail", (128, 128, False), 0, "out", lambda: tail_terms(128)),
    SizeCase("tail_c256", "r50_op_bneck_tail", "tail", (256, 256, False), 0, "out", lambda: tail_terms(256)),
    SizeCase("tail_c256_no_next", "r50_op_bneck_tail", "tail", (256, 0, False), 0, "out", lambda: tail_terms(256)),
    SizeCase("block1", "r50_op_bneck_block1", "block1", (64, False), 0, "out", block1_terms),
    SizeCase("block1_ds", "r50_op_bneck_block1_ds", "block1", (64, True), 0, "out", block1_terms),
    SizeCase("block2", "r50_op_bneck_block2", "block2", (True,), 0, "out", block2_terms),
    SizeCase("cat_chain", "r50_op_bneck_cat_chain", "cat_chain", (28,), 0, "x", cat_chain_terms),
    # limits above the memory cap: run where the largest 16-bit tensor (the pools' input, the stem's output) crosses 2^31 elements
    SizeCase("maxpool", "r50_op_maxpool", "maxpool", (112, 112, 64), 0, "cap", lambda: maxpool_terms(112, 112, 64),
             n_run=crossing_n(112 * 112 * 64), beyond=False),
    SizeCase("avgpool", "r50_op_avgpool", "avgpool", (49, 2048), 0, "cap", lambda: avgpool_terms(49, 2048),
             n_run=crossing_n(49 * 2048), beyond=False),
    SizeCase("stem", "r50_op_stem", "stem", (), 0, "cap", stem_terms, n_run=crossing_n(112 * 112 * 64), beyond=False),
]

# the entry points of the issue: each must have a case, and a limits sentence in its header comment
ENTRY_POINTS = ["r50_op_conv2d", "r50_op_conv2d_f16", "r50_op_conv2d_w2", "r50_op_conv2d_split", "r50_op_conv2d_fp8", "r50_op_conv1x1_cat",
                "r50_op_bneck_tail", "r50_op_bneck_block1", "r50_op_bneck_block1_ds", "r50_op_bneck_block2", "r50_op_bneck_cat_chain",
                "r50_op_stem", "r50_op_maxpool", "r50_op_avgpool"]

# what today's rules give (the issue's table), so that a change of a rule shows up as a change of a number here
EXPECTED_N_MAX = {"conv_x_64x128": 5349, "conv_x_128x128_p3": 2674, "conv_y_g8": 1337, "conv_xback_128x128": 42798, "conv_c64": 5349,
                  "conv_s2": 2674, "conv_f16": 5349, "conv_w2": 5349, "conv_split": 2674, "conv_fp8": 5349, "cat_auto": 65535,
                  "tail_c64_c1_64": (1 << 22) - 1, "tail_c128": (1 << 21) - 1, "tail_c256": (1 << 20) - 1, "block1": 1337, "block1_ds": 1337,
                  "block2": 2674, "cat_chain": 1337}


def comment_blocks(fn: str, header_text: str) -> str:
    """The comment text that belongs to prototype ``fn`` in a header: every comment between the end of the preceding prototype and ``fn``'s own;
    where there is none (two prototypes under one comment), the nearest comment in front of it."""
    import re
    m = re.search(r"^\s*(?:int|int64_t|size_t)\s+" + re.escape(fn) + r"\s*\(", header_text, flags=re.M)
    assert m, f"{fn} is not declared"
    before = header_text[:m.start()]
    prev = [p.end() for p in re.finditer(r"^\s*(?:int|int64_t|size_t)\s+r50_op_\w+\s*\([^;{}]*\)\s*;", before, flags=re.M)]
    start = prev[-1] if prev else 0
    blocks = re.findall(r"/\*.*?\*/", before[start:], flags=re.S)
    if not blocks:
        blocks = re.findall(r"/\*.*?\*/", before, flags=re.S)[-1:]
    return "\n".join(blocks)
