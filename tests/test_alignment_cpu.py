"""The alignment contract of include/r50*.h read back from the headers, and the harness of tests/alignment.py proved on CPU tensors.

  the contract  every pointer parameter resolves to a requirement; every `void` device pointer carries R50_ALIGNED; annotations are powers
                of two between the element size and 256; every annotation is enforced by name in csrc/r50_abi.hip; the ops whose header
                prose states an alignment agree with their annotation; every entry point a table row names is declared.
  the harness   ``shift`` gives the asked address residues and keeps bytes, shape and dtype; through the recording proxy and a
                ``ShiftedArena`` on CPU tensors, a toy op that rounds its pointer down to 16 bytes before it reads is caught (it reads the
                fill), a toy op that stores 4-byte pairs past the last element of a 2-byte-displaced output is caught by the back band, and
                an honest toy op passes.
"""
import re

import pytest
import torch

from tests import alignment as AL
from tests import guard_bands as G
from tests.test_guard_bands_cpu import SMALL, _shifted

ABI = (AL.ROOT / "implementation_phd_lab_vision_amd" / "csrc" / "r50_abi.hip").read_text()

# (entry point, parameter, bytes) as the header comments of the ops that stated an alignment before R50_ALIGNED existed put it ("x 16-byte
# aligned", "src, out or out_flip not 4-byte aligned (the table: 8-byte)", "v or out not 8-byte aligned (counts not 4-byte aligned)"):
# the annotation pass cannot silently relax one of them.
STATED = [
    ("r50_op_gather_window_rows", "src_f32", 16), ("r50_op_gather_window_rows", "dst", 16),
    ("r50_op_ar_latent_grad", "ar", 16), ("r50_op_ar_latent_grad", "phi", 16), ("r50_op_ar_latent_grad", "dphi_hat", 16),
    ("r50_op_ar_latent_grad", "dar", 16),
    ("r50_op_hal_latent_grad", "h", 16), ("r50_op_hal_latent_grad", "phi", 16), ("r50_op_hal_latent_grad", "dh_reg", 16),
    ("r50_op_hal_latent_grad", "dh", 16),
    ("r50_op_rollout_latent_grad", "fut", 16), ("r50_op_rollout_latent_grad", "phi", 16), ("r50_op_rollout_latent_grad", "dfut", 16),
    ("r50_op_grad_norm", "g", 16), ("r50_op_row_norm2", "x", 16), ("r50_op_nn_search", "q", 16), ("r50_op_nn_search", "x", 16),
    ("r50_op_pose_rotations", "quat", 16), ("r50_op_resample_sequences", "out_time", 8),
    ("r50_op_bootstrap_sums", "v", 8), ("r50_op_bootstrap_sums", "out", 8), ("r50_op_bootstrap_sums", "counts", 4),
    ("r50_op_crop_resize_boxes_u8", "src_u8", 4), ("r50_op_crop_resize_boxes_u8", "out_tchw_u8", 4),
    ("r50_op_crop_resize_boxes_u8", "out_flip_tchw_u8", 4), ("r50_op_crop_resize_boxes_u8", "table_dev", 8),
]


def _device_pointers():
    return [(fn, p) for fn, params in AL.prototypes().items() for p in params if p.device]


def _least_element_bytes(fn, p):
    """The smallest element the op may be given through this pointer: the pointee type; for `void`, one byte for uint8 / fp8 tensors and raw
    workspaces, else the two bytes of the 16-bit element types `et` selects."""
    if p.pointee_bytes is not None:
        return p.pointee_bytes
    return 1 if re.search(r"u8|fp8|workspace|scratch", fn + " " + p.name) else 2


def test_every_pointer_parameter_resolves_to_a_requirement():
    protos = AL.prototypes()
    assert {"r50_forward", "r50_op_conv2d", "r50_op_hal_latent_grad", "r50_op_crop_resize_boxes_u8", "r50_op_view_fuse"} <= set(protos)
    assert len(_device_pointers()) >= 300
    for fn, p in _device_pointers():
        assert p.required and p.required >= 1, f"{fn}: device pointer `{p.name}` ({p.ctype}) has no requirement"
    for fn, params in protos.items():
        for p in params:
            if p.pointer and not p.device and p.name != "stream" and not p.ctype.startswith("r50_") and p.ctype != "void":
                assert p.required, f"{fn}: host pointer `{p.name}` ({p.ctype}) has no natural alignment"


def test_every_void_device_pointer_is_annotated():
    voids = [(fn, p) for fn, p in _device_pointers() if p.ctype == "void"]
    assert len(voids) >= 100
    missing = [f"{fn}: {p.name}" for fn, p in voids if p.annotation is None]
    assert not missing, f"`void` device pointers without R50_ALIGNED: {missing}"


def test_annotations_are_powers_of_two_between_the_element_size_and_256():
    n = 0
    for fn, p in _device_pointers():
        if p.annotation is None:
            continue
        n += 1
        a = p.annotation
        assert a & (a - 1) == 0 and 1 <= a <= 256, f"{fn}: `{p.name}` R50_ALIGNED({a})"
        assert a >= _least_element_bytes(fn, p), f"{fn}: `{p.name}` R50_ALIGNED({a}) is below its element size"
    assert n >= 150
    for fn, params in AL.prototypes().items():
        for p in params:
            assert p.annotation is None or p.device, f"{fn}: `{p.name}` is annotated but is no device pointer"


def test_every_annotation_is_enforced_by_name():
    """csrc/r50_abi.hip checks every annotated pointer that needs more than one byte through its frame's `aligned`, under the header's
    parameter name and with the header's bytes -- so a refusal names the parameter, and no annotated pointer can reach a launch unchecked.
    The entry point a check belongs to is the one its frame (`const Op op{"r50_...", ...}`, the nearest one above the check) names; inside
    the definition of an exported `int r50_...(` that name must be the function's own, and be the only time the body spells it."""
    frames = [(m.start(), re.findall(r'"(r50_\w+)"', m.group(1))) for m in re.finditer(r'\bconst Op op\{([^;]*?)\};', ABI)]
    assert len(frames) >= 70 and all(fns for _at, fns in frames)
    checks, n_checked = {}, 0
    for m in re.finditer(r'\bop\.aligned\(\s*\{(.*?)\}\s*\)\)', ABI, flags=re.S):
        fns = [f for at, f in frames if at < m.start()][-1]
        for _ptr, name, nbytes in re.findall(r'\{\s*(\w+)\s*,\s*([^,{}]+?)\s*,\s*([^{}]+?)\s*\}', m.group(1)):
            n_checked += 1
            for fn in fns:
                checks.setdefault(fn, []).append((name, nbytes))
    print(f"{n_checked} pointers checked by name in r50_abi.hip, for {len(checks)} entry points")
    assert n_checked >= 142 and len(checks) >= 43            # what the need_aligned calls held before the frames
    for m in re.finditer(r'^int (r50_\w+)\([^;{}]*\) \{\n(.*?)^\}', ABI, flags=re.S | re.M):
        fn, body = m.group(1), m.group(2)
        if "const Op op{" in body:
            named = re.findall(r'"(r50_\w+)', body)
            assert named == [fn] if fn.startswith("r50_op_") else set(named) == {fn}, f"{fn}: its body names {named}"
    for fn, p in _device_pointers():
        if p.annotation is None or p.annotation == 1:
            continue
        got = [nb for name, nb in checks.get(fn, []) if f'"{p.name}"' in name]
        assert got, f"{fn}: `{p.name}` is R50_ALIGNED({p.annotation}) in the header, but r50_abi.hip does not check it"
        assert any(re.search(rf"\b{p.annotation}u?\b", nb) for nb in got), f"{fn}: `{p.name}` is checked for {got}, the header says {p.annotation}"


def test_the_stated_alignments_agree_with_the_annotations():
    protos = AL.prototypes()
    for fn, name, nbytes in STATED:
        p = {q.name: q for q in protos[fn]}[name]
        assert p.required == nbytes, f"{fn}: `{name}` was stated as {nbytes}-byte aligned, the header now gives {p.required}"


def test_every_entry_point_of_a_table_row_is_declared():
    from tests.rows import ALL_ROWS
    protos = AL.prototypes()
    assert len(ALL_ROWS) >= 200
    for row in ALL_ROWS:
        for op in row.ops:
            assert op in protos, f"row {row.id} names {op}, which no header declares"
            assert any(p.device for p in protos[op]), f"row {row.id}: {op} has no device operand"


# ------------------------------------------------------------------------------------------------------------------------------
# the harness on CPU tensors
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32, torch.float64, torch.int32], ids=str)
def test_shift_gives_the_asked_residue_and_keeps_bytes_shape_and_dtype(dtype):
    src = (torch.arange(3 * 5 * 7) % 97).view(3, 5, 7).to(dtype)
    size = src.element_size()
    for shift in (0, size, 3 * size, 16, 48, 8 * 16 - size):
        for fill in G.FILLS:
            t = G.guarded(src, fill, band=SMALL, shift=shift)
            e = G.guarded_empty(src.shape, dtype, fill, band=SMALL, shift=shift)
            for v in (t, e):
                front, back = G.bands_of(v)
                assert v.is_contiguous() and v.shape == src.shape and v.dtype == dtype
                assert front.numel() == SMALL + shift and back.numel() >= SMALL and front.data_ptr() % 64 == 0
                assert (v.data_ptr() - front.data_ptr()) == SMALL + shift and v.data_ptr() % 64 == shift % 64
                assert bool((front == fill).all()) and bool((back == fill).all())
                assert back.data_ptr() == v.data_ptr() + v.numel() * size
            assert torch.equal(G.bits(t), G.bits(src))
            assert G.holds_fill(e, fill) == e.numel()
    with pytest.raises(ValueError):
        G.guarded(src.to(torch.float32), G.FILL_BIG, band=SMALL, shift=2)       # would split an element


def test_least_and_below_shifts_place_the_pointer():
    for a in (2, 4, 8, 16, 64, 256):
        for offset in (0, a, 3 * a, 40 * a):
            req = AL.Requirement(a, offset, "f", "p")
            for k in range(4):
                p = 4096 + AL.least_shift(req, k) + offset
                assert AL.displaced(p, a) and (p // a) % 8 == AL.ODD[k]
            p = 4096 + AL.below_shift(req) + offset
            assert p % a == a // 2
    assert [AL.least_shift(AL.Requirement(1, 0, "f", "p"), k) for k in range(4)] == [1, 2, 3, 1]
    assert AL.displaced(4097, 1) and AL.displaced(4098, 1) and not AL.displaced(4096, 1) and not AL.displaced(32, 16) and AL.displaced(48, 16)


class _ToyLib:
    """Stands in for the ctypes library: r50_op_cast_rows (src fp32 natural, dst R50_ALIGNED(4)) computed in torch on the arena's tensors.
    how = "honest"; "rounds_down": reads src from its address rounded down to 16 bytes; "pair_past": stores whole 4-byte pairs, one
    element past an odd-length dst."""

    def __init__(self, arena, how):
        self.arena, self.how = arena, how

    def r50_last_error(self, _h):
        return b"r50_op_cast_rows: dst must be 4-byte aligned"

    def r50_op_cast_rows(self, src, rows, c, dst, cpad, et, stream):
        if dst % 4:
            return -1
        ops = dict(self.arena.operands)
        x, y = ops["src"], ops["dst"]
        assert x.data_ptr() == src and y.data_ptr() == dst
        if self.how == "rounds_down":
            x = _shifted(x, -((src % 16) // 4))
        v = x.to(torch.bfloat16).view(torch.int16)
        if self.how == "pair_past":
            y.as_strided((y.numel() + 1,), (1,), y.storage_offset())[:-1].copy_(v.view(-1))
            y.as_strided((y.numel() + 1,), (1,), y.storage_offset())[-1] = 0
        else:
            y.copy_(v)
        return 0


def _toy_run(arena, how):
    x = torch.tensor([[-1.5, 2.0, 0.25], [-3.0, 7.0, 11.0], [0.5, 1.0, 9.0]])
    src, dst = arena.inp("src", x), arena.out("dst", (3, 3), torch.int16)
    lib = _ToyLib(arena, how)
    with AL.recording(arena, lib=lib, stop_at=getattr(arena, "victim", None)) as proxy:
        from implementation_phd_lab_vision_amd import _lib as L
        rc = L.load_library().r50_op_cast_rows(src.data_ptr(), 3, 3, dst.data_ptr(), 3, 0, None)
    return rc, proxy


def _cpu_arenas():
    from tests.guard_bands import Arena

    class CpuArena(Arena):
        def inp(self, name, t):
            return self._put(name, t.detach().clone().contiguous())

        def out(self, name, shape, dtype, defined=True):
            self.results[name] = self._put(name, torch.zeros(tuple(shape), dtype=dtype))
            self.defined[name] = defined
            return self.results[name]
    return CpuArena, AL.make_shifted_arena(CpuArena, "cpu")


def _plain_and_reqs():
    CpuArena, Shifted = _cpu_arenas()
    plain = CpuArena(None)
    rc, proxy = _toy_run(plain, "honest")
    assert rc == 0
    reqs = AL.requirements(proxy.seen)
    assert {k: (v.bytes, v.param) for k, v in reqs.items()} == {"src": (4, "src_f32"), "dst": (4, "dst")}       # from include/r50.h
    return plain, reqs, Shifted


def test_an_honest_toy_op_passes_at_the_least_alignment():
    plain, reqs, Shifted = _plain_and_reqs()
    least = Shifted(reqs, "least")
    rc, proxy = _toy_run(least, "honest")
    assert rc == 0 and all(AL.displaced(s.pointer, s.required) for s in proxy.seen) and len(proxy.seen) == 2
    assert {s.pointer % 8 for s in proxy.seen} == {4} and least.shifts == {"src": 4, "dst": 12}
    G.assert_bands_intact(least.operands, least.fill)
    assert torch.equal(G.bits(least.results["dst"]), G.bits(plain.results["dst"])) and G.holds_fill(least.results["dst"], least.fill) == 0


def test_a_toy_op_that_rounds_its_pointer_down_is_caught():
    plain, reqs, Shifted = _plain_and_reqs()
    least = Shifted(reqs, "least")
    rc, _proxy = _toy_run(least, "rounds_down")
    assert rc == 0
    G.assert_bands_intact(least.operands, least.fill)                       # it only reads: the bands cannot see it
    assert not torch.equal(G.bits(least.results["dst"]), G.bits(plain.results["dst"])), "the op read the fill and still gave the plain bits"
    plain2 = type(plain)(None)
    _toy_run(plain2, "rounds_down")                                          # on the allocator's alignment the same op is invisible
    assert torch.equal(G.bits(plain2.results["dst"]), G.bits(plain.results["dst"]))


def test_a_toy_op_that_stores_a_pair_past_its_last_element_is_caught():
    _plain, reqs, Shifted = _plain_and_reqs()
    least = Shifted(reqs, "least")
    rc, _proxy = _toy_run(least, "pair_past")
    assert rc == 0
    with pytest.raises(AssertionError, match="behind `dst`"):
        G.assert_bands_intact(least.operands, least.fill)


def test_below_the_alignment_the_proxy_stops_at_the_refusal():
    _plain, reqs, Shifted = _plain_and_reqs()
    below = Shifted(reqs, "below", victim="dst")
    with pytest.raises(AL.Refused) as e:
        _toy_run(below, "honest")
    assert e.value.rc == -1 and e.value.param == "dst" and e.value.param in e.value.message and below.shifts == {"src": 0, "dst": 2}
    assert G.holds_fill(below.results["dst"], below.fill) == below.results["dst"].numel()       # nothing was written
