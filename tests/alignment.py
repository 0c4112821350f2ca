"""Operands at exactly the least alignment an op admits -- test infrastructure for tests/test_alignment_gpu.py and tests/test_alignment_cpu.py.

Every other op test hands the library pointers that come straight from the allocator (256-byte aligned and better), while production
passes contiguous slices (``out[2:]``, ``acc[3:]``, ``dseq[n * b:]``).  include/r50.h states, per device pointer, the alignment the
kernels behind it need (``R50_ALIGNED(n)``, else the natural alignment of the pointee type) and csrc/r50_abi.hip refuses anything below it
before any launch.  Here:

  the header reader   ``prototypes()`` parses every prototype of include/r50*.h: per entry point and parameter the pointee size, the
                      annotation and the requirement (the annotation, else the pointee size).  The header is the only source of a
                      requirement: the tests keep no table of their own.
  the recording proxy ``recording(arena)`` stands in front of the ctypes library for one run (it replaces ``_lib.load_library``, which the
                      wrappers and the tables' ``lib()`` of tests/guard_bands.py both call every time).  It forwards every call and notes, for each integer argument
                      that falls inside an arena operand's bytes, (operand, entry point, parameter, offset into the operand, pointer).  So
                      the 200-odd table rows need no annotation of their own: a plain run tells which C parameter each operand is.
  ``requirements``    per operand, the largest requirement over the parameters it was passed as, with the offset it was passed at.
  ``ShiftedArena``    the interface of ``Arena`` (tests/guard_bands.py); every operand between 0x7B bands, ``shift`` bytes behind
                      the front band (tests/guard_bands.py).  mode "least": the pointer the op receives is an odd multiple of its
                      requirement A (p % A == 0 and p % 2A == A; the odd multiple cycles 1, 3, 5, 7 over a row's operands, for A = 1 the
                      shift cycles 1, 2, 3), asserted afterwards on what the proxy saw.  mode "below": one victim operand sits A/2 off an
                      A-aligned address, all others as the allocator gives them; the proxy stops the row at the first call that receives
                      the victim below that parameter's own requirement (``Refused`` carries its status and the library's message; a
                      call that takes the same operand through a parameter with a smaller requirement runs, legitimately), so nothing runs after a refusal -- and
                      nothing is ever launched below a requirement unless the library failed to refuse, which is the failing test.

What this cannot see: the handle's internal activation arena; host pointers; alignments between the tested odd multiple and the
allocator's; and what the hardware would do below a requirement, which is deliberately never tried.
"""
import contextlib
import functools
import re
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional

import torch

from tests import guard_bands as G

ROOT = Path(__file__).resolve().parents[1]
HEADERS = sorted((ROOT / "include").glob("r50*.h"))

POINTEE_BYTES = {"float": 4, "double": 8, "int": 4, "int64_t": 8, "uint64_t": 8, "uint8_t": 1, "char": 1, "size_t": 8}
# Entry points that manage a handle or answer a size query: no device operand among their pointers (handles, host descriptors, host
# out-parameters).  Not an alignment table: it only tells the reader which `void*` are not device pointers.
HOST_ONLY = {"r50_create", "r50_load_weights", "r50_share_weights", "r50_set_option", "r50_get_option", "r50_profile_reset",
             "r50_profile_collect", "r50_profile_count", "r50_profile_entry", "r50_get_packed", "r50_set_fp8_scales", "r50_last_error",
             "r50_destroy", "r50_version", "r50_stem_scratch_bytes", "r50_op_nn_search_workspace", "r50_track_weight_precision"}


class Param(NamedTuple):
    name: str
    ctype: str                  # the pointee (or value) type without const
    pointer: bool
    device: bool                # a device operand: a pointer that is neither `stream`, a handle, a *_host pointer nor a host out-parameter
    pointee_bytes: Optional[int]    # None for void and for structs
    annotation: Optional[int]
    required: Optional[int]     # bytes: the annotation, else the pointee size; None only where neither exists (a finding for the CPU test)


def _strip(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^\s*#.*$", " ", text, flags=re.M)


def _param(fn: str, raw: str) -> Param:
    m = re.search(r"R50_ALIGNED\(\s*(\d+)\s*\)", raw)
    annotation = int(m.group(1)) if m else None
    text = re.sub(r"R50_ALIGNED\(\s*\d+\s*\)", " ", raw)
    array = "[" in text
    text = re.sub(r"\[[^\]]*\]", " ", text)
    name = re.findall(r"[A-Za-z_]\w*", text)[-1]
    stars = text.count("*")
    pointer = stars > 0 or array
    ctype = " ".join(w for w in re.findall(r"[A-Za-z_]\w*", text)[:-1] if w != "const")
    size = POINTEE_BYTES.get(ctype) if stars <= 1 and not (stars == 1 and array) else 8
    host = (fn in HOST_ONLY or name == "stream" or name.endswith("_host") or ctype.startswith("r50_") or array or stars > 1 or
            ctype == "char")
    device = pointer and not host
    required = annotation if annotation is not None else (size if pointer else None)
    return Param(name, ctype, pointer, device, size if pointer else None, annotation, required)


@functools.lru_cache(maxsize=None)
def prototypes(headers=None) -> Dict[str, List[Param]]:
    """entry point -> its parameters, over every prototype of include/r50*.h (or of the given header files)."""
    out: Dict[str, List[Param]] = {}
    for path in (HEADERS if headers is None else [Path(h) for h in headers]):
        text = _strip(Path(path).read_text())
        for m in re.finditer(r"^\s*(?:const\s+char\s*\*|int64_t|size_t|int|void)\s+(r50_\w+)\s*\(([^;{}]*)\)\s*;", text, flags=re.M):
            fn, args = m.group(1), m.group(2).strip()
            assert fn not in out, f"{fn} is declared twice"
            out[fn] = [] if args in ("", "void") else [_param(fn, a) for a in args.split(",")]
    assert len(out) >= 90 and "r50_op_avgpool" in out and "r50_op_bootstrap_sums" in out, f"the header reader found {len(out)} prototypes"
    return out


# ------------------------------------------------------------------------------------------------------------------------------
class Seen(NamedTuple):
    operand: str
    fn: str
    param: str
    index: int
    offset: int
    pointer: int
    required: int
    call: int = 0               # the how-manieth call of the run it was


class Refused(Exception):
    """Raised by the proxy in mode "below" at the first call that received the victim: the row stops there."""

    def __init__(self, fn, param, rc, message):
        super().__init__(f"{fn}({param}) returned {rc}: {message}")
        self.fn, self.param, self.rc, self.message = fn, param, rc, message


def _as_int(v):
    if isinstance(v, bool):
        return None
    if isinstance(v, int):
        return v
    val = getattr(v, "value", None)
    return val if isinstance(val, int) and not isinstance(val, bool) else None


class RecordingLib:
    """Stands in front of the ctypes library: forwards everything, notes which arena operand each pointer argument is."""

    def __init__(self, lib, arena, stop_at: Optional[str] = None):
        self._lib, self._arena, self._stop_at = lib, arena, stop_at
        self.seen: List[Seen] = []
        self.calls: List[str] = []

    def _ranges(self):
        return [(name, t.data_ptr(), t.data_ptr() + max(t.numel() * t.element_size(), 1)) for name, t in self._arena.operands]

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        protos = prototypes()
        if name not in protos or not callable(fn):
            return fn

        def call(*args):
            params = protos[name]
            assert len(args) == len(params), f"{name}: {len(args)} arguments for {len(params)} parameters of the header"
            ranges = self._ranges()
            hit = None
            for i, (a, p) in enumerate(zip(args, params)):
                v = _as_int(a)
                if v is None or not p.device:
                    continue
                for op_name, lo, hi in ranges:
                    if lo <= v < hi:
                        assert p.required, f"{name}: parameter {p.name} has no alignment requirement"
                        s = Seen(op_name, name, p.name, i, v - lo, v, p.required, len(self.calls))
                        self.seen.append(s)
                        if op_name == self._stop_at and hit is None and v % p.required:      # below THIS parameter's requirement
                            hit = s
                        break
            self.calls.append(name)
            rc = fn(*args)
            if hit is not None:
                msg = self._lib.r50_last_error(None)
                raise Refused(name, hit.param, rc, msg.decode() if msg else "")
            return rc
        return call


@contextlib.contextmanager
def recording(arena, stop_at: Optional[str] = None, lib=None):
    """For the duration ``_lib.load_library`` gives a ``RecordingLib`` on ``arena``: the one path to the library, for the Python wrappers
    and for the tables' ``lib()`` (tests/guard_bands.py) alike."""
    from implementation_phd_lab_vision_amd import _lib as L
    real = L.load_library() if lib is None else lib
    proxy = RecordingLib(real, arena, stop_at)
    saved = L.load_library
    try:
        L.load_library = lambda: proxy
        yield proxy
    finally:
        L.load_library = saved


class Requirement(NamedTuple):
    bytes: int          # A
    offset: int         # the offset into the operand at which the parameter that sets A received it
    fn: str
    param: str


def requirements(seen: List[Seen]) -> Dict[str, Requirement]:
    """Per operand: the largest requirement over the parameters it was passed as, at the offset it was passed with."""
    out: Dict[str, Requirement] = {}
    for s in seen:
        if s.operand not in out or s.required > out[s.operand].bytes:
            out[s.operand] = Requirement(s.required, s.offset, s.fn, s.param)
    return out


ODD = (1, 3, 5, 7)
BYTE_SHIFTS = (1, 2, 3)


def least_shift(req: Requirement, k: int) -> int:
    """Bytes behind a band boundary (itself a multiple of 4096) so that boundary + shift + offset is the odd multiple ODD[k % 4] of A; for
    A = 1 the shifts 1, 2, 3."""
    a = req.bytes
    if a == 1:
        return BYTE_SHIFTS[k % 3]
    return (ODD[k % 4] * a - req.offset) % (8 * a)


def below_shift(req: Requirement) -> int:
    return (req.bytes // 2 - req.offset) % req.bytes


def displaced(pointer: int, a: int) -> bool:
    """The pointer is an odd multiple of A (for A = 1: off every 4-byte boundary or on an odd one, i.e. not a multiple of 4)."""
    return pointer % 4 != 0 if a == 1 else (pointer % a == 0 and pointer % (2 * a) == a)


def make_shifted_arena(base, device):
    """``ShiftedArena`` over ``base`` (the ``Arena`` class of tests/guard_bands.py; a CPU stand-in in tests/test_alignment_cpu.py)."""

    class ShiftedArena(base):
        def __init__(self, reqs: Dict[str, Requirement], mode: str = "least", victim: Optional[str] = None, fill: int = G.FILL_BIG):
            super().__init__(fill)
            assert mode in ("least", "below") and (mode == "below") == (victim is not None)
            self.reqs, self.mode, self.victim = reqs, mode, victim
            self.shifts: Dict[str, int] = {}
            self.payloads: Dict[str, torch.Tensor] = {}      # name -> the payload of an input or in-out (rows never modify their payloads)

        def _shift(self, name, element_size):
            req = self.reqs.get(name)
            assert req is not None, f"operand `{name}` was not matched to a parameter in the plain run"
            if self.mode == "least":
                s = least_shift(req, len(self.shifts))
            else:
                s = below_shift(req) if name == self.victim else 0
            assert s % element_size == 0, f"`{name}`: shift {s} is no multiple of its element size {element_size}"
            self.shifts[name] = s
            return s

        def inp(self, name, t):
            self.payloads[name] = t
            return self._put(name, G.guarded(t, self.fill, device=device, shift=self._shift(name, t.element_size())))

        def _empty(self, name, shape, dtype):
            size = torch.empty((), dtype=dtype).element_size()
            return G.guarded_empty(shape, dtype, self.fill, device=device, shift=self._shift(name, size))

        def out(self, name, shape, dtype, defined=True):
            self.results[name] = self._put(name, self._empty(name, shape, dtype))
            self.defined[name] = defined
            return self.results[name]

        def ws(self, name, shape, dtype):
            return self._put(name, self._empty(name, shape, dtype))

    return ShiftedArena
