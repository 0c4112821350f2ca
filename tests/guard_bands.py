"""Poisoned guard bands around kernel operands -- test infrastructure, CPU and GPU tensors alike.

A guarded operand lives inside one larger ``uint8`` allocation: ``[front band | payload | back band]``.  Every band byte holds one fill
value, so a kernel whose index arithmetic strays off its operand reads a known, hostile value instead of whatever the allocator left
next to it, and a kernel that writes off its operand leaves a mark that ``assert_bands_intact`` finds.  A test runs a kernel from the
same payloads three times -- on ordinary tensors, between 0xFF bands and between 0x7B bands -- and asks for the same output bits.

Two fills, because neither sees everything:

  0xFF in every byte  NaN as bf16, fp16, fp32, fp64 and e4m3fn; -1 as int32, 255 as uint8.  A stray NaN poisons a sum -- but an epilogue
                      that ends in ``fmax(v, 0)`` (every ReLU) turns it into 0 and hides it.
  0x7B in every byte  large, finite and positive: bf16 / fp32 ~ 1.3e36, fp16 61,280, fp64 ~ 6.5e286, e4m3 352, int32 ~ 2.07e9 (an index far
                      out of range), uint8 123.  It survives ReLU, fmax and fmin.

The front band's length is a multiple of 4096 bytes, so with ``shift=0`` the payload keeps the alignment the allocator gave the arena.
``shift`` (bytes, a multiple of the element size) moves the payload that far behind the front band -- ``[front band | shift bytes of fill |
payload | rest of the page(s), fill | back band]`` -- which is how tests/alignment.py places an operand at exactly the least alignment its
op admits ("Pointer alignment").  The gap counts as front band for ``bands_of`` / ``assert_bands_intact``.
"""
import functools
from typing import Callable, Iterable, NamedTuple, Sequence, Tuple

import torch

FILL_NAN = 0xFF
FILL_BIG = 0x7B
FILLS = (FILL_NAN, FILL_BIG)
PAGE = 4096
BAND = 4 << 20          # bytes per band; ``Arena.reach`` asserts per row that this is twice what the kernel could reach


def _round_up(v: int, m: int) -> int:
    return -(-v // m) * m


def _place(nbytes: int, fill: int, band: int, device, shift: int = 0, element_size: int = 1) -> torch.Tensor:
    if band <= 0 or band % PAGE:
        raise ValueError("band length must be a positive multiple of 4096 bytes")
    if fill not in range(256):
        raise ValueError("fill is one byte")
    if shift < 0 or shift % element_size:
        raise ValueError("shift must be a non-negative multiple of the element size")
    return torch.full((band + _round_up(max(shift + nbytes, 1), PAGE) + band,), fill, dtype=torch.uint8, device=device)


def guarded(t: torch.Tensor, fill: int, band: int = BAND, device=None, shift: int = 0) -> torch.Tensor:
    """A contiguous tensor with ``t``'s shape, dtype and bytes (on ``device``, default ``t``'s) between two bands of ``fill`` bytes, its first
    byte ``shift`` bytes behind the front band."""
    device = t.device if device is None else torch.device(device)
    src = t.detach().contiguous()
    nbytes = src.numel() * src.element_size()
    arena = _place(nbytes, fill, band, device, shift, src.element_size())
    view = arena[band + shift: band + shift + nbytes].view(src.dtype).view(src.shape)
    view.copy_(src)
    return view


def guarded_empty(shape: Sequence[int], dtype: torch.dtype, fill: int, band: int = BAND, device="cpu", shift: int = 0) -> torch.Tensor:
    """An output or workspace of ``shape`` / ``dtype`` between two bands (``shift`` as in ``guarded``); the payload is pre-filled with ``fill``
    as well, so an element the kernel leaves unwritten, or reads before writing it, differs between the fills."""
    shape = tuple(int(s) for s in shape)
    numel = 1
    for s in shape:
        numel *= s
    size = torch.empty((), dtype=dtype).element_size()
    nbytes = numel * size
    arena = _place(nbytes, fill, band, torch.device(device), shift, size)
    return arena[band + shift: band + shift + nbytes].view(dtype).view(shape)


RANDOM_CHUNK = 1 << 26      # elements drawn at a time by ``guarded_random``


def guarded_random(shape: Sequence[int], dtype: torch.dtype, fill: int, generator: torch.Generator, scale: float = 1.0,
                   limit: float = None, band: int = BAND, device="cpu", shift: int = 0) -> torch.Tensor:
    """Device-side placement of an operand too large to stage through the host (``guarded`` copies a tensor that already exists, which a
    2 GiB operand would hold twice): ``guarded_empty`` whose payload is then drawn where it lies, ``RANDOM_CHUNK`` elements at a time, as
    ``scale`` x standard normal values from ``generator`` (a generator of that device), clamped to +-``limit`` if given, rounded to
    ``dtype``.  Normal draws have no period: a read that wraps by 2^31 or 2^32 bytes sees other data."""
    t = guarded_empty(shape, dtype, fill, band, device, shift)
    flat = t.view(-1)
    for i in range(0, flat.numel(), RANDOM_CHUNK):
        part = flat[i: i + RANDOM_CHUNK]
        r = torch.randn(part.numel(), generator=generator, device=t.device, dtype=torch.float32)
        if scale != 1.0:
            r.mul_(scale)
        if limit is not None:
            r.clamp_(-limit, limit)
        part.copy_(r.to(dtype))
    return t


def bands_of(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (front, back) bands of a tensor made by ``guarded`` / ``guarded_empty`` (or of a view of one: its bands are then everything in
    front of and behind the view's own bytes), as uint8 views of the arena."""
    if not t.is_contiguous():
        raise ValueError("bands_of: need the contiguous view guarded() returned")
    arena = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    start = t.storage_offset() * t.element_size()
    end = start + t.numel() * t.element_size()
    return arena[:start], arena[end:]


def first_damage(band: torch.Tensor, fill: int):
    """None if every byte of ``band`` is ``fill``, else (offset of the first changed byte, how many bytes changed)."""
    bad = band != fill
    if not bool(bad.any()):
        return None
    idx = torch.nonzero(bad)
    return int(idx[0]), int(idx.numel())


def assert_bands_intact(operands: Iterable[Tuple[str, torch.Tensor]], fill: int, what: str = "") -> None:
    """Byte-compare both bands of every (name, tensor) operand of a call with ``fill``: inputs too -- a kernel must not write there either."""
    for name, t in operands:
        front, back = bands_of(t)
        assert front.numel() >= PAGE and back.numel() >= PAGE, f"{what}: {name} has no guard bands"
        for side, band in (("in front of", front), ("behind", back)):
            dmg = first_damage(band, fill)
            if dmg is not None:
                off = dmg[0] - band.numel() if side == "in front of" else dmg[0]
                raise AssertionError(f"{what}: {dmg[1]} byte(s) of the {fill:#04x} band {side} `{name}` were written, the first at byte "
                                     f"offset {off:+d} from the operand's {'start' if side == 'in front of' else 'end'}")


_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t: torch.Tensor) -> torch.Tensor:
    """``t`` as integers of its element size: comparisons see NaN payloads and the sign of zero."""
    return t.contiguous().view(_INT_OF_SIZE[t.element_size()])


def fill_pattern(dtype: torch.dtype, fill: int) -> torch.Tensor:
    """One element of ``dtype`` whose every byte is ``fill``."""
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((size,), fill, dtype=torch.uint8).view(dtype)[0]


def holds_fill(t: torch.Tensor, fill: int) -> int:
    """How many elements of ``t`` are the all-``fill`` pattern."""
    size = t.element_size()
    pat = torch.full((size,), fill, dtype=torch.uint8).view(_INT_OF_SIZE[size])[0]
    return int((bits(t) == pat.to(t.device)).sum())


# ---- the row catalogue's harness: what a table module of tests/rows/ is written with, and what every harness runs its rows through
DEV = "cuda:0"
BF, HF, F32, F64, I32, U8 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int32, torch.uint8


@functools.lru_cache(maxsize=None)
def _built():
    from implementation_phd_lab_vision_amd import _lib as L
    L.build_library()          # once per process: it hashes the sources
    return L


def lib():
    """The library, built once per process.  ``load_library`` is looked up on every call (it caches the handle itself), so that
    tests/alignment.py's ``recording`` can stand in front of it by replacing that one name."""
    return _built().load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(rc, what):
    assert rc == 0, f"{what}: {lib().r50_last_error(None)}"


def ptr(t):
    return None if t is None else t.data_ptr()


class Row(NamedTuple):
    family: str
    id: str
    ops: Tuple[str, ...]
    make: Callable          # () -> payloads (built once per row, shared by the three runs, never modified)
    launch: Callable        # (arena, payloads) -> None
    check: Callable = None  # (plain arena, payloads) -> None: the family's own oracle check, for a shape no other test runs
    scrub: Callable = None  # (payloads) -> None: for a row with state of its own (a backbone handle): overwrite what a run leaves in it


class Arena:
    """The operands of one run: plain tensors (fill None) or guarded ones."""

    def __init__(self, fill):
        self.fill = fill
        self.operands = []          # (name, tensor): everything whose bands are checked
        self.results = {}           # name -> tensor: outputs and in-outs, compared across the runs
        self.defined = {}           # name -> True where the op defines every element
        self.reached = 0

    def _put(self, name, t):
        assert name not in dict(self.operands), f"operand name {name} used twice"
        self.operands.append((name, t))
        return t

    def inp(self, name, t):
        if self.fill is None:
            return self._put(name, t.detach().to(DEV, copy=True).contiguous())
        g = guarded(t, self.fill, device=DEV)
        assert g.is_cuda and g.storage_offset() * g.element_size() == BAND and g.data_ptr() % 256 == 0, f"`{name}`: {g.device}, at {g.data_ptr():#x}"
        return self._put(name, g)

    def inout(self, name, t):
        self.results[name] = self.inp(name, t)
        return self.results[name]

    def out(self, name, shape, dtype, defined=True):
        if self.fill is None:
            t = torch.zeros(tuple(shape), dtype=U8, device=DEV).view(dtype) if dtype == torch.float8_e4m3fn else \
                torch.zeros(tuple(shape), dtype=dtype, device=DEV)
        else:
            t = guarded_empty(shape, dtype, self.fill, device=DEV)
        self.results[name] = self._put(name, t)
        self.defined[name] = defined
        return t

    def ws(self, name, shape, dtype):
        if self.fill is None:
            return self._put(name, torch.zeros(tuple(shape), dtype=dtype, device=DEV))
        return self._put(name, guarded_empty(shape, dtype, self.fill, device=DEV))

    def host_check(self, fn):
        """A look at a result on the host in the middle of a row.  Here: at once.  (tests/stream_order.py's arena puts it off until its run
        is over, so that the look does not hold the host.)"""
        fn()

    def between_calls(self, fn):
        """Between two calls of a row that go through one stateful object on the same inputs.  Here: nothing (each run is compared with the
        others as a whole).  tests/stream_order.py's arena runs ``fn``, which puts another batch through the object."""

    def reach(self, nbytes):
        """How far (bytes) this call's unchecked address arithmetic could land off an operand; the band must be twice that."""
        self.reached = max(self.reached, int(nbytes))
        assert BAND >= 2 * int(nbytes), f"guard band of {BAND} bytes is less than twice the reach {nbytes}"


def _checks_fill(t, fill):
    """Element sizes of two bytes and more: no legitimate output is the all-fill pattern.  One byte: only e4m3's NaN."""
    return t.element_size() >= 2 or (t.dtype == torch.float8_e4m3fn and fill == FILL_NAN)


def close_payloads(payloads) -> None:
    for v in payloads if isinstance(payloads, tuple) else ():
        if hasattr(v, "close"):
            v.close()              # a backbone handle


def run_row(row):
    payloads = row.make()
    try:
        _three_runs(row, payloads)
    finally:
        close_payloads(payloads)


def _three_runs(row, payloads):
    runs = {}
    for fill in (None,) + FILLS:
        a = Arena(fill)
        row.launch(a, payloads)
        torch.cuda.synchronize()
        assert a.reached > 0, f"{row.id}: the row does not state its reach"
        what = f"{row.id} fill {'plain' if fill is None else hex(fill)}"
        if fill is not None:
            assert_bands_intact(a.operands, fill, what)
            for name, t in a.results.items():
                if a.defined.get(name) and _checks_fill(t, fill):
                    n = holds_fill(t, fill)
                    assert n == 0, f"{what}: {n} of {t.numel()} elements of output `{name}` still hold the fill pattern"
        runs[fill] = a
    plain = runs[None]
    assert plain.results, f"{row.id}: no output"
    if row.check is not None:
        row.check(plain, payloads)
    for fill in FILLS:
        assert list(runs[fill].results) == list(plain.results), \
            f"{row.id} fill {fill:#x}: results {list(runs[fill].results)}, the plain run's {list(plain.results)}"
        for name, t in runs[fill].results.items():
            a, b = bits(t), bits(plain.results[name])
            if not torch.equal(a, b):
                bad = torch.nonzero((a != b).view(-1))
                raise AssertionError(f"{row.id} fill {fill:#x}: `{name}` differs from the plain run in {bad.numel()} of {a.numel()} "
                                     f"elements, the first at flat index {int(bad[0])}")


# ---- toy "kernels" in plain torch on ``as_strided`` views: what the harness is proved on (tests/test_guard_bands_cpu.py on the CPU,
# tests/test_guard_bands_gpu.py on device arenas)
def _shifted(x: torch.Tensor, by: int) -> torch.Tensor:
    """x's window moved by `by` elements: the view an index mistake of that size reads or writes."""
    return x.as_strided(x.shape, x.stride(), x.storage_offset() + by)


def _toy_reads_one_before(x, out):
    """y[i] = x[i] + 1 * x[i-1] over the whole operand: at i = 0 it reads one element in front of x."""
    out.copy_(x + _shifted(x, -1))


def _toy_reads_one_before_then_relu(x, out):
    """The same, then ReLU the way the kernels' fmax treats NaN: max(NaN, 0) = 0."""
    v = x + _shifted(x, -1)
    out.copy_(torch.where(torch.isnan(v), torch.zeros_like(v), v).clamp_min(0))


def _toy_writes_one_past(x, out):
    _shifted(out, 1).copy_(x)
    out[0] = x[0]


PAYLOAD = torch.tensor([-1.5, 2.0, 0.25, -3.0, 7.0])       # x[0] < 0: the true pre-activation of y[0] is negative
