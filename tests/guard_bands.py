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
from typing import Iterable, Sequence, Tuple

import torch

FILL_NAN = 0xFF
FILL_BIG = 0x7B
FILLS = (FILL_NAN, FILL_BIG)
PAGE = 4096
BAND = 4 << 20          # bytes per band; tests/test_guard_bands_gpu.py asserts per case that this is twice what the kernel could reach


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
