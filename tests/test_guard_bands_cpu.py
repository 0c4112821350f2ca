"""The guard-band harness (tests/guard_bands.py) proved on the CPU: three toy "kernels" in plain torch on ``as_strided`` views of the arena
show what the harness detects and why it needs two fills; the fills' bit patterns are checked per dtype; and every op of include/r50.h
must have a row in tests/rows/r50.py (or a reason not to)."""
import math
import re
from pathlib import Path

import pytest
import torch

from tests import guard_bands as G
from tests.guard_bands import PAYLOAD, _shifted, _toy_reads_one_before, _toy_reads_one_before_then_relu, _toy_writes_one_past  # noqa: F401

ROOT = Path(__file__).resolve().parents[1]
SMALL = 2 * G.PAGE                      # band length of the toy runs


def _three_runs(kernel, payload, dtype=torch.float32):
    """The kernel on a plain tensor with a benign (zero) neighbour, as the caching allocator would give it, and between both fills."""
    outs = {}
    benign = torch.zeros(payload.numel() + 2, dtype=dtype)
    benign[1:-1] = payload
    out = torch.zeros(payload.numel() + 2, dtype=dtype)
    kernel(benign[1:-1], out[1:-1])
    outs["plain"] = out[1:-1].clone()
    for fill in G.FILLS:
        x = G.guarded(payload, fill, band=SMALL)
        y = G.guarded_empty(payload.shape, dtype, fill, band=SMALL)
        kernel(x, y)
        outs[fill] = (x, y)
    return outs


def _same_bits(a, b):
    return torch.equal(G.bits(a), G.bits(b))


def test_a_read_in_front_of_the_operand_is_caught_by_both_fills():
    runs = _three_runs(_toy_reads_one_before, PAYLOAD)
    for fill in G.FILLS:
        x, y = runs[fill]
        assert not _same_bits(y, runs["plain"]), f"fill {fill:#x} did not change the result"
        G.assert_bands_intact([("x", x), ("y", y)], fill)               # it only read
    assert torch.isnan(runs[G.FILL_NAN][1][0]) and float(runs[G.FILL_BIG][1][0]) > 1e35
    assert _same_bits(runs[G.FILL_NAN][1][1:], runs["plain"][1:])       # the other elements are functions of the payload alone


def test_a_relu_hides_the_nan_fill_and_the_finite_fill_survives_it():
    """The recorded reason for two fills: the stray NaN becomes 0 in the ReLU, exactly what the honest negative pre-activation gives."""
    runs = _three_runs(_toy_reads_one_before_then_relu, PAYLOAD)
    assert _same_bits(runs[G.FILL_NAN][1], runs["plain"]), "0xFF was expected to be swallowed by the ReLU"
    assert not _same_bits(runs[G.FILL_BIG][1], runs["plain"]), "0x7B must survive the ReLU"
    assert float(runs[G.FILL_BIG][1][0]) > 1e35


def test_a_write_past_the_output_is_caught_by_the_band_check():
    for fill in G.FILLS:
        x = G.guarded(PAYLOAD, fill, band=SMALL)
        y = G.guarded_empty(PAYLOAD.shape, torch.float32, fill, band=SMALL)
        _toy_writes_one_past(x, y)
        G.assert_bands_intact([("x", x)], fill)
        with pytest.raises(AssertionError, match=r"behind `y`.*offset \+0"):
            G.assert_bands_intact([("x", x), ("y", y)], fill, "toy")
    y = G.guarded_empty((5,), torch.float32, G.FILL_BIG, band=SMALL)
    _shifted(y, -1).copy_(PAYLOAD)                                      # and one element in front of it
    with pytest.raises(AssertionError, match=r"in front of `y`.*offset -4"):
        G.assert_bands_intact([("y", y)], G.FILL_BIG)


def test_an_honest_kernel_passes_and_an_unwritten_element_shows():
    for fill in G.FILLS:
        x = G.guarded(PAYLOAD, fill, band=SMALL)
        y = G.guarded_empty(PAYLOAD.shape, torch.float32, fill, band=SMALL)
        assert G.holds_fill(y, fill) == 5                               # the payload of an output starts out poisoned
        y[:4] = x[:4] * 2
        assert G.holds_fill(y, fill) == 1                               # the element the "kernel" left out
        y[4] = x[4] * 2
        assert G.holds_fill(y, fill) == 0 and torch.equal(y, PAYLOAD * 2)
        G.assert_bands_intact([("x", x), ("y", y)], fill)


# fp64: exponent field 0x7B7 = 1975, so 2^952 * 1.72 = 6.5e286
FLOATS = [torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.float8_e4m3fn]
BIG = {torch.bfloat16: 1.3e36, torch.float16: 61280.0, torch.float32: 1.3e36, torch.float64: 6.54e286, torch.float8_e4m3fn: 352.0}


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_fill_patterns_of_the_float_formats(dtype):
    nan = float(G.fill_pattern(dtype, G.FILL_NAN).to(torch.float64))
    assert math.isnan(nan)
    big = float(G.fill_pattern(dtype, G.FILL_BIG).to(torch.float64))
    assert math.isfinite(big) and big > 0
    assert abs(big - BIG[dtype]) <= 0.06 * BIG[dtype], big
    if dtype in (torch.float16, torch.float8_e4m3fn):
        assert big == BIG[dtype]


def test_fill_patterns_of_the_integer_formats():
    assert int(G.fill_pattern(torch.int32, G.FILL_NAN)) == -1
    assert int(G.fill_pattern(torch.uint8, G.FILL_NAN)) == 255
    assert int(G.fill_pattern(torch.int32, G.FILL_BIG)) == 0x7B7B7B7B > 2 ** 30     # beyond the largest n any op accepts
    assert int(G.fill_pattern(torch.uint8, G.FILL_BIG)) == 123


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32, torch.float64, torch.int32], ids=str)
def test_guarded_keeps_bytes_shape_and_alignment(dtype):
    src = (torch.arange(3 * 5 * 7) % 97).view(3, 5, 7).to(dtype)
    for fill in G.FILLS:
        t = G.guarded(src.transpose(0, 2), fill, band=SMALL)            # a non-contiguous source: the result is contiguous
        assert t.is_contiguous() and t.shape == (7, 5, 3) and t.dtype == dtype and torch.equal(t, src.transpose(0, 2))
        front, back = G.bands_of(t)
        assert front.numel() == SMALL and front.numel() % G.PAGE == 0 and back.numel() >= SMALL
        assert (t.data_ptr() - front.data_ptr()) == SMALL and front.data_ptr() % 64 == 0 and t.data_ptr() % 64 == 0
        assert bool((front == fill).all()) and bool((back == fill).all())
        assert back.data_ptr() == t.data_ptr() + t.numel() * t.element_size()      # the back band starts at the operand's last byte + 1
    with pytest.raises(ValueError):
        G.guarded(src, G.FILL_NAN, band=1000)                           # would misalign the operand


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn], ids=str)
def test_guarded_random_draws_the_payload_in_place_between_intact_bands(dtype, monkeypatch):
    """The device-side placement of tests/test_size_limits_gpu.py, here on the CPU and with a chunk smaller than the payload: bands as
    ``guarded`` makes them, every chunk drawn (none left holding the fill), no value repeated with a period, the same draw from the same
    seed under either fill, the clamp honoured."""
    monkeypatch.setattr(G, "RANDOM_CHUNK", 1000)
    draws = {}
    for fill in G.FILLS:
        g = torch.Generator().manual_seed(5)
        t = G.guarded_random((3, 29, 37), dtype, fill, g, scale=2.0, limit=3.0, band=SMALL)
        assert t.shape == (3, 29, 37) and t.dtype == dtype and t.is_contiguous()
        G.assert_bands_intact([("t", t)], fill, "guarded_random")
        front, _ = G.bands_of(t)
        assert front.numel() == SMALL and t.data_ptr() % 64 == 0
        v = t.float()
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) <= 3.0 and float(v.abs().max()) > 2.0
        flat = v.view(-1)
        assert not torch.equal(flat[:1000], flat[1000:2000]) and not torch.equal(flat[:1024], flat[1024:2048])
        assert len(torch.unique(flat[-219:])) > 8             # the last, short chunk was drawn too
        draws[fill] = G.bits(t).clone()
    assert torch.equal(draws[G.FILL_NAN], draws[G.FILL_BIG])


def _header_ops():
    """Every r50_op_* prototype of include/r50.h, the two forward entry points and the stem's scratch-size query."""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "r50.h").read_text(), flags=re.S)
    names = re.findall(r"^\s*(?:int|int64_t|size_t)\s+(r50_\w+)\s*\(", text, flags=re.M)
    assert len(names) == len(set(names)) and "r50_create" in names
    keep = [n for n in names if n.startswith("r50_op_") or n in ("r50_forward", "r50_forward_u8", "r50_stem_scratch_bytes")]
    assert len(keep) >= 60 and "r50_op_avgpool" in keep and "r50_op_nn_search_workspace" in keep
    return keep


def test_every_op_of_the_header_has_a_guard_band_row():
    """A new op fails here until a row of tests/rows/r50.py runs it between guard bands.  NOT_GUARDED is for entry points that take no
    device operand, and for nothing else."""
    from tests.rows import r50 as T
    covered = set()
    for row in T.ROWS:
        covered.update(row.ops)
    header = _header_ops()
    assert covered <= set(header), f"rows name ops the header does not have: {sorted(covered - set(header))}"
    missing = [n for n in header if n not in covered and n not in T.NOT_GUARDED]
    assert not missing, f"no guard-band row for: {missing}"
    for name, reason in T.NOT_GUARDED.items():
        assert name in header and name not in covered, name
        assert "no device operand" in reason, f"{name}: {reason!r}"
    ids = [row.id for row in T.ROWS]
    assert len(ids) == len(set(ids)), "row ids must be unique"
