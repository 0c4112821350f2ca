"""Every kernel between poisoned guard bands: its result is a function of its operands' bytes alone, and it writes its outputs and
nothing else.

The convolution, body, head and evaluation kernels address memory through a buffer descriptor + a per-lane voffset + a scalar soffset and
count on the hardware range check (which looks at voffset only) to return zeros for padding taps, rows past M, queries past nq and rows
past n; the conv descriptors start x_back bytes in front of x.  An index mistake in a halo, a ragged last tile, a causal clamp at t = 0,
a t0 / i0 offset or a last window therefore does not fault: it reads what lies next to the operand, which under a caching allocator is
mapped, finite, leftover data.  Here every operand of a call -- inputs, weights, biases, residuals, index tables, outputs, in-outs and
workspaces -- is placed between two bands of tests/guard_bands.py, and each row of tests/rows/r50.py runs three times from the same seeded
payloads (``run_row`` of tests/guard_bands.py):

  1. plain: ordinary separate tensors, as every other test runs the op;
  2. every operand between 0xFF bands (NaN in every float format, -1 as int32);
  3. every operand between 0x7B bands (large, finite, positive: the fill that survives a ReLU, fmax or fmin).

Asserted, exactly: outputs and in-outs are the same BITS in the three runs (integer views: NaN payloads and -0 count); every band of
every operand is intact after runs 2 and 3; an output whose every element the op defines holds no element of the fill pattern (an output's
payload starts out as fill).  Workspaces (only buffers the header documents as scratch) get the band check alone.

The bands are G.BAND bytes; each row states how far its kernel's unchecked arithmetic could reach (x_back, the largest soffset
displacement ((k-1) W + (k-1)) Cin 2 of a conv, one staged chunk of nn_search, one tile's rows times the row pitch) and the band is
asserted to be at least twice that.  Shapes come from the existing case lists, whose own tests hold the plain run to its oracle; a
row whose shape no other test runs carries a `check`, that family's own oracle check with its own bar, applied to the plain run.

What this cannot see: a stray uint8 read under a zero weight (the frame ops' rows are there for the nonzero-weight reads and for the
writes); and the activation arena inside an r50_handle: the
header has no op-level uint8 stem, so uint8 frames reach the stem through r50_forward_u8 alone, where x and out are guarded (at n = 1 and
n = 3) and the stem's own output and scratch, like every other activation of the network, are the handle's and are not.  tests/test_guard_bands_cpu.py proves the harness on toy kernels and holds this table complete.
Every payload here keeps the allocator's alignment; operands at the least alignment each op admits are tests/test_alignment_gpu.py's
(the same rows between the same bands, shifted; DESIGN.md section 4, "Pointer alignment").
"""
import pytest
import torch

from tests import guard_bands as G
from tests.guard_bands import DEV, F32, PAYLOAD, _toy_reads_one_before_then_relu, _toy_writes_one_past, run_row
from tests.rows.r50 import ROWS

pytestmark = pytest.mark.gpu


def _family(family):
    rows = [r for r in ROWS if r.family == family]
    return pytest.mark.parametrize("row", rows, ids=[r.id for r in rows])


# ------------------------------------------------------------------------------------------------------------------------------
@_family("igemm")
def test_igemm_every_tile(row):
    run_row(row)


@_family("special_conv")
def test_shape_specialised_convs(row):
    run_row(row)


@_family("head_gemm")
def test_head_gemms_every_tile(row):
    run_row(row)


@_family("pair_fp8_cat")
def test_pair_fp8_and_two_source_convs(row):
    run_row(row)


@_family("fused")
def test_fused_bodies_and_tails(row):
    run_row(row)


@_family("stem_pools_network")
def test_stem_pools_network(row):
    run_row(row)


@_family("frames")
def test_frame_ops(row):
    run_row(row)


@_family("head")
def test_head_ops(row):
    run_row(row)


@_family("losses")
def test_losses(row):
    run_row(row)


@_family("evaluation")
def test_evaluation_ops(row):
    run_row(row)


def test_the_harness_detects_on_the_device_what_it_detects_on_the_cpu():
    """The toy kernels of tests/guard_bands.py (plain torch on as_strided views; tests/test_guard_bands_cpu.py runs them on the CPU) on device arenas: the stray read behind a ReLU is
    missed by 0xFF and caught by 0x7B, the stray write is caught by the band check -- so a green table above is not a blind one."""
    benign, plain = torch.zeros(7, device=DEV), torch.zeros(7, device=DEV)
    benign[1:-1] = PAYLOAD.to(DEV)
    _toy_reads_one_before_then_relu(benign[1:-1], plain[1:-1])
    same = {}
    for fill in G.FILLS:
        x = G.guarded(PAYLOAD, fill, device=DEV)
        assert x.is_cuda and G.bands_of(x)[0].numel() == G.BAND and x.data_ptr() - G.bands_of(x)[0].data_ptr() == G.BAND
        y = G.guarded_empty(PAYLOAD.shape, F32, fill, device=DEV)
        _toy_reads_one_before_then_relu(x, y)
        same[fill] = torch.equal(G.bits(y), G.bits(plain[1:-1]))
        G.assert_bands_intact([("x", x), ("y", y)], fill)
        _toy_writes_one_past(x, y)
        with pytest.raises(AssertionError, match="behind `y`"):
            G.assert_bands_intact([("x", x), ("y", y)], fill)
    assert same == {G.FILL_NAN: True, G.FILL_BIG: False}


def test_every_row_belongs_to_a_test():
    families = {"igemm", "special_conv", "head_gemm", "pair_fp8_cat", "fused", "stem_pools_network", "frames", "head", "losses", "evaluation"}
    assert {r.family for r in ROWS} == families
