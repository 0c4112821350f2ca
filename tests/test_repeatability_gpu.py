"""Every op holds its bits run after run, alone and under contention.

The harness is tests/repeatability.py (read its docstring first).  Every row of every guard-band table (``ALL_ROWS`` of
tests/rows/) runs once plainly and then R times per mode, from the same payloads, every run with fresh 0xFF-poisoned
outputs between 0xFF bands:

  hot rows    the rows whose ``ops`` reach a hand-synchronised kernel (``repeatability.HAND_SYNCED``), and the op-level stem: R = 16 in
              each of ``quiet``, ``noise_mem``, ``noise_mfma`` and ``twin``.
  plain rows  every other row (``__syncthreads()`` and fixed-order trees; their headers make the same promise): R = 2 in ``quiet`` and
              ``twin``.  ``twin`` also catches a hidden workspace shared by two concurrent calls of one op.

Asserted, exactly: every output and in-out of every repetition holds the bits of the plain run; no defined output element still holds the
fill; every band of every operand of every repetition is intact after the last one.  No shape and no tolerance of its own: the plain run
is what every other test holds to its fp64 or oracle reference.

A repetition under noise counts only if the burst ended after the row did, a twin repetition only if the two copies' event intervals
intersect.  A hot row in which more than a quarter of the repetitions did not overlap fails with that reason, in every mode; a plain row
fails if none of its twin repetitions overlapped (at R = 2 a quarter is less than one repetition): a row that never ran beside its twin
says nothing about a shared workspace.  A row whose op synchronises the host before it launches (``BLOCKS_HOST`` of
tests/stream_order.py: ``r50_op_stem``, ``r50_op_resize_frames_u8``) gets a host thread per copy, under the same bars.  For
those rows the interval of a copy spans its upload or read-back, the host synchronisation and the kernels: the events show that the
two calls were inside the library at the same time and how far apart they ended (printed), not that the kernels themselves coincided.
``test_every_mode_overlapped`` prints the shares.

Process-wide options (``cu_cap``, ``stem_strip``, ``tail3_bp``) must read 0 when a test ends.  The cap combined with noise is not tried.

Measured on an MI355X, one session: see DESIGN.md section 4, "Repeatability".
"""
import pytest

from tests import guard_bands as G
from tests import repeatability as RP
from tests.guard_bands import _checks_fill, close_payloads
from tests.rows import ALL_ROWS
from tests.stream_order import may_block

pytestmark = pytest.mark.gpu

HOT_ROWS = [r for r in ALL_ROWS if RP.is_hot(r)]
PLAIN_ROWS = [r for r in ALL_ROWS if not RP.is_hot(r)]
KNOBS = ("cu_cap", "stem_strip", "tail3_bp")
OVERLAP = {}                # (row id, mode) -> (repetitions that overlapped, repetitions, the row's device ms, hot, the mode's note)


@pytest.fixture(scope="module")
def knob_handle(lib_built):
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    bb = ResNet50Backbone(seed=0, max_batch=1).to("cuda:0").eval()
    try:
        yield bb
    finally:
        for k in KNOBS:
            bb.set_option(k, 0)
        bb.close()


@pytest.fixture(autouse=True)
def knobs_read_zero_when_a_test_ends(knob_handle):
    yield
    left = {k: knob_handle.get_option(k) for k in KNOBS}
    for k in KNOBS:                                   # a failing test must not leave the rest of the GPU suite capped
        knob_handle.set_option(k, 0)
    assert all(v == 0 for v in left.values()), f"a test left process-wide knobs set: {left}"


def holds_host(row):
    """The row's op synchronises the host before it launches (``BLOCKS_HOST`` of tests/stream_order.py, which tests/test_stream_order_gpu.py holds
    exact: a row outside it that holds the host fails there, and so does a stale entry)."""
    return may_block(row)


def hold_row(row, mode, reps, hot):
    lib = G.lib()
    payloads, payloads2 = row.make(), None
    try:
        plain = RP.plain_run(row, payloads)
        dev_ms, host_ms = RP.timed_run(row, payloads, plain.spec)
        if mode == "quiet":
            runs = RP.run_quiet(row, payloads, plain.spec, reps)
        elif mode in RP.NOISE_MODES:
            session = RP.burst_ms(lib, HOT_ROWS)
            assert 4 * dev_ms <= 1.25 * session, (f"{row.id}: one run takes {dev_ms:.3f} ms on the device, against {session / RP.BURST_FACTOR:.3f} ms for "
                                                  f"{RP.MEASURED_SLOWEST_ROW[0]}: this row is now the slowest, record it in MEASURED_SLOWEST_ROW")
            burst = max(session, 4 * dev_ms)            # never less than four times this very row
            runs = RP.run_noisy(row, payloads, plain.spec, reps, mode, lib, burst)
        else:
            payloads2 = row.make() if RP.carries_state(row, payloads) else None
            runs = RP.run_twin(row, payloads, payloads if payloads2 is None else payloads2, plain.spec, reps, lib, host_ms,
                               two_threads=holds_host(row))
    finally:
        close_payloads(payloads)
        close_payloads(payloads2)
    what = f"{row.id} {mode}"
    for label, a in runs.arenas:
        a.finish()
        assert list(a.results) == list(plain.results), f"{what}: result names differ between {label} and the plain run"
        for name, want in plain.results.items():
            RP.assert_same_bits(what, name, label, a.results[name], want)
            if a.defined.get(name) and _checks_fill(want, a.fill):
                n = G.holds_fill(a.results[name], a.fill)
                assert n == 0, f"{what}: {n} of {want.numel()} elements of output `{name}` of {label} still hold the fill pattern"
    for label, a in runs.arenas:
        G.assert_bands_intact(a.operands, a.fill, f"{what}, {label}")
    if runs.overlap is not None:
        good, n = sum(runs.overlap), len(runs.overlap)
        OVERLAP[(row.id, mode)] = (good, n, dev_ms, hot, runs.note)
        print(f"repeatability {what}: {good} of {n} repetitions overlapped; one run takes {dev_ms:.3f} ms on the device; {runs.note}")
        if hot:
            assert RP.enough_overlap(runs.overlap), (f"{what}: only {good} of {n} repetitions overlapped ({runs.detail}): the row has not been "
                                                     "tested under this mode")
        else:
            assert good > 0, f"{what}: none of {n} repetitions overlapped ({runs.detail}): the row never ran beside its twin"


def _params(rows, modes):
    return pytest.mark.parametrize("row,mode", [(r, m) for r in rows for m in modes], ids=[f"{r.id}-{m}" for r in rows for m in modes])


@_params(HOT_ROWS, RP.MODES)
def test_hot_rows_hold_their_bits(row, mode):
    hold_row(row, mode, RP.R_HOT, True)


@_params(PLAIN_ROWS, ("quiet", "twin"))
def test_plain_rows_hold_their_bits(row, mode):
    hold_row(row, mode, RP.R_PLAIN, False)


def test_every_mode_overlapped():
    """Runs after the tables (pytest keeps file order) and fails if they did not: per mode the share of repetitions that overlapped, the
    slowest row and the row with the least overlap, and once more the bar for every row that ran."""
    assert set(RP.kernels_reached(HOT_ROWS)) == set(RP.HAND_SYNCED) and all(RP.kernels_reached(HOT_ROWS).values())
    print(f"repeatability: {len(HOT_ROWS)} hot rows, {len(PLAIN_ROWS)} plain rows")
    assert any(v[3] for v in OVERLAP.values()), "no hot row has run in this session: this test reports on the tables above it and must run after them"
    low = []
    for mode in RP.MODES[1:]:
        for hot in (True, False):
            seen = {k: v for k, v in OVERLAP.items() if k[1] == mode and v[3] == hot}
            if not seen:
                continue
            good, n = sum(v[0] for v in seen.values()), sum(v[1] for v in seen.values())
            slow = max(seen, key=lambda k: seen[k][2])
            worst = min(seen, key=lambda k: seen[k][0] / seen[k][1])
            print(f"repeatability {mode}, {'hot' if hot else 'plain'} rows: {good} of {n} repetitions overlapped ({100.0 * good / n:.1f} %) over "
                  f"{len(seen)} rows; slowest row {slow[0]} ({seen[slow][2]:.3f} ms); least overlap {worst[0]} "
                  f"({seen[worst][0]} of {seen[worst][1]}; {seen[worst][4]})")
            if mode in RP.NOISE_MODES:
                tight = max(seen, key=lambda k: int(seen[k][4].split()[2]))
                print(f"repeatability {mode}: the tightest row is {tight[0]}: {seen[tight][4]}")
            if hot:
                low += [f"{k[0]} {mode}: {v[0]} of {v[1]}" for k, v in seen.items() if (v[1] - v[0]) > RP.MAX_NOT_OVERLAPPED * v[1]]
            else:
                low += [f"{k[0]} {mode}: {v[0]} of {v[1]}" for k, v in seen.items() if v[0] == 0]
    assert not low, f"rows under their overlap bar: {low}"
