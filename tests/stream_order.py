"""Ops on a side stream with late inputs -- test infrastructure for tests/test_stream_order_gpu.py.

Every other op test runs on the legacy null stream with inputs that were complete before the call, and synchronises the device before it
looks.  That hides a launch that ignores its ``stream`` argument (it lands on the stream the test uses anyway), a fork to an internal
non-blocking stream without its event, and a host synchronisation inside an op.  ``LateArena`` has the interface of ``Arena`` in
tests/test_guard_bands_gpu.py, so every ``launch(arena, payloads)`` of the guard-band tables runs unchanged, but:

  * the row runs on a side stream ``S`` of torch's pool (``with torch.cuda.stream(S)``);
  * every input is NOT there yet when the op is enqueued: the operand holds a stale value (NaN in every float format, 255 as uint8, 0 in
    an index table so that a stale index stays in range), and the true payload arrives by a device-to-device copy on ``S`` that sits
    behind a ``torch.cuda._sleep``.  An op that reads its input anywhere but in ``S``'s order reads the stale value.  This input-side check
    is deterministic: the host enqueues the whole row in a fraction of the sleep, so the stale value is provably still there;
  * ``finish()`` notes whether the host was held until the sleep ended (``blocked``: the op, or the row, synchronised the host), clones every
    result on ``S`` (the snapshots: what the caller's next kernel on ``S`` would read), overwrites every pure input on ``S`` with its stale
    value again (what the caller's next kernel might do), and only then synchronises the device.

The snapshot against the final tensor (a missing join on the write side) and the overwritten inputs (a straggler on an internal stream
that still reads after the op's place in ``S``'s order) are races: they can only fail, never prove.

The runtime multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES), and a side stream that shares the null stream's queue
runs behind it: a launch misdirected to stream 0 would then still see its input.  ``choose_stream`` therefore takes the first stream of
torch's pool on which such a launch provably runs during the sleep (``BackboneLanes._pick_streams`` has the same concern), and fails if 24
candidates give none.

Measured on an MI355X, one session, host time from the first ``inp`` to ``launch`` returning over the 164 rows that do not hold the host:
the slowest is head_gemm row ``fp16-dw_m1024_k64_n3072`` with 2.37 ms (three igemm tiles, staging included); every other row is below
2.3 ms.  Four times that is 9.5 ms, so the sleep stays at the 50 ms it started with (21 times the slowest row; the cap is 200 ms).
``choose_stream`` and ``choose_second_stream`` both took the first candidate in that session.  The rows that held the host, each for the
whole 50 ms, are the three ``BLOCKS_HOST`` of tests/test_stream_order_gpu.py admits: ``resize_frames_u8`` (reads ``src_idx`` back) and
``stem-n1`` / ``stem-n3`` (``r50_op_stem`` uploads a host temporary).
"""
import functools
import time

import torch

from tests import guard_bands as G
from tests.test_guard_bands_gpu import DEV, Arena

U8 = torch.uint8
INDEX_TYPES = (torch.int32, torch.int64)
MAX_CANDIDATES = 24

MEASURED_SLOWEST_ROW = ("fp16-dw_m1024_k64_n3072", 2.37)          # (row id, host ms from the first inp to launch returning)
SLEEP_MS = 50.0


def stale_like(t: torch.Tensor, device=DEV) -> torch.Tensor:
    """A tensor on ``device`` of ``t``'s shape and dtype holding the stale value: 0xFF in every byte (NaN as any float, 255 as uint8), 0 for the
    index types -- a stale index table stays in range, so a bug shows up as a wrong result and never as an out-of-bounds access."""
    if t.dtype in INDEX_TYPES:
        return torch.zeros(t.shape, dtype=t.dtype, device=device)
    nbytes = t.numel() * t.element_size()
    return torch.full((nbytes,), G.FILL_NAN, dtype=U8, device=device).view(t.dtype).view(t.shape)


def poisoned(shape, dtype, device=DEV) -> torch.Tensor:
    """An output or workspace whose every byte is 0xFF, as ``guarded_empty`` pre-fills its payload.  No bands: their placement is the
    guard-band tests' job."""
    shape = tuple(int(v) for v in shape)
    numel = 1
    for v in shape:
        numel *= v
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), G.FILL_NAN, dtype=U8, device=device).view(dtype).view(shape)


def restale_(t: torch.Tensor) -> None:
    """Overwrite ``t`` with its stale value on the current stream (no allocation, no host data)."""
    if t.dtype in INDEX_TYPES:
        t.zero_()
    else:
        t.view(-1).view(U8).fill_(G.FILL_NAN)


@functools.lru_cache(maxsize=None)
def calibrate(ms: float = SLEEP_MS) -> int:
    """The ``torch.cuda._sleep`` cycle count that lasts ``ms`` milliseconds: two sleeps timed with events, once per session."""
    n = 20_000_000
    torch.cuda._sleep(1000)                                 # the first use loads the spin kernel
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(n)
    torch.cuda._sleep(n)
    b.record()
    torch.cuda.synchronize()
    per_cycle = a.elapsed_time(b) / (2 * n)
    assert per_cycle > 0, "torch.cuda._sleep took no time"
    return int(ms / per_cycle)


class LateArena(Arena):
    """The operands of one run on the side stream ``stream`` with late inputs (see the module docstring).  Use inside
    ``with torch.cuda.stream(stream)``; call ``finish()`` right after ``row.launch`` returns."""

    def __init__(self, stream: "torch.cuda.Stream", cycles: int):
        super().__init__(None)
        self.fill = G.FILL_NAN                  # the poison of outputs and workspaces (``_checks_fill``)
        self.stream, self.cycles = stream, int(cycles)
        self.sleep_done = None
        self.inputs = []                        # (name, operand): everything that arrived late
        self.staging = []                       # kept alive until the device is synchronised
        self.snapshots = {}
        self.blocked = None
        self.enqueue_ms = None
        self._t0 = None
        self._deferred = []

    def _on_default(self, make):
        default = torch.cuda.default_stream()
        with torch.cuda.stream(default):
            made = make()
            default.synchronize()               # that stream only: the side stream may be asleep
        return made

    def inp(self, name, t):
        src = t.detach().contiguous()
        if self._t0 is None:
            self._t0 = time.perf_counter()
        staged, operand = self._on_default(lambda: (src.to(DEV, copy=True), stale_like(src)))   # never a pageable copy on the side stream
        self.staging.append(staged)
        with torch.cuda.stream(self.stream):
            if self.sleep_done is None:
                torch.cuda._sleep(self.cycles)
                self.sleep_done = torch.cuda.Event()
                self.sleep_done.record(self.stream)
            operand.copy_(staged, non_blocking=True)
        self.inputs.append((name, operand))
        return self._put(name, operand)

    def out(self, name, shape, dtype, defined=True):
        t = self._on_default(lambda: poisoned(shape, dtype))
        self.results[name] = self._put(name, t)
        self.defined[name] = defined
        return t

    def ws(self, name, shape, dtype):
        return self._put(name, self._on_default(lambda: poisoned(shape, dtype)))

    def between_calls(self, fn):
        """A row with state of its own puts another batch through it between two calls on the same inputs; enqueued on the side stream,
        without a host synchronisation."""
        fn()

    def host_check(self, fn):
        """A row's own look at a result on the host: here after ``finish()``, so that the look itself does not hold the host."""
        self._deferred.append(fn)

    def finish(self, overwrite_inputs=True):
        assert self.sleep_done is not None, "the row has no input"
        self.blocked = bool(self.sleep_done.query())
        self.enqueue_ms = (time.perf_counter() - self._t0) * 1e3
        pure = [(n, t) for n, t in self.inputs if all(t is not r for r in self.results.values())]
        with torch.cuda.stream(self.stream):
            self.snapshots = {name: t.clone() for name, t in self.results.items()}
            for _name, t in pure if overwrite_inputs else ():
                restale_(t)
        torch.cuda.synchronize()
        for fn in self._deferred:
            fn()
        return self


def assert_same_bits(what, name, which, got, want):
    """``got`` (the ``which`` -- snapshot or final tensor -- of result ``name`` on the side stream) holds the bits of ``want``, the
    default-stream run: integer views, so NaN payloads and -0 count."""
    a, b = G.bits(got), G.bits(want)
    assert a.shape == b.shape and a.dtype == b.dtype, (f"{what}: the {which} of `{name}` on the side stream is {tuple(got.shape)} {got.dtype}, the "
                                                       f"default-stream run gave {tuple(want.shape)} {want.dtype}")
    if not torch.equal(a, b):
        bad = torch.nonzero((a != b).view(-1))
        raise AssertionError(f"{what}: the {which} of `{name}` on the side stream differs from the default-stream run in {bad.numel()} of "
                             f"{a.numel()} elements, the first at flat index {int(bad[0])}")


def cast_rows_probe(lib, stream, cycles, how, other=None):
    """``r50_op_cast_rows`` (fp32 -> bf16, 40 rows x 64: the bf16 conversion keeps a NaN, the fp16 one saturates it away) with a late input on ``stream``.  how = "honest": the op gets ``stream``'s handle;
    "stream0": handle 0, a launch that ignores its stream; "no_join": the op runs on ``other`` behind an event recorded on ``stream`` after
    the input copy and behind a sleep of its own, and nothing makes ``stream`` wait for ``other``.  Reads NaN floats and writes its own
    output: nothing here can fault.  Returns (arena, bits of the same op on the default stream)."""
    rows, c = 40, 64
    x = torch.randn((rows, c), generator=torch.Generator().manual_seed(4064)) * 3.0

    def operands(a):
        return a.inp("src", x), a.out("dst", (rows, c), torch.bfloat16)

    plain = Arena(None)
    src, dst = operands(plain)
    rc = lib.r50_op_cast_rows(src.data_ptr(), rows, c, dst.data_ptr(), c, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.r50_last_error(None)
    torch.cuda.synchronize()
    want = G.bits(dst).clone()

    late = LateArena(stream, cycles)
    with torch.cuda.stream(stream):
        src, dst = operands(late)
        if how == "no_join":
            ev = torch.cuda.Event()
            ev.record(stream)                   # behind the input copy
            other.wait_event(ev)
            with torch.cuda.stream(other):
                torch.cuda._sleep(cycles)
            handle = other.cuda_stream
        else:
            handle = {"honest": stream.cuda_stream, "stream0": 0}[how]
        rc = lib.r50_op_cast_rows(src.data_ptr(), rows, c, dst.data_ptr(), c, 0, handle)
        assert rc == 0, lib.r50_last_error(None)
        late.finish(overwrite_inputs=how != "no_join")      # the unjoined op is to write the true result, late
    return late, want


def _misdirected_launch_shows(lib, stream, cycles) -> bool:
    late, want = cast_rows_probe(lib, stream, cycles, "stream0")
    snap = late.snapshots["dst"]
    return (not late.blocked) and bool(torch.isnan(snap).any()) and not torch.equal(G.bits(snap), want)


_CHOSEN = {}


def choose_stream(lib):
    """(stream, candidates tried): the first stream of torch's pool on which a launch misdirected to stream 0 provably runs during the
    sleep.  One choice per session; fails (never skips) if ``MAX_CANDIDATES`` candidates give none."""
    if "side" not in _CHOSEN:
        cycles = calibrate()
        for tried in range(1, MAX_CANDIDATES + 1):
            cand = torch.cuda.Stream(DEV)
            if _misdirected_launch_shows(lib, cand, cycles):
                _CHOSEN["side"] = (cand, tried)
                print(f"stream_order.choose_stream: candidate {tried} of {MAX_CANDIDATES} runs beside the null stream")
                break
        else:
            raise AssertionError(f"choose_stream: none of {MAX_CANDIDATES} pool streams ran a null-stream launch during the sleep: every one "
                                 "of them shares the null stream's hardware queue, and the stream-order tests would see nothing")
    return _CHOSEN["side"]


def choose_second_stream(lib):
    """(stream, candidates tried): a second pool stream that runs beside the chosen one -- on which the same op, issued without a join,
    provably has not written its output when the chosen stream takes its snapshot."""
    if "second" not in _CHOSEN:
        side, _ = choose_stream(lib)
        cycles = calibrate()
        for tried in range(1, MAX_CANDIDATES + 1):
            cand = torch.cuda.Stream(DEV)
            if cand.cuda_stream == side.cuda_stream:
                continue
            late, _want = cast_rows_probe(lib, side, cycles, "no_join", other=cand)
            if G.holds_fill(late.snapshots["dst"], late.fill) == late.snapshots["dst"].numel():
                _CHOSEN["second"] = (cand, tried)
                print(f"stream_order.choose_second_stream: candidate {tried} of {MAX_CANDIDATES} runs beside the chosen stream")
                break
        else:
            raise AssertionError(f"choose_second_stream: none of {MAX_CANDIDATES} pool streams ran beside the chosen side stream")
    return _CHOSEN["second"]
