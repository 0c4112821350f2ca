"""Ops on a side stream with late inputs -- test infrastructure for tests/test_stream_order_gpu.py and the per-header
tests/test_*_stream_order_gpu.py.

Every other op test runs on the legacy null stream with inputs that were complete before the call, and synchronises the device before it
looks.  That hides a launch that ignores its ``stream`` argument (it lands on the stream the test uses anyway), a fork to an internal
non-blocking stream without its event, and a host synchronisation inside an op.  ``LateArena`` has the interface of ``Arena`` in
tests/guard_bands.py, so every ``launch(arena, payloads)`` of the guard-band tables runs unchanged, but:

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
whole 50 ms, are the three ``BLOCKS_HOST`` below admits: ``resize_frames_u8`` (reads ``src_idx`` back) and
``stem-n1`` / ``stem-n3`` (``r50_op_stem`` uploads a host temporary).
"""
import functools
import json
import re
import time

import torch

from tests import guard_bands as G
from tests.guard_bands import DEV, Arena
from tests.helpers import GOLDEN

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


# ---- which rows may hold the host -------------------------------------------------------------------------------------------
# Rows (by id) or ops (by name: every row that launches it) that may hold the host until the side stream's sleep has ended.  The run on
# the MI355X added nothing to what reading r50_abi.hip gives: these three rows of 167 held the host (50 ms each, the whole sleep), no other
# row more than 2.4 ms.  hipMallocAsync / hipFreeAsync in r50_op_bneck_tail and r50_op_bneck_cat_chain do not hold it.
BLOCKS_HOST = {
    "r50_op_resize_frames_u8": "copies src_idx to the host and synchronises the stream before it launches",
    "r50_op_stem": "uploads the packed host weights and synchronises the stream (the packed image is a host temporary)",
}

# backbone_launch_plan.json counts launches by kind; the op-level entry point(s) of each kind.  "conv1" and "stem_pack" are the stem's two
# kernels, which r50_forward launches from the handle's resident weights: the op-level r50_op_stem is a test entry point that packs and uploads
# host weights on every call, and no per-step path calls it.
PLAN_KIND_OPS = {"avgpool": ("r50_op_avgpool",), "bneck_block2": ("r50_op_bneck_block2",), "bneck_catchain": ("r50_op_bneck_cat_chain",),
                 "bneck_tail": ("r50_op_bneck_tail",), "bneck_tail3": ("r50_op_bneck_tail",), "conv1": (), "stem_pack": (),
                 "igemm": ("r50_op_conv2d", "r50_op_conv2d_f16", "r50_op_conv2d_w2", "r50_op_conv2d_split", "r50_op_conv2d_fp8", "r50_op_conv1x1_cat",
                           "r50_op_bneck_block1", "r50_op_bneck_block1_ds"),
                 "maxpool": ("r50_op_maxpool",)}


def hot_path_ops():
    """The ops of the per-step hot paths: every op a recorded train step launches (the fp16 head's GEMMs are recorded under
    ``r50_op_conv2d``), every launch kind of the backbone's plan, and the forward itself."""
    train = json.loads((GOLDEN / "train_launch_sequences.json").read_text())
    ops = {re.match(r"r50_op_\w+", what).group(0) for seq in train["sequences"].values() for what in seq}
    ops.add("r50_op_conv2d_f16")
    plan = json.loads((GOLDEN / "backbone_launch_plan.json").read_text())
    kinds = {k for prec in plan["plans"].values() for entry in prec.values() for k in entry["launches"]}
    assert kinds <= set(PLAN_KIND_OPS), f"launch kinds without an op: {sorted(kinds - set(PLAN_KIND_OPS))}"
    for k in kinds:
        ops.update(PLAN_KIND_OPS[k])
    return ops | {"r50_forward", "r50_forward_u8"}


def may_block(row):
    return row.id in BLOCKS_HOST or any(op in BLOCKS_HOST for op in row.ops)


def check_blocking_table(rows):
    """The conditions on ``BLOCKS_HOST`` over ``rows``, the rows that run late (also asserted without a GPU by tests/test_stream_order_cpu.py)."""
    ids, ops = {row.id for row in rows}, {op for row in rows for op in row.ops}
    for key, reason in BLOCKS_HOST.items():
        assert key in ids or key in ops, f"BLOCKS_HOST names `{key}`, which is neither a row nor an op of a row"
        assert reason.strip(), f"BLOCKS_HOST[{key}] gives no reason"
    hot = hot_path_ops()
    listed = [row for row in rows if may_block(row)]
    for row in listed:
        bad = sorted(set(row.ops) & hot)
        assert not bad, f"BLOCKS_HOST admits row {row.id}, which launches hot-path op(s) {bad}: an op of a per-step path must not hold the host"
    assert len(listed) * 10 <= len(rows), f"BLOCKS_HOST admits {len(listed)} of {len(rows)} rows: more than 10 %"


# ---- the runners: a row, and a Python entry point, late on the side stream against the default stream -----------------------
def run_row_late(row):
    side, _ = choose_stream(G.lib())
    payloads = row.make()
    try:
        plain = Arena(None)
        row.launch(plain, payloads)
        torch.cuda.synchronize()
        if row.scrub is not None:
            row.scrub(payloads)        # a handle's buffers must not still hold what these very payloads left there
        late = LateArena(side, calibrate())
        with torch.cuda.stream(side):
            row.launch(late, payloads)
            late.finish()
    finally:
        G.close_payloads(payloads)
    print(f"stream_order row {row.id}: host {late.enqueue_ms:.2f} ms from the first inp to launch returning, blocked {late.blocked}")
    assert plain.results and list(late.results) == list(plain.results), f"{row.id}: result names differ between the runs"
    for name, want in plain.results.items():
        assert_same_bits(row.id, name, "snapshot", late.snapshots[name], want)
        assert_same_bits(row.id, name, "final tensor", late.results[name], want)
        if late.defined.get(name) and G._checks_fill(want, late.fill):
            n = G.holds_fill(late.snapshots[name], late.fill)
            assert n == 0, f"{row.id}: {n} of {want.numel()} elements of output `{name}` still hold the poison in the snapshot"
    if late.blocked and not may_block(row):
        raise AssertionError(f"{row.id}: the host was held until the side stream's sleep had ended ({late.enqueue_ms:.1f} ms): either it "
                             "synchronises the host, or the sleep is too short: see calibrate()")
    if may_block(row) and not late.blocked:
        raise AssertionError(f"{row.id}: listed in BLOCKS_HOST, but it did not hold the host: the entry is stale")


def _tensors_of(result):
    """name -> tensor for whatever a wrapper returned: a tensor, a tuple of tensors (None entries left out) or a dict."""
    if isinstance(result, torch.Tensor):
        return {"result": result}
    if isinstance(result, dict):
        return {str(k): v for k, v in result.items() if isinstance(v, torch.Tensor)}
    return {f"result[{i}]": v for i, v in enumerate(result) if isinstance(v, torch.Tensor)}


def side_against_default(what, call, inputs, scrub=None):
    """``call(late, tensors)`` once on the default stream (late = None) and once under ``with torch.cuda.stream(S)`` (late = the ``LateArena``)
    with every tensor of ``inputs`` produced late on ``S``: behind the sleep, by a device copy from staging.  Whatever tensors it returns are
    snapshot on ``S`` right after the call; snapshot bits == final bits == default-stream bits.  Returns the late arena (``blocked`` tells
    whether the wrapper held the host, which a wrapper that reads a result on the host does by design).  ``scrub()`` runs between the two:
    an object with cached workspaces (a head, a backbone handle) gets another batch, so that a launch which read a workspace too early
    would not find there what the same inputs left a moment ago."""
    side, _ = choose_stream(G.lib())
    want = _tensors_of(call(None, {k: v.to(DEV) for k, v in inputs.items()}))
    torch.cuda.synchronize()
    if scrub is not None:
        scrub()
        torch.cuda.synchronize()
    late = LateArena(side, calibrate())
    with torch.cuda.stream(side):
        got = _tensors_of(call(late, {k: late.inp(k, v) for k, v in inputs.items()}))
        late.results.update(got)
        late.finish()
    assert want and list(got) == list(want), f"{what}: result names differ between the runs"
    for name, w in want.items():
        assert_same_bits(what, name, "snapshot", late.snapshots[name], w)
        assert_same_bits(what, name, "final tensor", late.results[name], w)
    print(f"stream_order wrapper {what}: host {late.enqueue_ms:.2f} ms, blocked {late.blocked}")
    return late
