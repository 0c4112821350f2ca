"""The same bits run after run, alone and under contention -- test infrastructure for tests/test_repeatability_gpu.py and
tests/test_repeatability_cpu.py.

DESIGN.md, include/r50*.h and the kernel comments promise "the same bits on every run".  Every other test launches a row once on an idle
chip, synchronises and compares: a wait count one stage short, or a barrier on the wrong side of a fragment read, gives the right bits
whenever the LDS-DMA happens to land in time, which on an idle chip with one launch in flight is nearly always.  Here a row of the
guard-band tables (``ALL_ROWS`` of tests/rows/: ``make`` / ``launch`` / ``scrub``) runs R times per mode and every run is
held, bit for bit, to the plain run -- the run every other test holds to its fp64 or oracle reference, so bit equality carries those bars
over and no shape or tolerance of its own enters.

  plain run   ``plain_run``: ordinary tensors on the default stream under a ``SpecArena``, which also notes every operand the row asks for
              (kind, name, shape, dtype, payload) in order.
  the runs    ``ReplayArena`` builds every operand of a run from that list BEFORE anything is enqueued: inputs and in-outs from the same
              payloads (``row.make()``, once), outputs and workspaces pre-filled with 0xFF, everything between 0xFF bands
              (tests/guard_bands.py).  ``row.launch`` then only launches: no copy and no allocation of the harness falls into the window in
              which the noise runs.  A look at a result on the host (``host_check``) is put off until the mode is over.  After every run
              of a row with state of its own, ``row.scrub(payloads)``.
  quiet       R launches back to back on the default stream, nothing else running.
  noise_mem   the row runs on ``stream_order.choose_stream``'s stream while ``choose_second_stream``'s -- which provably runs beside it,
              on another hardware queue -- negates a 1 GiB fp32 buffer in place, kernel after kernel (``buf.mul_(-1)``: no LDS, four times
              the 256 MiB MALL, HBM and address-unit pressure).
  noise_mfma  the same with bf16 ``torch.mm`` on 4096 x 4096 operands (fp16 if bf16 is not usable): MFMA, LDS and occupancy pressure, so
              that workgroups which need 128-160 KB of LDS start late and in another order.
  twin        the row on both streams at once, each copy with its own arena (a row that carries a backbone handle builds its payloads
              twice).  Both copies start behind one gate -- a short ``torch.cuda._sleep`` on the default stream, whose event both
              streams wait for, so that both hear of it the same way -- and the host has enqueued both before either begins.  A row
              whose op synchronises the host before it launches (``r50_op_stem``, ``r50_op_resize_frames_u8``) gets a host thread per
              copy: one thread would enqueue the second copy when the first is all but over.

Overlap is shown, not assumed.  Per noise repetition: one noise kernel, an event behind it which the row's stream waits for, the rest of
the burst, the row; events behind the row and behind the burst.  The repetition counts only if the burst ended after the row did
(``overlapped``).  Per twin repetition the two copies' event intervals must intersect (``intervals_intersect``).  A row in which more
than a quarter of the repetitions did not overlap fails (``enough_overlap``): it has not been tested.

The burst is sized from a measurement.  ``burst_ms`` times, once per session, the device time of ``MEASURED_SLOWEST_ROW`` with events and
takes ``BURST_FACTOR`` times that, at least ``NOISE_MS``; a row gets a longer burst if four times its own device time is more, and a row
more than a quarter slower than the recorded one fails and says so.  Measured on an MI355X: the slowest hot row is
``features-features_u8-fp32x-n1-n3-max_batch4`` with 7.3 ms on the device (four forwards; every op-level row is below 0.5 ms); one
``noise_mem`` kernel lasts 0.359 ms (6 TB/s), one ``noise_mfma`` kernel 0.110 ms (1.26 PFLOP/s in bf16).  With a burst of four times the
slowest row (29.2 ms) every repetition overlapped, but that row ended when 99 % of the ``noise_mem`` burst was over: beside a stream
that saturates HBM the four forwards take four times as long (the fp8 network row reached 78 % of the ``noise_mfma`` burst).  Hence
``BURST_FACTOR`` = 6, about 44 ms: some 120 ``noise_mem`` or 400 ``noise_mfma`` kernels.  The overlap shares are in DESIGN.md section 4,
"Repeatability".

The detector can fail.  Two diagnostic builds of the library, from a copy of csrc/ outside the tree, that change only which values reach
the MFMAs, each against the 20 igemm and head_gemm rows at R = 16: (1) ``igemm_bf16_kernel`` without its per-step barrier is caught by
all four modes (15, 19, 15 and 17 of the 20 rows, nearly all at repetition 0); (2) ``igemm_ws_kernel`` with the loaders' steady-state
wait one stage short passes ``quiet`` (20 of 20) and ``twin`` (20 of 20) and is caught by ``noise_mem`` (7 rows, first at repetitions
0, 0, 1, 3, 3, 4 and 15) and by ``noise_mfma`` (3 rows, at repetitions 6, 10 and 14).  Hence the noise modes, and hence R = 16 and no less.

``HAND_SYNCED`` names the kernels whose barriers, wait counts or sleeps are placed by hand, with the entry points that reach each
(read off csrc/r50_abi.hip); a row is hot if its ``ops`` meet them.  ``scan_hand_synced`` finds the same set in csrc/*.h as source text
(our own C++ for our own idiom: ``__builtin_amdgcn_s_barrier``, an ``s_waitcnt`` in an asm statement, ``wait_vmcnt``,
``__builtin_amdgcn_s_sleep``, directly or through a ``__device__`` helper or a macro); tests/test_repeatability_cpu.py holds the two equal.
``__syncthreads()``, ``sched_barrier`` and the wave-level ``wave_barrier`` / ``fence`` are not hand-placed waits: the compiler sizes
them.  That leaves ``draw_skeletons_u8_kernel`` (``__syncthreads()`` only) out, and it would leave ``stem_fused3_kernel`` out too: its
one barrier per row pair is a ``__syncthreads()``.  It is a 12-wave pipeline all the same, so ``SYNCTHREADS_PIPELINES`` lists it by hand,
and the CPU test holds that list to the source as well.

What this cannot see: a race whose window none of the four modes opens; the contention of a D2H copy or an RCCL gather; and the cap on
workgroups (tests/test_work_distribution_gpu.py) combined with noise.
"""
import re
import threading
import time
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from tests import guard_bands as G
from tests.guard_bands import DEV, Arena

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "implementation_phd_lab_vision_amd" / "csrc"

MODES = ("quiet", "noise_mem", "noise_mfma", "twin")
NOISE_MODES = ("noise_mem", "noise_mfma")
R_HOT, R_PLAIN = 16, 2                  # the file takes more than four times tests/test_alignment_gpu.py's time: only the plain rows' R may give
MAX_NOT_OVERLAPPED = 0.25               # share of a row's repetitions that may fail to overlap

# (row id, device ms of one run with events) of the slowest hot row, MI355X, one session; ``burst_ms`` re-measures it every session
MEASURED_SLOWEST_ROW = ("features-features_u8-fp32x-n1-n3-max_batch4", 7.30)
BURST_FACTOR = 6                        # at 4 the slowest row ended when 99 % of the noise_mem burst was over (see above)
NOISE_MS = 4.0                          # the burst is never shorter
NOISE_MEM_BYTES = 1 << 30               # four times the MALL (256 MiB), 256 times one XCD's L2
NOISE_MM_N = 4096
GATE_MS = 0.2                           # twin: the gate sleeps this long plus 1.5 times the row's host enqueue time
THREAD_GATE_MS = 2.0                    # ... and this much longer where two host threads have to be started first

_FWD = ("r50_forward", "r50_forward_u8", "r50_forward_layer")
_CONV16 = ("r50_op_conv2d", "r50_op_conv2d_f16")
# kernel -> the entry points of include/r50.h that reach it (csrc/r50_abi.hip: launch_igemm_et, launch_igemm_fp8, launch_bneck_*,
# launch_stem_fused, r50_op_nn_search; run_stack for r50_forward*)
HAND_SYNCED: Dict[str, Tuple[str, ...]] = {
    "igemm_bf16_kernel": _CONV16 + ("r50_op_conv2d_w2", "r50_op_conv2d_split") + _FWD,
    "igemm_ws_kernel": _CONV16 + ("r50_op_conv2d_w2", "r50_op_conv2d_fp8", "r50_op_conv1x1_cat") + _FWD,
    "gemm8p_kernel": _CONV16 + ("r50_op_conv1x1_cat",) + _FWD,
    "conv3x3_c64_kernel": _CONV16 + _FWD,
    "conv3x3_xres_kernel": _CONV16 + _FWD,
    "conv3x3_s2_kernel": _CONV16 + _FWD,
    "bneck_tail2_kernel": ("r50_op_bneck_tail",) + _FWD,
    "bneck_tail3p_kernel": ("r50_op_bneck_tail",) + _FWD,
    "bneck_catchain_kernel": ("r50_op_bneck_cat_chain",) + _FWD,
    "bneck_block1_kernel": ("r50_op_bneck_block1", "r50_op_bneck_block1_ds") + _FWD,
    "bneck_block2_kernel": ("r50_op_bneck_block2",) + _FWD,
    "nn_search_kernel": ("r50_op_nn_search",),
    "stem_fused3_kernel": _FWD,
}
# Keys of HAND_SYNCED that the scan must NOT find: multi-wave pipelines whose one barrier per step is a ``__syncthreads()``.
SYNCTHREADS_PIPELINES = {
    "stem_fused3_kernel": "12 waves, one __syncthreads() per row pair between the packer waves and the conv waves",
}
# Entry points that are hot although they reach no kernel above.  r50_op_stem launches stem_pack_kernel and stem_conv_kernel
# (``__syncthreads()`` only; the fused stem is reached through r50_forward* alone), but it is the op-level stem and runs under noise too.
ALSO_HOT = {
    "r50_op_stem": "the op-level stem: two kernels with __syncthreads() only, held under noise like the fused stem of r50_forward",
}


def hot_ops() -> frozenset:
    return frozenset(op for ops in HAND_SYNCED.values() for op in ops) | frozenset(ALSO_HOT)


def is_hot(row) -> bool:
    return bool(set(row.ops) & hot_ops())


def kernels_reached(rows) -> Dict[str, List[str]]:
    """kernel of HAND_SYNCED -> the ids of the rows whose ``ops`` name one of its entry points."""
    return {k: [r.id for r in rows if set(r.ops) & set(eps)] for k, eps in HAND_SYNCED.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# the scan of csrc/*.h (source text only)
# ------------------------------------------------------------------------------------------------------------------------------
HAND_PLACED = re.compile(r"\b(?:__builtin_amdgcn_s_barrier|__builtin_amdgcn_s_sleep|__builtin_amdgcn_s_waitcnt|s_waitcnt|s_sleep|s_barrier)\b")
_IDENT = re.compile(r"[A-Za-z_]\w*")


def strip_comments(text: str) -> str:
    """Comments become blanks; line breaks stay, so a position still tells the line."""
    def blank(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    text = re.sub(r"/\*.*?\*/", blank, text, flags=re.S)
    return re.sub(r"//[^\n]*", blank, text)


def _matching(text: str, at: int, open_ch: str, close_ch: str) -> int:
    """The index just behind the bracket that closes the one at ``at``."""
    depth = 0
    for i in range(at, len(text)):
        c = text[i]
        if c == open_ch:
            depth += 1
        elif c == close_ch:
            depth -= 1
            if depth == 0:
                return i + 1
    raise ValueError(f"unbalanced {open_ch} at offset {at}")


class Function(NamedTuple):
    kind: str           # "global" | "device" | "macro"
    name: str
    body: str


def functions_of(text: str) -> List[Function]:
    """Every ``__global__`` / ``__device__`` function DEFINITION of ``text`` (comments already stripped) with its body, and every
    function-like or object-like ``#define`` with its replacement text."""
    out: List[Function] = []
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+([A-Za-z_]\w*)((?:[^\n\\]|\\\n|\\.)*)", text, flags=re.M):
        out.append(Function("macro", m.group(1), m.group(2)))
    for m in re.finditer(r"__(global|device)__", text):
        i, depth, name, last_ident = m.end(), 0, None, None
        while i < len(text):
            c = text[i]
            if c == "(":
                if depth == 0:
                    name = last_ident
                i = _matching(text, i, "(", ")")
                continue
            if c in ";=" or c == "{":
                break
            w = _IDENT.match(text, i)
            if w:
                last_ident = w.group(0)
                i = w.end()
                continue
            i += 1
        if i >= len(text) or text[i] != "{" or name is None or name.startswith("__"):
            continue                    # a declaration, a __device__ variable, or an attribute's own parentheses only
        end = _matching(text, i, "{", "}")
        out.append(Function(m.group(1), name, text[i:end]))
    return out


def scan_hand_synced(paths: Optional[Sequence[Path]] = None) -> Dict[str, List[str]]:
    """``__global__`` kernel -> why it counts as hand-synchronised: the builtins of ``HAND_PLACED`` in its body, and the ``__device__``
    helpers and macros it names that contain one (directly or through another helper)."""
    paths = sorted(CSRC.glob("*.h")) if paths is None else list(paths)
    fns: List[Function] = []
    for p in paths:
        fns += functions_of(strip_comments(Path(p).read_text()))
    direct = {f.name: sorted(set(HAND_PLACED.findall(f.body))) for f in fns}
    helpers = {f.name for f in fns if f.kind != "global" and direct[f.name]}
    grew = True
    while grew:                         # a helper or macro that names a synchronising helper synchronises too
        grew = False
        for f in fns:
            if f.kind != "global" and f.name not in helpers and any(re.search(rf"\b{re.escape(h)}\b", f.body) for h in helpers):
                helpers.add(f.name)
                grew = True
    found: Dict[str, List[str]] = {}
    for f in fns:
        if f.kind != "global":
            continue
        why = list(direct[f.name]) + sorted(h for h in helpers if re.search(rf"\b{re.escape(h)}\b", f.body))
        if why:
            found[f.name] = sorted(set(found.get(f.name, []) + why))
    return found


def global_kernels(paths: Optional[Sequence[Path]] = None) -> Dict[str, str]:
    """``__global__`` kernel -> its body (comments stripped), over csrc/*.h."""
    paths = sorted(CSRC.glob("*.h")) if paths is None else list(paths)
    return {f.name: f.body for p in paths for f in functions_of(strip_comments(Path(p).read_text())) if f.kind == "global"}


# ------------------------------------------------------------------------------------------------------------------------------
# the comparator and the overlap rule (no GPU needed)
# ------------------------------------------------------------------------------------------------------------------------------
def unravel(flat: int, shape: Sequence[int]) -> Tuple[int, ...]:
    """The row-major coordinates of flat index ``flat`` in ``shape``; for an NHWC output (image, row, col, channel)."""
    flat, shape = int(flat), tuple(int(s) for s in shape)
    numel = 1
    for s in shape:
        numel *= s
    assert 0 <= flat < numel, f"flat index {flat} outside {shape}"
    coords = []
    for s in reversed(shape):
        flat, r = divmod(flat, s)
        coords.append(r)
    return tuple(reversed(coords))


def describe_difference(got: torch.Tensor, want: torch.Tensor) -> Optional[str]:
    """None if ``got`` holds the bits of ``want`` (integer views: NaN payloads and -0 count), else where they differ: how many elements,
    the first and last flat index and the coordinates of the first -- for a 4-D (NHWC) output its (image, row, col, channel), which
    names a tile and a stage and not just "differs"."""
    a, b = G.bits(got), G.bits(want)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"is {tuple(got.shape)} {got.dtype}, the plain run gave {tuple(want.shape)} {want.dtype}"
    if torch.equal(a, b):
        return None
    bad = torch.nonzero((a != b).view(-1)).view(-1)
    first, last = int(bad[0]), int(bad[-1])
    at = unravel(first, want.shape)
    where = f"(image, row, col, channel) = {at}" if len(at) == 4 else f"coordinates {at}"
    return (f"differs from the plain run in {bad.numel()} of {a.numel()} elements, flat indices {first} .. {last}, the first at {where} "
            f"of shape {tuple(want.shape)}")


def assert_same_bits(what: str, name: str, which: str, got: torch.Tensor, want: torch.Tensor) -> None:
    """``got`` (operand ``name`` of run ``which``) holds the bits of ``want``, the plain run's."""
    diff = describe_difference(got, want)
    if diff is not None:
        raise AssertionError(f"{what}: `{name}` of {which} {diff}")


def overlapped(op_end_ms: float, noise_end_ms: float) -> bool:
    """Both times from the event behind the burst's first kernel, which the row's stream waited for: the burst ended after the row did."""
    return noise_end_ms > op_end_ms >= 0.0


def intervals_intersect(a: Tuple[float, float], b: Tuple[float, float]) -> bool:
    """Two (start, end) intervals on one clock share more than a point."""
    return max(a[0], b[0]) < min(a[1], b[1])


def enough_overlap(flags: Sequence[bool]) -> bool:
    """Not more than a quarter of the repetitions failed to overlap (and there was one)."""
    n = len(flags)
    return n > 0 and (n - sum(bool(f) for f in flags)) <= MAX_NOT_OVERLAPPED * n


# ------------------------------------------------------------------------------------------------------------------------------
# arenas (GPU; nothing below runs at import)
# ------------------------------------------------------------------------------------------------------------------------------
class SpecArena(Arena):
    """The plain run (ordinary tensors) that also notes every operand the row asks for, in order."""

    def __init__(self):
        super().__init__(None)
        self.spec = []                      # (kind, name, payload | (shape, dtype))

    def inp(self, name, t):
        self.spec.append(("inp", name, t))
        return super().inp(name, t)

    def inout(self, name, t):
        r = super().inout(name, t)          # goes through ``inp``
        self.spec[-1] = ("inout", name, t)
        return r

    def out(self, name, shape, dtype, defined=True):
        self.spec.append(("out", name, (tuple(int(v) for v in shape), dtype)))
        return super().out(name, shape, dtype, defined)

    def ws(self, name, shape, dtype):
        self.spec.append(("ws", name, (tuple(int(v) for v in shape), dtype)))
        return super().ws(name, shape, dtype)


class ReplayArena(Arena):
    """One run's operands, all built at construction from a ``SpecArena``'s list: between 0xFF bands, outputs and workspaces
    pre-filled with 0xFF.  ``row.launch`` finds them by name; nothing is copied or allocated while it runs."""

    def __init__(self, spec):
        super().__init__(G.FILL_NAN)
        self.ready = {}
        for kind, name, v in spec:
            assert name not in self.ready, f"operand name {name} used twice"
            if kind in ("inp", "inout"):
                self.ready[name] = (kind, G.guarded(v, self.fill, device=DEV))
            else:
                self.ready[name] = (kind, G.guarded_empty(v[0], v[1], self.fill, device=DEV))
        self._deferred = []

    def _take(self, kind, name, shape, dtype):
        assert name in self.ready, f"the row asked for operand `{name}`, which its plain run did not (or asked twice)"
        had, t = self.ready.pop(name)
        assert had == kind and tuple(t.shape) == tuple(int(v) for v in shape) and t.dtype == dtype, \
            f"operand `{name}`: {kind} {tuple(shape)} {dtype} now, {had} {tuple(t.shape)} {t.dtype} in the plain run"
        return self._put(name, t)

    def inp(self, name, t):
        return self._take("inp", name, t.shape, t.dtype)

    def inout(self, name, t):
        self.results[name] = self._take("inout", name, t.shape, t.dtype)
        return self.results[name]

    def out(self, name, shape, dtype, defined=True):
        self.results[name] = self._take("out", name, shape, dtype)
        self.defined[name] = defined
        return self.results[name]

    def ws(self, name, shape, dtype):
        return self._take("ws", name, shape, dtype)

    def host_check(self, fn):
        self._deferred.append(fn)           # a look on the host would hold it in the middle of the window

    def finish(self):
        assert not self.ready, f"operands of the plain run that this run never asked for: {sorted(self.ready)}"
        for fn in self._deferred:
            fn()


def carries_state(row, payloads) -> bool:
    return row.scrub is not None or any(hasattr(v, "close") for v in (payloads if isinstance(payloads, tuple) else ()))


def plain_run(row, payloads):
    """The plain run on the current (default) stream: the ``SpecArena`` with the reference bits and the operand list."""
    plain = SpecArena()
    row.launch(plain, payloads)
    torch.cuda.synchronize()
    assert plain.results, f"{row.id}: no output"
    if row.scrub is not None:
        row.scrub(payloads)
    return plain


def _event():
    return torch.cuda.Event(enable_timing=True)


def timed_run(row, payloads, spec) -> Tuple[float, float]:
    """(device ms between events around one replayed run on the default stream, host ms ``row.launch`` took)."""
    a = ReplayArena(spec)
    torch.cuda.synchronize()
    s, e = _event(), _event()
    s.record()
    t0 = time.perf_counter()
    row.launch(a, payloads)
    host_ms = (time.perf_counter() - t0) * 1e3
    e.record()
    torch.cuda.synchronize()
    if row.scrub is not None:
        row.scrub(payloads)
    return float(s.elapsed_time(e)), host_ms


class Noise:
    """A stream of identical kernels on ``stream``: ``one()`` enqueues one, ``burst(ms)`` as many as last ``ms``."""

    def __init__(self, mode, stream):
        self.mode, self.stream, self.dtype = mode, stream, None
        with torch.cuda.stream(stream):
            if mode == "noise_mem":
                self.buf = torch.ones(NOISE_MEM_BYTES // 4, dtype=torch.float32, device=DEV)
            else:
                for dtype in (torch.bfloat16, torch.float16):
                    try:
                        g = torch.Generator(device=DEV).manual_seed(5)
                        self.a = (torch.randn((NOISE_MM_N, NOISE_MM_N), generator=g, device=DEV) * 0.01).to(dtype)
                        self.b = (torch.randn((NOISE_MM_N, NOISE_MM_N), generator=g, device=DEV) * 0.01).to(dtype)
                        self.c = torch.empty((NOISE_MM_N, NOISE_MM_N), dtype=dtype, device=DEV)
                        torch.mm(self.a, self.b, out=self.c)
                        stream.synchronize()
                        self.dtype = dtype
                        break
                    except RuntimeError as err:          # this dtype's GEMM is not usable here
                        print(f"repeatability: torch.mm in {dtype} is not usable: {err}")
                assert self.dtype is not None, "noise_mfma: torch.mm is usable neither in bf16 nor in fp16 on this machine"
            for _ in range(3):
                self.one()
            stream.synchronize()
            s, e = _event(), _event()
            s.record(stream)
            for _ in range(8):
                self.one()
            e.record(stream)
            stream.synchronize()
        self.kernel_ms = s.elapsed_time(e) / 8
        assert self.kernel_ms > 0

    def one(self):
        if self.mode == "noise_mem":
            self.buf.mul_(-1.0)
        else:
            torch.mm(self.a, self.b, out=self.c)

    def burst(self, ms):
        n = int(ms / self.kernel_ms) + 1
        for _ in range(n):
            self.one()
        return n


_SESSION = {}


def streams(lib):
    """(the row's stream, the stream beside it) of tests/stream_order.py: two pool streams that provably run side by side, so on two
    of the (default: 4) hardware queues.  No queue is added and nothing is captured."""
    from tests import stream_order as SO
    return SO.choose_stream(lib)[0], SO.choose_second_stream(lib)[0]


def noise_for(mode, lib) -> Noise:
    if mode not in _SESSION:
        _SESSION[mode] = Noise(mode, streams(lib)[1])
        print(f"repeatability: one {mode} kernel lasts {_SESSION[mode].kernel_ms:.3f} ms")
    return _SESSION[mode]


def burst_ms(lib, rows) -> float:
    """The length of a noise burst, once per session: ``BURST_FACTOR`` times the device time of ``MEASURED_SLOWEST_ROW``, measured now."""
    if "burst" not in _SESSION:
        row = next(r for r in rows if r.id == MEASURED_SLOWEST_ROW[0])
        payloads = row.make()
        try:
            plain = plain_run(row, payloads)
            dev_ms, _host = timed_run(row, payloads, plain.spec)
        finally:
            G.close_payloads(payloads)
        _SESSION["burst"] = max(NOISE_MS, BURST_FACTOR * dev_ms)
        print(f"repeatability: {row.id} takes {dev_ms:.3f} ms on the device; a noise burst lasts {_SESSION['burst']:.2f} ms")
    return _SESSION["burst"]


class Runs(NamedTuple):
    arenas: List[Tuple[str, object]]        # (label, ReplayArena) of every run of the mode
    overlap: Optional[List[bool]]           # per repetition, None for quiet
    detail: str                             # the repetitions that did not overlap, with their times
    note: str = ""                          # the tightest figure of the mode, for the report


def run_quiet(row, payloads, spec, reps) -> Runs:
    arenas = [ReplayArena(spec) for _ in range(reps)]
    torch.cuda.synchronize()
    for a in arenas:
        row.launch(a, payloads)
        if row.scrub is not None:
            torch.cuda.synchronize()
            row.scrub(payloads)
    torch.cuda.synchronize()
    return Runs([(f"quiet repetition {i}", a) for i, a in enumerate(arenas)], None, "")


def run_noisy(row, payloads, spec, reps, mode, lib, burst) -> Runs:
    side, beside = streams(lib)
    noise = noise_for(mode, lib)
    arenas = [ReplayArena(spec) for _ in range(reps)]
    torch.cuda.synchronize()
    marks = []
    for a in arenas:
        first, op_end, noise_end = _event(), _event(), _event()
        with torch.cuda.stream(beside):
            noise.one()
            first.record(beside)
        side.wait_event(first)                  # the row starts once the noise runs
        with torch.cuda.stream(beside):
            noise.burst(burst)
            noise_end.record(beside)
        with torch.cuda.stream(side):
            row.launch(a, payloads)
            op_end.record(side)
        marks.append((first, op_end, noise_end))
        if row.scrub is not None:
            torch.cuda.synchronize()
            row.scrub(payloads)
    torch.cuda.synchronize()
    times = [(f.elapsed_time(o), f.elapsed_time(n)) for f, o, n in marks]
    flags = [overlapped(o, n) for o, n in times]
    detail = "; ".join(f"{i}: row ended {o:.3f} ms, burst {n:.3f} ms" for i, (o, n) in enumerate(times) if not overlapped(o, n))
    note = "at most %.0f %% of the burst was over when the row ended" % (100.0 * max(o / n for o, n in times))
    return Runs([(f"{mode} repetition {i}", a) for i, a in enumerate(arenas)], flags, detail, note)


def _launch_on(stream, row, arena, payloads, start, end, errors):
    """One copy of a twin repetition, on the calling thread: events around ``row.launch`` on ``stream``."""
    try:
        with torch.cuda.stream(stream):
            start.record(stream)
            row.launch(arena, payloads)
            end.record(stream)
    except BaseException as err:                # handed to the test's thread
        errors.append(err)


def run_twin(row, payloads, payloads2, spec, reps, lib, host_ms, two_threads=False) -> Runs:
    """``two_threads``: each copy is enqueued by a host thread of its own (the library call releases the interpreter lock).  For a row
    whose op synchronises the host before it launches: one thread would enqueue the second copy only when the first has left its
    synchronisation and launched, that is when the first copy is all but over."""
    from tests import stream_order as SO
    sa, sb = streams(lib)
    pairs = [(ReplayArena(spec), ReplayArena(spec)) for _ in range(reps)]
    gate = max(1, int(SO.calibrate(1.0) * (GATE_MS + 1.5 * 2 * host_ms + (THREAD_GATE_MS if two_threads else 0.0))))
    torch.cuda.synchronize()
    marks = []
    default = torch.cuda.default_stream()
    for a, b in pairs:
        g, a0, a1, b0, b1 = _event(), _event(), _event(), _event(), _event()
        torch.cuda._sleep(gate)                 # the gate: on the default stream, so that both copies hear of it the same way
        g.record(default)
        sa.wait_event(g)                        # both copies start when the gate opens, both already enqueued
        sb.wait_event(g)
        errors = []
        if two_threads:
            workers = [threading.Thread(target=_launch_on, args=(sa, row, a, payloads, a0, a1, errors)),
                       threading.Thread(target=_launch_on, args=(sb, row, b, payloads2, b0, b1, errors))]
            for w in workers:
                w.start()
            for w in workers:
                w.join()
        else:
            _launch_on(sa, row, a, payloads, a0, a1, errors)
            _launch_on(sb, row, b, payloads2, b0, b1, errors)
        if errors:
            torch.cuda.synchronize()
            raise errors[0]
        marks.append((g, a0, a1, b0, b1))
        if row.scrub is not None:
            torch.cuda.synchronize()
            row.scrub(payloads)
            row.scrub(payloads2)
    torch.cuda.synchronize()
    spans = [((g.elapsed_time(a0), g.elapsed_time(a1)), (g.elapsed_time(b0), g.elapsed_time(b1))) for g, a0, a1, b0, b1 in marks]
    flags = [intervals_intersect(x, y) for x, y in spans]
    detail = "; ".join(f"{i}: first copy {x[0]:.3f} .. {x[1]:.3f} ms, second {y[0]:.3f} .. {y[1]:.3f} ms"
                       for i, (x, y) in enumerate(spans) if not intervals_intersect(x, y))
    arenas = [(f"twin repetition {i}, {which} copy", t) for i, (a, b) in enumerate(pairs) for which, t in (("first", a), ("second", b))]
    apart = sorted(abs(x[1] - y[1]) * 1e3 for x, y in spans)
    note = f"the two copies ended {apart[0]:.0f} to {apart[-1]:.0f} us apart (median {apart[len(apart) // 2]:.0f} us)"
    return Runs(arenas, flags, detail, note)
