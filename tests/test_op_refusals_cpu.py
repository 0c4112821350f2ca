"""What every r50_op_* hook answers when it refuses, replayed against a recording: status and r50_last_error(NULL) text per case.

tests/golden/op_refusals.json was recorded from the library as it stood before the hooks were given one frame (name, refusals, dispatch,
status); a change of the op layer in csrc/r50_abi.hip that alters one refusal, its status or its wording shows up here without a GPU.
Recording again (only when a hook or a message changes on purpose): ``python -m tests.test_op_refusals_cpu`` on a machine without a GPU.

The cases come from the headers (tests.alignment.prototypes) and from tests/size_limits.py:

  null/<op>             every r50_op_* hook with all pointers NULL and all numbers 0
  below/<op>/<param>    every device parameter whose requirement A is above 1 byte sits A/2 off an A-aligned fake address, every other
                        device pointer on a 256-aligned fake address, host pointers NULL, numbers 0
  beyond/<case id>      every one-step-beyond case of tests/size_limits.py (n_max + 1), through the call sites of
                        tests/test_size_limits_gpu.py, on 256-aligned fake addresses

Fake addresses are never handed to a library that could launch: the module is skipped where a GPU is present.  Every case is answered
before the hook's first launch, copy, allocation or attribute call and without reading through a pointer: read in csrc/r50_abi.hip, each
hook checks alignment and its counts (a count of 0 is refused by every hook) before it reads a host table or touches the stream, and the
size rules run in fill_conv_args, the launchers' argument checks and the two early checks of r50_op_bneck_tail / r50_op_bneck_cat_chain.
The one HIP function on these paths is hipGetErrorString, a table lookup, for the refusals that carry no note of their own.

Left out: nothing.  The two size queries (r50_stem_scratch_bytes, r50_op_nn_search_workspace) have no pointer and no status; the handle
functions (r50_forward*) are not hooks.
"""
import ctypes as C
import json

import pytest
import torch

from tests import alignment as AL
from tests import guard_bands as G
from tests import size_limits as S

FIXTURE = AL.ROOT / "tests" / "golden" / "op_refusals.json"
BASE = 0x7F0000000000           # fake device addresses: 256-aligned, 1 MiB apart


def _hooks():
    return {fn: params for fn, params in AL.prototypes().items() if fn.startswith("r50_op_") and any(p.pointer for p in params)}


def _call(fn, params, address_of):
    """Calls ``fn`` with ``address_of(i, param)`` for device pointers (None = NULL), NULL for every other pointer and 0 for every number."""
    lib = G.lib()
    f = getattr(lib, fn)
    args = []
    for i, (p, ctype) in enumerate(zip(params, f.argtypes)):
        if not p.pointer:
            args.append(0)
            continue
        addr = address_of(i, p) if p.device else None
        args.append(None if addr is None else C.cast(C.c_void_p(addr), ctype))
    return _answer(lib, f(*args))


def _answer(lib, rc):
    msg = lib.r50_last_error(None)
    return {"status": int(rc), "text": msg.decode() if msg else ""}


class _Fake:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def _beyond(case, monkeypatch_stream):
    from tests.test_size_limits_gpu import FAMILIES
    fam = FAMILIES[case.family]
    hw = fam.weights(case)
    names = [list(fam.inputs(case)), list(fam.device_weights(case, hw)), list(fam.outputs(case)), list(fam.workspace(case, case.n_max + 1))]
    k = iter(range(1, 1000))
    I, W, O, ws = ({name: _Fake(BASE + (next(k) << 20)) for name in group} for group in names)
    with monkeypatch_stream():
        rc = fam.call(case, case.n_max + 1, I, W, O, ws)
    return _answer(G.lib(), rc)


def _no_stream():
    import contextlib

    @contextlib.contextmanager
    def cm():
        keep, G.stream = G.stream, lambda: None
        try:
            yield
        finally:
            G.stream = keep
    return cm


def replay():
    """case id -> {"status", "text"}, in a fixed order."""
    out = {}
    hooks = _hooks()
    for fn, params in hooks.items():
        out[f"null/{fn}"] = _call(fn, params, lambda i, p: None)
    for fn, params in hooks.items():
        for v, victim in enumerate(params):
            if victim.device and victim.required and victim.required > 1:
                a = victim.required
                out[f"below/{fn}/{victim.name}"] = _call(
                    fn, params, lambda i, p: BASE + ((i + 1) << 20) + (a // 2 if i == v else 0))
    for case in S.CASES:
        if case.beyond:
            out[f"beyond/{case.id}"] = _beyond(case, _no_stream())
    return out


needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="fake addresses are never handed to a library that can launch")


def test_every_hook_with_a_pointer_has_a_null_case():
    protos = AL.prototypes()
    ops = [fn for fn in protos if fn.startswith("r50_op_")]
    queries = [fn for fn in ops if not any(p.pointer for p in protos[fn])]
    assert sorted(queries) == ["r50_op_nn_search_workspace"]        # r50_stem_scratch_bytes, the other size query, is no r50_op_* name
    recorded = json.loads(FIXTURE.read_text())
    nulls = [k for k in recorded if k.startswith("null/")]
    print(f"{len(nulls)} null cases, {sum(k.startswith('below/') for k in recorded)} below, {sum(k.startswith('beyond/') for k in recorded)} beyond")
    assert sorted(nulls) == sorted(f"null/{fn}" for fn in _hooks()) and len(nulls) == len(ops) - len(queries) >= 70
    assert sorted(k for k in recorded if k.startswith("beyond/")) == sorted(f"beyond/{c.id}" for c in S.CASES if c.beyond)
    for k, v in recorded.items():
        assert v["status"] == -1 and v["text"].startswith(k.split("/")[1] if not k.startswith("beyond/") else "r50_op_"), f"{k}: {v}"


@needs_no_gpu
def test_every_refusal_reads_as_recorded():
    recorded = json.loads(FIXTURE.read_text())
    got = replay()
    assert list(got) == list(recorded), "the case list changed: a hook, a parameter or a size case was added or removed"
    differ = {k: (recorded[k], got[k]) for k in got if got[k] != recorded[k]}
    assert not differ, "\n".join(f"{k}: recorded {a}, now {b}" for k, (a, b) in differ.items())


if __name__ == "__main__":
    assert not torch.cuda.is_available()
    FIXTURE.write_text(json.dumps(replay(), indent=1) + "\n")
    print(f"recorded {FIXTURE}")
