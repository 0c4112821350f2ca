"""The guard-band rows of include/r50_resample.h: ``ROWS_RESAMPLE`` (tests/test_resample_guard_bands_gpu.py says what they cover)."""
import functools

import torch

from tests import resample_reference as RR
from tests.guard_bands import F32, I32, Row, lib, stream


ROWS_RESAMPLE = []


def _make(joints, kind):
    c = RR.ragged_case(joints, seed=joints)
    pay = {k: torch.from_numpy(c[k]) for k in ("x", "idx", "seq_start", "out_time", "out_seq", "out_left")}
    pay.update(f=c["f"], s=c["s"], g=c["g"], j=joints, kind=kind, max_gap=c["max_gap"])
    return pay


def _launch(a, pay):
    # the two rows a stencil can step past either end of the poses
    a.reach(2 * pay["j"] * 3 * 4)
    rc = lib().r50_op_resample_sequences(a.inp("x", pay["x"]).data_ptr(), a.inp("idx", pay["idx"]).data_ptr(),
                                          a.inp("seq_start", pay["seq_start"]).data_ptr(), pay["f"], pay["s"], pay["j"],
                                          a.inp("out_time", pay["out_time"]).data_ptr(), a.inp("out_seq", pay["out_seq"]).data_ptr(),
                                          a.inp("out_left", pay["out_left"]).data_ptr(), pay["g"], pay["kind"], pay["max_gap"],
                                          a.out("y", (pay["g"], pay["j"], 3), F32).data_ptr(), a.out("flags", (pay["g"],), I32).data_ptr(), stream())
    assert rc == 0, lib().r50_last_error(None)


for _j in (17, 1, 64):
    for _kind, _name in ((RR.LINEAR, "linear"), (RR.CUBIC, "cubic")):
        ROWS_RESAMPLE.append(Row("resample", f"resample_sequences-ragged-J{_j}-{_name}", ("r50_op_resample_sequences",),
                                 functools.partial(_make, _j, _kind), _launch))
