"""The guard-band rows of include/r50_bootstrap.h: ``ROWS_BOOTSTRAP`` (tests/test_bootstrap_guard_bands_gpu.py says what they cover)."""
import functools

import numpy as np
import torch

from tests.guard_bands import F64, I32, Row, lib, stream

STRATA = (1, 5, 70)

ROWS_BOOTSTRAP = []


def unit_rows(units, m, seed):
    """(U, m) fp64 with mixed signs and zeros; from m = 7 on, column 1 is of the order 1e300 and column 2 of the order 1e-300."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((units, m)) * rng.choice([0.0, 1.0, 1.0, 1e3], size=(units, m))
    if m >= 7:
        v[:, 1] *= 1e300
        v[:, 2] *= 1e-300
    return v


def _make(m, reps, with_counts):
    start = np.concatenate([[0], np.cumsum(STRATA)]).astype(np.int32)
    return {"v": torch.from_numpy(unit_rows(int(start[-1]), m, m)), "start": torch.from_numpy(start), "u": int(start[-1]), "g": len(STRATA),
            "m": m, "reps": reps, "counts": with_counts, "seed": 0xFEDCBA9876543210, "window": 16}


def _launch(a, pay):
    a.reach(pay["m"] * 8)                                                           # one row of v: the stride of the sum's loads
    out = a.out("out", (pay["reps"], pay["g"], pay["m"]), F64)
    counts = a.out("counts", (pay["reps"], pay["u"]), I32) if pay["counts"] else None
    rc = lib().r50_op_bootstrap_sums(a.inp("v", pay["v"]).data_ptr(), a.inp("stratum_start", pay["start"]).data_ptr(), pay["u"], pay["g"],
                                      pay["m"], 2 ** 32 - 2, pay["reps"], pay["seed"], pay["window"], out.data_ptr(),
                                      None if counts is None else counts.data_ptr(), stream())
    assert rc == 0, lib().r50_last_error(None)


for _m in (7, 300):
    for _counts in (True, False):
        ROWS_BOOTSTRAP.append(Row("bootstrap", f"bootstrap_sums-strata-1-5-70-M{_m}-window16-{'counts' if _counts else 'nocounts'}",
                                  ("r50_op_bootstrap_sums",), functools.partial(_make, _m, 5, _counts), _launch))
