"""The guard-band rows of include/r50_refine.h: ``ROWS_REFINE`` (tests/test_refine_gpu.py runs them between guard bands and late on a side stream)."""
import ctypes
import functools

import numpy as np
import torch

from tests import guard_bands as G
from tests import refine_reference as RR
from tests.guard_bands import F32, F64, Row
from tests.refine_cases import _case


def _make(joints, with_conf, lbone):
    c = _case(joints, with_conf)
    row_seq, row_seg = RR.row_tables(c["seq_start"], c["idx"])
    seg_start = np.append(np.flatnonzero(np.diff(row_seg, prepend=-1)), row_seg.size)
    t = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt))   # noqa: E731
    return dict(x0=t(c["x0"], np.float32), rays=t(c["rays"], np.float32), conf=None if c["conf"] is None else t(c["conf"], np.float32),
                seq_start=t(c["seq_start"]), row_seq=t(row_seq), seg_start=t(seg_start), row_seg=t(row_seg), lens=t(c["bone_len"], np.float64),
                edges=[v for e in c["edges"] for v in e], f=int(row_seg.size), g=int(seg_start.size - 1), s=int(len(c["seq_start"]) - 1), j=joints,
                lbone=lbone)


def _launch(a, pay):
    """Energy, five sweeps, energy: as ``refine_sequences``."""
    f, g, s, j = pay["f"], pay["g"], pay["s"], pay["j"]
    # a row is found through a table entry times the row pitch; a wrong bound of a block's staged rows (its own and the halo) could reach
    # that many rows of the fp64 iterate past an end
    a.reach((64 + 4) * 3 * j * 8 if j <= 32 else (32 + 4) * 3 * j * 8)
    lib, st = G.lib(), G.stream()
    edges = (ctypes.c_int * len(pay["edges"]))(*pay["edges"])
    x0, rays = a.inp("x0", pay["x0"]), a.inp("rays", pay["rays"])
    conf = a.inp("conf", pay["conf"]).data_ptr() if pay["conf"] is not None else None
    seq_start, row_seg = a.inp("seq_start", pay["seq_start"]), a.inp("row_seg", pay["row_seg"])
    lens = a.inp("bone_len", pay["lens"]).data_ptr() if pay["lbone"] != 0.0 else None
    n_edges = len(pay["edges"]) // 2 if pay["lbone"] != 0.0 else 0
    before = a.out("energy_before", (s, 6), F64)
    rc = lib.r50_op_pose_fit_energy(x0.data_ptr(), x0.data_ptr(), rays.data_ptr(), conf, seq_start.data_ptr(), row_seg.data_ptr(), f, s, j,
                                    edges if n_edges else None, n_edges, lens, 0.1, before.data_ptr(), st)
    assert rc == 0, lib.r50_last_error(None)
    out = a.out("out", (f, j, 3), F32)
    rc = lib.r50_op_pose_fit_sweeps(x0.data_ptr(), rays.data_ptr(), conf, a.inp("seg_start", pay["seg_start"]).data_ptr(), row_seg.data_ptr(),
                                    a.inp("row_seq", pay["row_seq"]).data_ptr(), f, g, s, j, edges if n_edges else None, n_edges, lens, 1.0, 1.0,
                                    1.0, pay["lbone"], 0.6, 0.1, 5, a.ws("workspace", (2 * f * j * 3,), F64).data_ptr(), out.data_ptr(), st)
    assert rc == 0, lib.r50_last_error(None)
    rc = lib.r50_op_pose_fit_energy(out.data_ptr(), x0.data_ptr(), rays.data_ptr(), conf, seq_start.data_ptr(), row_seg.data_ptr(), f, s, j,
                                    edges if n_edges else None, n_edges, lens, 0.1, a.out("energy_after", (s, 6), F64).data_ptr(), st)
    assert rc == 0, lib.r50_last_error(None)


ROWS_REFINE = [Row("refine", f"fit_energy+fit_sweeps-J{j}-{'conf' if cf else 'confNULL'}-bone{int(lb)}",
                   ("r50_op_pose_fit_sweeps", "r50_op_pose_fit_energy"), functools.partial(_make, j, cf, lb), _launch)
               for j, cf, lb in ((17, True, 1.0), (17, False, 0.0), (3, True, 1.0), (64, True, 1.0))]
