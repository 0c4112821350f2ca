"""The guard-band rows of include/r50_kinematics.h: ``ROWS_KINEMATICS`` (tests/test_kinematics_gpu.py runs them between guard bands and late on a side stream)."""
import functools

import numpy as np
import torch

from tests import guard_bands as G
from tests.guard_bands import F32, F64, I32, Row
from tests.kinematics_cases import SHAPES, _case, _product_skeleton


def _make(shape):
    c = _case(shape, 0.005)
    sk = _product_skeleton(SHAPES[shape][0])
    seq_start = c["seq_start"]
    row_seq = np.repeat(np.arange(len(seq_start) - 1, dtype=np.int32), np.diff(seq_start))
    return dict(x=torch.from_numpy(c["x"]), seq_start=torch.from_numpy(seq_start), row_seq=torch.from_numpy(row_seq), sk=sk, f=int(seq_start[-1]),
                s=len(seq_start) - 1, j=sk.joints)


def _launch(a, pay):
    """Both ops: the rest offsets feed the per-frame pass, as in ``pose_rotations``."""
    # every row is found through a table entry times the row pitch; a wrong entry within the table's own range lands within the poses, and
    # one row block (64 rows at most) past either end is what a wrong bound could reach
    a.reach(64 * pay["j"] * 4 * 4)
    lib, s = G.lib(), G.stream()
    f, n, j = pay["f"], pay["s"], pay["j"]
    x = a.inp("x", pay["x"])
    rest = a.out("rest", (n, j, 3), F64)
    rc = lib.r50_op_rest_offsets(x.data_ptr(), a.inp("seq_start", pay["seq_start"]).data_ptr(), f, n, j, *pay["sk"].c_args(), rest.data_ptr(), s)
    assert rc == 0, lib.r50_last_error(None)
    rc = lib.r50_op_pose_rotations(x.data_ptr(), a.inp("row_seq", pay["row_seq"]).data_ptr(), f, n, j, *pay["sk"].c_args(), rest.data_ptr(),
                                   a.out("quat", (f, j, 4), F32).data_ptr(), a.out("euler", (f, j, 3), F32).data_ptr(),
                                   a.out("rigid", (f, j, 3), F32).data_ptr(), a.out("resid", (f,), F32).data_ptr(),
                                   a.out("flags", (f,), I32).data_ptr(), s)
    assert rc == 0, lib.r50_last_error(None)


ROWS_KINEMATICS = [Row("kinematics", f"rest_offsets+pose_rotations-{shape}", ("r50_op_rest_offsets", "r50_op_pose_rotations"),
                       functools.partial(_make, shape), _launch) for shape in SHAPES]
