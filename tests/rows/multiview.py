"""The guard-band rows of include/r50_multiview.h: ``ROWS_MULTIVIEW`` (tests/test_multiview_guard_bands_gpu.py says what they cover)."""
import functools

import numpy as np
import torch

from tests.guard_bands import F32, F64, I32, Row, lib, stream


ROWS_MULTIVIEW = []


# two takes: four cameras with ragged ends and a gap (the longest pair has 63 matched rows: 315 points at J = 5, a ragged second round of
# the per-thread loop), and two cameras that share a single frame; then a lone camera.  153 rows: 39 workgroups of the fuse kernel, the
# last ragged.
_SPEC = [((9, "sit", 1), list(range(0, 70))), ((9, "sit", 2), list(range(2, 30)) + list(range(33, 68))), ((9, "sit", 3), list(range(2, 12))),
         ((9, "sit", 4), list(range(10, 12))), ((9, "walk", 1), [0, 1, 2]), ((9, "walk", 2), [2, 3, 4, 5]), ((11, "walk", 1), [0])]
assert sum(len(fr) for _, fr in _SPEC) == 153


def _make(joints, seed, mode=0):
    from implementation_phd_lab_vision_amd.multiview import ViewTable
    from tests import multiview_reference as MR
    keys = [k for k, _ in _SPEC]
    seq_start = np.concatenate([[0], np.cumsum([len(fr) for _, fr in _SPEC])]).astype(np.int32)
    frame_idx = np.concatenate([np.asarray(fr, dtype=np.int32) for _, fr in _SPEC])
    table = ViewTable.from_sequences(keys, seq_start, frame_idx)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((table.rows, joints, 3), generator=g) * 0.3 + torch.tensor([0.0, 0.0, 5.0])
    want = MR.view_table(keys, seq_start, frame_idx)
    fit, _ = MR.rigid_fit(x.numpy(), x.numpy(), want["pairs"])                     # the fuse row's transforms: made on the host
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1))            # noqa: E731
    return dict(x=x, f=table.rows, j=joints, p=table.pairs, mode=mode, pair_start=t(table.pair_start), match=t(table.match),
                peer_start=t(table.peer_start), peer_row=t(table.peer_row), peer_fit=t(table.peer_fit), fit=torch.from_numpy(fit),
                longest=int(np.diff(table.pair_start).max()))


def _reach(a, pay):
    # Both kernels find a row through a table entry times the row pitch; a wrong entry within the table's own range lands within the
    # poses.  What an index mistake could reach past either end: one row block of the fuse kernel (4 rows) plus the longest pair.
    a.reach((4 + pay["longest"]) * pay["j"] * 3 * 4)


def _fit_launch(a, pay):
    """y and x one buffer, as the pass calls it."""
    _reach(a, pay)
    x = a.inp("x", pay["x"])
    rc = lib().r50_op_view_rigid_fit(x.data_ptr(), x.data_ptr(), pay["f"], pay["f"], pay["j"], a.inp("pair_start", pay["pair_start"]).data_ptr(),
                                      a.inp("match", pay["match"]).data_ptr(), pay["p"], a.out("fit", (pay["p"], 16), F64).data_ptr(), stream())
    assert rc == 0, lib().r50_last_error(None)


def _fuse_launch(a, pay):
    _reach(a, pay)
    rc = lib().r50_op_view_fuse(a.inp("pose", pay["x"]).data_ptr(), pay["f"], pay["j"], a.inp("peer_start", pay["peer_start"]).data_ptr(),
                                 a.inp("peer_row", pay["peer_row"]).data_ptr(), a.inp("peer_fit", pay["peer_fit"]).data_ptr(),
                                 a.inp("fit", pay["fit"]).data_ptr(), pay["p"], pay["mode"], a.out("fused", (pay["f"], pay["j"], 3), F32).data_ptr(),
                                 a.out("disagreement", (pay["f"],), F32).data_ptr(), stream())
    assert rc == 0, lib().r50_last_error(None)


for _j in (17, 5, 33, 64):
    ROWS_MULTIVIEW.append(Row("multiview", f"view_rigid_fit-J{_j}", ("r50_op_view_rigid_fit",), functools.partial(_make, joints=_j, seed=_j),
                              _fit_launch))
    for _mode, _name in enumerate(("mean", "median", "others")):
        if _j in (17, 5) or _mode == 1:
            ROWS_MULTIVIEW.append(Row("multiview", f"view_fuse-{_name}-J{_j}", ("r50_op_view_fuse",),
                                      functools.partial(_make, joints=_j, seed=50 + _j + _mode, mode=_mode), _fuse_launch))
