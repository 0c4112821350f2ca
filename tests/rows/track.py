"""The guard-band rows of include/r50_track.h: ``ROWS_TRACK`` (tests/test_track_guard_bands_gpu.py says what they cover)."""
import functools

import torch

from tests import track_reference as TR
from tests.guard_bands import U8, Row, lib, stream


ROWS_TRACK = []


def _make(out_size, mode, tail):
    from implementation_phd_lab_vision_amd.track import BoxTable
    c = TR.ragged_case(out_size, tail)
    table = BoxTable(c["offsets"], c["sizes"], c["boxes"], c["src_bytes"], out_size, mode)
    return dict(buf=c["buf"], table=torch.from_numpy(table.host), t=table.t, max_ww=table.max_ww, src_bytes=c["src_bytes"], out=out_size,
                mode=mode)


def _launch(flip):
    def launch(a, pay):
        # the widest image's two staged rows plus the dword rounding at either end: what a wrong row or column index could reach
        a.reach(2 * 80 * 3 + 8)
        src, table = a.inp("src", pay["buf"]), a.inp("table", pay["table"])
        shape = (pay["t"], 3, pay["out"], pay["out"])
        out = a.out("out", shape, U8)
        out_flip = a.out("out_flip", shape, U8) if flip else None
        rc = lib().r50_op_crop_resize_boxes_u8(src.data_ptr(), pay["src_bytes"], table.data_ptr(), pay["t"], pay["max_ww"], out.data_ptr(),
                                                None if out_flip is None else out_flip.data_ptr(), pay["out"], pay["mode"], stream())
        assert rc == 0, lib().r50_last_error(None)
    return launch


for _out in (8, 224):
    for _mode, _name in ((0, "float"), (1, "fixed")):
        for _flip in (False, True):
            for _tail in TR.TAILS:
                ROWS_TRACK.append(Row("track", f"crop_resize_boxes_u8-ragged-out{_out}-{_name}-tail{_tail}" + ("-flip" if _flip else ""),
                                      ("r50_op_crop_resize_boxes_u8",), functools.partial(_make, _out, _mode, _tail), _launch(_flip)))
