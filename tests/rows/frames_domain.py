"""The guard-band rows of the crop + resize kernels over their domain: ``ROWS_FRAMES_DOMAIN``, and the oracle results
tests/test_frames_domain_gpu.py shares with them (it runs the rows between guard bands and late on a side stream)."""
import functools

import numpy as np
import torch

from implementation_phd_lab_vision_amd import frames as F
from implementation_phd_lab_vision_amd import track
from oracle import resize_oracle as ro
from tests import resize_cases as RC
from tests.guard_bands import U8, Row, lib, stream

MODES = [F.RESIZE_FLOAT, F.RESIZE_FIXED]
MODE_IDS = ["float", "fixed"]


@functools.lru_cache(maxsize=None)
def _want(hh, ww, out, mode):
    """The oracle's (T, 3, out, out) result for ``RC.image(hh, ww, out)``: computed once per case and mode, shared, never modified."""
    x = RC.crop_nchw(RC.image(hh, ww, out))
    got = ro.resize_bilinear_u8(x, out, out) if mode == F.RESIZE_FIXED else ro.resize_bilinear_u8_float_restated(x, out, out)
    t = torch.from_numpy(np.ascontiguousarray(got))
    assert t.shape == (RC.T, 3, out, out) and t.dtype == U8, f"the oracle gave {tuple(t.shape)} {t.dtype}, not {(RC.T, 3, out, out)} uint8"
    return t


def _table_want(case, out, mode):
    return torch.stack([_want(hh, ww, out, mode)[fi] for (hh, ww), fi in case["frames"]])


ROWS_FRAMES_DOMAIN = []


def _producer_make(hh, ww, out):
    return RC.embed(RC.image(hh, ww, out, t=2), *RC.placements(hh, ww)[0][1:])


def _producer_launch(out, mode):
    def launch(a, pay):
        clip, (top, left, hh, ww) = pay
        t, h, w, _ = clip.shape
        a.reach(2 * w * 3 + 8)                                       # two source rows, plus the dword rounding at either end
        f = a.inp("frames", clip)
        for flags in (0, 3):
            o = a.out(f"out[flags {flags}]", (t, 3, out, out), U8)
            rc = lib().r50_op_crop_resize_u8(f.data_ptr(), t, h, w, top, left, hh, ww, o.data_ptr(), out, mode, flags, stream())
            assert rc == 0, lib().r50_last_error(None)
    return launch


def _producer_check(out, mode):
    def check(plain, pay):
        clip, (top, left, hh, ww) = pay
        x = np.transpose(clip.numpy(), (0, 3, 1, 2))[:, :, top:top + hh, left:left + ww]
        want = ro.resize_bilinear_u8(x, out, out) if mode == F.RESIZE_FIXED else ro.resize_bilinear_u8_float_restated(x, out, out)
        want = torch.from_numpy(np.ascontiguousarray(want))
        got, flipped = plain.results["out[flags 0]"].cpu(), plain.results["out[flags 3]"].cpu()
        assert torch.equal(got, want), f"flags 0: {int((got != want).sum())} of {want.numel()} bytes differ from the oracle"
        assert torch.equal(flipped, torch.flip(want, dims=[0, -1])), "flags 3: not the oracle's result flipped in time and across"
    return check


def _table_make(out, mode, tail):
    c = RC.packed_table(out, tail)
    table = track.BoxTable(c["offsets"], c["sizes"], c["boxes"], c["src_bytes"], out, mode)
    return dict(case=c, buf=c["buf"], table=torch.from_numpy(table.host), t=table.t, max_ww=table.max_ww, src_bytes=c["src_bytes"], out=out, mode=mode)


def _table_launch(a, pay):
    a.reach(2 * pay["case"]["max_w"] * 3 + 8)                         # two source rows of the widest image, plus the dword rounding
    src, table = a.inp("src", pay["buf"]), a.inp("table", pay["table"])
    shape = (pay["t"], 3, pay["out"], pay["out"])
    o, of = a.out("out", shape, U8), a.out("out_flip", shape, U8)
    rc = lib().r50_op_crop_resize_boxes_u8(src.data_ptr(), pay["src_bytes"], table.data_ptr(), pay["t"], pay["max_ww"], o.data_ptr(), of.data_ptr(),
                                             pay["out"], pay["mode"], stream())
    assert rc == 0, lib().r50_last_error(None)


def _table_check(plain, pay):
    want = _table_want(pay["case"], pay["out"], pay["mode"])
    got, flipped = plain.results["out"].cpu(), plain.results["out_flip"].cpu()
    assert torch.equal(got, want) and torch.equal(flipped, torch.flip(want, dims=[-1])), \
        f"{int((got != want).sum())} of {want.numel()} bytes of out differ from the oracle, or out_flip is not its mirror image"


for _mode, _name in zip(MODES, MODE_IDS):
    for _hh, _ww, _out in ((40, 8, 12), (1033, 691, 344)):
        ROWS_FRAMES_DOMAIN.append(Row("frames_domain", f"crop_resize_u8-{_hh}x{_ww}_to_{_out}-{_name}", ("r50_op_crop_resize_u8",),
                                      functools.partial(_producer_make, _hh, _ww, _out), _producer_launch(_out, _mode), _producer_check(_out, _mode)))
    ROWS_FRAMES_DOMAIN.append(Row("frames_domain", f"crop_resize_boxes_u8-every_source-out12-{_name}-flip", ("r50_op_crop_resize_boxes_u8",),
                                  functools.partial(_table_make, 12, _mode, 3), _table_launch, _table_check))
