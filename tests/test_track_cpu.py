"""The box track and the per-frame-box crop op (INTEGRATION.md section AA) without a GPU: the seventh public header include/r50_track.h
bound, exported and guard-banded; the weight precision against the oracle; ``track_boxes`` against the restatements of
tests/track_reference.py; the refusals of ``BoxTable`` and of the C entry before any launch; the parser."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import track_reference as TR
from tests.test_kinematics_cpu import PREDICT_KEYS

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "r50_track.h"
OPS = {"r50_track_weight_precision", "r50_op_crop_resize_boxes_u8"}
NOT_GUARDED = {"r50_track_weight_precision": "host arithmetic: no device operand"}
IMG_H, IMG_W, N = 120, 200, 97


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = re.findall(r"^\s*(?:int|int64_t|size_t)\s+(r50_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    assert protos, "no prototypes parsed from include/r50_track.h"
    return [(name, len([a for a in args.split(",") if a.strip()])) for name, args in protos]


def test_every_prototype_of_the_track_header_is_bound_exported_and_guard_banded(lib_built):
    from implementation_phd_lab_vision_amd import _lib
    from tests.rows import track as T
    protos = _prototypes()
    names = [n for n, _ in protos]
    assert set(names) == OPS == set(_lib._SIGNATURES_TRACK) and len(names) == len(set(names))
    covered = set()
    for row in T.ROWS_TRACK:
        covered.update(row.ops)
    assert covered == OPS - set(NOT_GUARDED) and len({row.id for row in T.ROWS_TRACK}) == len(T.ROWS_TRACK)
    others = [(ROOT / "include" / h).read_text() for h in ("r50.h", "r50_hal.h", "r50_smooth.h", "r50_multiview.h", "r50_kinematics.h",
                                                            "r50_refine.h")]
    tables = (_lib._SIGNATURES, _lib._SIGNATURES_HAL, _lib._SIGNATURES_SMOOTH, _lib._SIGNATURES_MULTIVIEW, _lib._SIGNATURES_KINEMATICS,
              _lib._SIGNATURES_REFINE)
    for name, arity in protos:
        assert len(_lib._SIGNATURES_TRACK[name][1]) == arity, name
        assert hasattr(lib_built, name), f"{name} declared in r50_track.h but not exported by libr50hip.so"
        assert getattr(lib_built, name).argtypes == _lib._SIGNATURES_TRACK[name][1]
        assert not any(name in table for table in tables)
        assert name not in _lib.EXPORTED_SYMBOLS and not any(name in text for text in others)
    assert "r50_track.h" in (ROOT / "implementation_phd_lab_vision_amd" / "_lib.py").read_text().split("def _source_digest")[1].split("def ")[0]
    abi = (ROOT / "implementation_phd_lab_vision_amd" / "csrc" / "r50_abi.hip").read_text()
    assert '#include "track_kernels.h"' in abi and "r50_track.h" in abi
    kernel = (ROOT / "implementation_phd_lab_vision_amd" / "csrc" / "track_kernels.h").read_text()
    assert "resize_taps(" in kernel and "void resize_taps" not in kernel, "the taps are kernels.h's: used, not copied"


def test_weight_precision_is_the_oracles(lib_built):
    from implementation_phd_lab_vision_amd import track
    from oracle.resize_oracle import index_weights_int16
    for out_size in (8, 224):
        for size in range(1, 301):
            want = index_weights_int16(size, out_size)[3]
            assert lib_built.r50_track_weight_precision(size, out_size) == want, (size, out_size)
            assert track.weight_precision(size, out_size) == want
    assert lib_built.r50_track_weight_precision(0, 8) == -1 and lib_built.r50_track_weight_precision(8, 0) == -1


# ---- track_boxes ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk():
    return TR.walker(N, IMG_H, IMG_W)


def _inside(boxes, h, w):
    top, left, hh, ww = boxes.numpy().T
    return bool(((top >= 0) & (left >= 0) & (hh >= 1) & (ww >= 1) & (top + hh <= h) & (left + ww <= w) & (hh == ww)).all())


@pytest.mark.parametrize("window", [1, 7, 40, 97, 500])
def test_unsmoothed_boxes_are_the_boxes_of_the_shifted_windows(walk, window):
    from implementation_phd_lab_vision_amd import track
    got = track.track_boxes(walk, IMG_H, IMG_W, window=window, smooth=1)
    assert got.dtype == torch.int64 and tuple(got.shape) == (N, 4)
    assert torch.equal(got, TR.boxes_unsmoothed(walk, IMG_H, IMG_W, window)) and _inside(got, IMG_H, IMG_W)
    if window < N:
        assert len({tuple(b) for b in got.tolist()}) > 1, "the subject crosses the image: the boxes move"
    # the ends are shifted, not truncated: the first window // 2 + 1 frames share the first window
    assert all(torch.equal(got[i], got[0]) for i in range(min(N, window // 2 + 1)))


@pytest.mark.parametrize("window,smooth", [(40, None), (40, 9), (7, 40), (1, 2), (97, 500), (12, 97)])
def test_smoothed_boxes_are_the_fraction_restatement(walk, window, smooth):
    from implementation_phd_lab_vision_amd import track
    got = track.track_boxes(walk, IMG_H, IMG_W, window=window, smooth=smooth)
    want = TR.boxes_smoothed(walk, IMG_H, IMG_W, window, window if smooth is None else smooth)
    assert torch.equal(got, want) and _inside(got, IMG_H, IMG_W)


def test_the_mean_does_not_depend_on_order_and_keeps_a_constant():
    from implementation_phd_lab_vision_amd import track
    big = np.array([1e8, 1.0, -1e8, 0.25, 3.0, 1e-3, 7.5], dtype=np.float32)
    a = track._windowed_mean(big, 500)
    b = track._windowed_mean(big[::-1].copy(), 500)
    assert np.array_equal(a, b[::-1]) and len(set(a.tolist())) == 1
    const = np.full(53, np.float32(0.1), dtype=np.float32)
    for w in (2, 3, 7, 40, 53, 99):
        assert np.array_equal(track._windowed_mean(const, w).view(np.int32), const.view(np.int32))


def test_a_whole_video_window_is_the_one_box_of_predict(walk):
    from implementation_phd_lab_vision_amd import predict, track
    one = predict.choose_box(IMG_H, IMG_W, joints2d=walk)
    for window, smooth in ((N, None), (N, 1), (500, None), (500, 13)):
        got = track.track_boxes(walk, IMG_H, IMG_W, window=window, smooth=smooth)
        assert torch.equal(got, one[None].expand(N, 4))
    assert torch.equal(track.TrackSettings(window=N).boxes(walk, IMG_H, IMG_W), one[None].expand(N, 4))


def test_a_subject_clamped_at_the_border_and_the_refusals(walk):
    from implementation_phd_lab_vision_amd import frames, track
    corner = walk - walk.min(axis=(0, 1)) - 5.0                       # the walk starts hanging over the top left corner
    got = track.track_boxes(corner, IMG_H, IMG_W, window=7)
    assert _inside(got, IMG_H, IMG_W) and got[0].tolist()[:2] == [0, 0] and int(got[:, 0].max()) == 0 and int(got[-1, 1]) > 0
    far = walk + np.float32(1000.0)                                   # wholly past the bottom right corner: pushed back inside
    got = track.track_boxes(far, IMG_H, IMG_W, window=7)
    assert _inside(got, IMG_H, IMG_W) and bool((got[:, 0] + got[:, 2] == IMG_H).all()) and bool((got[:, 1] + got[:, 3] == IMG_W).all())
    # a square larger than the image is the one case square_crop_from_2d leaves sticking out; the track mirrors it, and the pass refuses it
    wide = track.track_boxes(walk * np.float32(3.0), IMG_H, IMG_W, window=N, smooth=1)
    assert torch.equal(wide[0], frames.square_crop_from_2d(torch.from_numpy(walk * np.float32(3.0)), IMG_H, IMG_W)) and not _inside(wide, IMG_H, IMG_W)
    with pytest.raises(ValueError, match="does not lie inside"):
        track.check_boxes(wide, N, IMG_H, IMG_W)
    j = torch.from_numpy(walk[:5])
    lo, hi = torch.aminmax(j.reshape(-1, 2), dim=0)
    assert torch.equal(frames.square_crop_from_extent(lo, hi, IMG_H, IMG_W), frames.square_crop_from_2d(j, IMG_H, IMG_W))
    for bad in (walk[0], walk[:, :, :1], walk[:0]):
        with pytest.raises(ValueError):
            track.track_boxes(bad, IMG_H, IMG_W)
    for kw in (dict(window=0), dict(smooth=0), dict(window=-3)):
        with pytest.raises(ValueError):
            track.track_boxes(walk, IMG_H, IMG_W, **kw)
    for kw in (dict(window=0), dict(window=2.5), dict(smooth=0), dict(scale=0.0), dict(scale=float("nan"))):
        with pytest.raises(ValueError):
            track.TrackSettings(**kw)
    assert track.TrackSettings(7, 3).describe() == "window=7 smooth=3 scale=1.6" and track.TrackSettings(7).describe() == "window=7 smooth=7 scale=1.6"


# ---- the table and the C entry -----------------------------------------------------------------------------------------------------------
def test_box_table_rows_and_refusals(lib_built):
    from implementation_phd_lab_vision_amd import frames, track
    from oracle.resize_oracle import index_weights_int16
    c = TR.ragged_case(8)
    assert [TR.ragged_case(8, tail)["src_bytes"] % 4 for tail in TR.TAILS] == [1, 2, 3]
    t = track.BoxTable(c["offsets"], c["sizes"], c["boxes"], c["src_bytes"], 8, frames.RESIZE_FIXED)
    assert t.host.dtype == np.int64 and t.host.shape == (7, 9) and t.t == 7 and t.max_ww == 31 and t.table is None
    assert np.array_equal(t.host[:, 0], c["offsets"]) and np.array_equal(t.host[:, 1:3], c["sizes"]) and np.array_equal(t.host[:, 3:7], c["boxes"])
    assert t.host[:, 7].tolist() == [index_weights_int16(int(w), 8)[3] for w in c["boxes"][:, 3]]
    assert t.host[:, 8].tolist() == [index_weights_int16(int(h), 8)[3] for h in c["boxes"][:, 2]]
    f = track.BoxTable(c["offsets"], c["sizes"], c["boxes"], c["src_bytes"], 224, frames.RESIZE_FLOAT)
    assert f.host[:, 7:].tolist() == [[1, 1]] * 7
    one = track.BoxTable([0], [64, 80], [[0, 0, 64, 80]], 3 * 64 * 80)               # sizes (2,) for every row; the image fills the buffer
    assert one.t == 1 and one.max_ww == 80

    def refused(match, offsets=c["offsets"], sizes=c["sizes"], boxes=c["boxes"], src_bytes=c["src_bytes"], out_size=8, mode=0):
        with pytest.raises(ValueError, match=match):
            track.BoxTable(offsets, sizes, boxes, src_bytes, out_size, mode)

    def with_box(i, box):
        b = c["boxes"].copy()
        b[i] = box
        return b
    for i, box in ((0, [3, 5, 40, 76]), (0, [25, 5, 40, 8]), (1, [-1, 0, 3, 1]), (1, [0, -1, 3, 1]), (2, [4, 2, 0, 20]), (2, [4, 2, 1, 0]),
                   (6, [15, 18, 7, 5]), (6, [15, 18, 6, 6])):
        refused("does not lie inside its", boxes=with_box(i, box))
    refused("does not lie inside \\[0", src_bytes=c["src_bytes"] - 1)                  # the last image ends one byte past the buffer
    off = c["offsets"].copy()
    off[0] = -4
    refused("does not lie inside \\[0", offsets=off)
    off[0], off[3] = 0, c["src_bytes"] - 10
    refused("does not lie inside \\[0", offsets=off)
    refused("unexpected", offsets=c["offsets"].astype(np.float32))
    refused("unexpected", boxes=c["boxes"].astype(np.float64))
    refused("unexpected", boxes=c["boxes"][:, :3])
    refused("unexpected", boxes=c["boxes"][:6])
    refused("unexpected", sizes=c["sizes"][:6])
    refused("unexpected", offsets=c["offsets"][:, None])
    refused("unexpected", offsets=np.zeros(0, np.int64), sizes=np.zeros((0, 2), np.int64), boxes=np.zeros((0, 4), np.int64))    # t = 0
    refused("at least 1 x 1", sizes=np.where(np.arange(7)[:, None] == 4, 0, c["sizes"]))
    refused("out_size", out_size=6)
    refused("out_size", out_size=0)
    refused("mode", mode=2)
    refused("too wide", offsets=[0], sizes=[1, 30000], boxes=[[0, 0, 1, 30000]], src_bytes=90000)
    with pytest.raises(ValueError, match="no CPU fallback"):
        track.crop_resize_boxes_u8(c["buf"], t)


def test_every_refusal_of_the_c_entry_returns_before_any_launch(lib_built):
    """No device is needed: each call is refused on its arguments.  The pointers are made-up addresses that nothing dereferences."""
    src, table, out, flip = (0x1000000 * k for k in range(1, 5))
    ok = dict(src=src, src_bytes=1000, table=table, t=3, max_ww=20, out=out, flip=flip, out_size=8, mode=0)
    bad = (dict(src=None), dict(table=None), dict(out=None), dict(src=src + 1), dict(src=src + 2), dict(out=out + 2), dict(flip=flip + 1),
           dict(flip=out), dict(flip=out + 4), dict(flip=out + 3 * 3 * 8 * 8 - 4), dict(flip=out - 3 * 3 * 8 * 8 + 4), dict(table=table + 4), dict(t=0), dict(t=-1), dict(src_bytes=0), dict(src_bytes=-5), dict(src_bytes=1 << 40),
           dict(out_size=0), dict(out_size=2), dict(out_size=6), dict(out_size=4100), dict(out_size=-8), dict(mode=2), dict(mode=-1),
           dict(max_ww=0), dict(max_ww=-1), dict(max_ww=(160 * 1024 - 12) // 6 + 1), dict(max_ww=1 << 30),
           dict(t=1 << 28, out_size=8), dict(t=(1 << 31) // 224 + 1, out_size=224))
    for kw in bad:
        a = dict(ok, **kw)
        rc = lib_built.r50_op_crop_resize_boxes_u8(a["src"], a["src_bytes"], a["table"], a["t"], a["max_ww"], a["out"], a["flip"],
                                                   a["out_size"], a["mode"], None)
        assert rc == -1, (kw, rc)                                                    # R50_ERR_INVALID: refused, not a launch that failed
        assert b"r50_op_crop_resize_boxes_u8" in lib_built.r50_last_error(None), kw


# ---- the parser ----------------------------------------------------------------------------------------------------------------------------
def test_parser_flag_rules_and_unchanged_default_namespace(capsys):
    from implementation_phd_lab_vision_amd import predict, track
    base = ["--frames", "a.npz", "--model_path", "m", "--out", "o"]
    plain = predict.parse_args(base)
    assert sorted(vars(plain)) == PREDICT_KEYS and predict.video_track(plain) is None
    a = predict.parse_args(base + ["--track"])
    assert a.track is True and sorted(vars(a)) == sorted(PREDICT_KEYS + ["track"])
    assert predict.video_track(a) == track.TrackSettings(40, None)
    a = predict.parse_args(base + ["--track", "--seq-len", "16"])
    assert predict.video_track(a) == track.TrackSettings(16, None)                   # the window defaults to the head's
    a = predict.parse_args(base + ["--track", "--track-window", "25", "--track-smooth", "1", "--seq-len", "16"])
    assert predict.video_track(a) == track.TrackSettings(25, 1) and sorted(vars(a)) == sorted(PREDICT_KEYS + ["track", "track_window", "track_smooth"])
    for bad in (["--track-window", "5"], ["--track-smooth", "5"], ["--track", "--track-window", "0"], ["--track", "--track-smooth", "0"],
                ["--track", "--track-window", "2.5"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
    err = capsys.readouterr().err
    assert "--track-window needs --track" in err and "--track-smooth needs --track" in err


def test_load_input_reads_boxes(tmp_path):
    """(That ``--track`` without ``boxes`` and ``joints2d`` is refused before the backbone is built needs the device: the GPU test.)"""
    from implementation_phd_lab_vision_amd import predict
    frames = np.zeros((3, 8, 8, 3), np.uint8)
    boxes = np.array([[0, 0, 8, 8]] * 3)
    np.savez(tmp_path / "a.npz", frames=frames, boxes=boxes)
    item = predict.load_input(str(tmp_path / "a.npz"))
    assert np.array_equal(item["boxes"], boxes) and "joints2d" not in item


def test_the_product_never_imports_the_test_restatement():
    pkg = ROOT / "implementation_phd_lab_vision_amd"
    for path in [pkg / "track.py", pkg / "predict.py", ROOT / "scripts" / "bench_track.py"]:
        text = path.read_text()
        assert "track_reference" not in text and "from tests" not in text and "import tests" not in text, path
