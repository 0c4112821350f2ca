"""The crop + resize kernels over the domain they accept, on the MI355X: ``r50_op_crop_resize_u8`` (the frame producer) and
``r50_op_crop_resize_boxes_u8`` (``predict --track``) against oracle/resize_oracle.py on every case of tests/resize_cases.py --
non-square boxes, output sizes from 4 to 448 (at 344 and 448 the per-row item loop takes a second round), the identity on one axis
only, up-scaling on one axis with down-scaling on the other, different weight precisions on the two axes.  tests/test_resize_oracle_cpu.py
pins the oracle to torch on the same cases.  Every comparison is exact; no kernel is compared with another kernel.

  (a) producer, fixed mode    == the oracle's fixed-point restatement, and == ``F.interpolate`` on uint8 where the host has AVX
  (b) producer, float mode    == the oracle's restatement of the fp32 route
  (c) hflip / trev / both     == ``torch.flip`` of the ORACLE's plain result
  (d) ``out=``                a clip's slice of a poisoned batch buffer at out = 344
  (e) the tracked kernel      one table of all 15 sources per output size, packed at byte offsets of every residue mod 4, against the
                              oracle frame by frame, with the mirrored output; a table of the single row (1, 1)
  (f) byte offsets past 2^32  in one 2^32 + 2^20 byte allocation that is never filled
  (g) ``predict``             under a non-square box: the crops and the camera with two different zooms

and the rows ``ROWS_FRAMES_DOMAIN`` of tests/rows/frames_domain.py between poisoned guard bands (tests/guard_bands.py's harness) and late
on a side stream (tests/stream_order.py's)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from implementation_phd_lab_vision_amd import frames as F
from implementation_phd_lab_vision_amd import predict, track
from oracle import resize_oracle as ro
from tests import resize_cases as RC
from tests.guard_bands import run_row
from tests.rows.frames_domain import MODE_IDS, MODES, ROWS_FRAMES_DOMAIN, _table_want, _want
from tests.stream_order import run_row_late
from tests.test_track_gpu import CAM, STRIDE, T as SEQ, backbone, head, video  # noqa: F401  (fixtures: the synthetic backbone, head, walker)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
POISON = 0x7B
HAS_AVX = "AVX" in torch.backends.cpu.get_cpu_capability()


@pytest.fixture(scope="module")
def lib():
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    return _lib.load_library()


def _where(got, want):
    bad = torch.nonzero(got != want)
    return f"{bad.shape[0]} of {want.numel()} bytes differ, the first at (t, c, y, x) = {bad[0].tolist()}" if bad.numel() else "equal"


# ---------------------------------------------------------------- (a), (b): the producer --------------------------------------------------
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_producer_fixed_mode_is_the_oracle_over_the_domain(lib, case):
    hh, ww, out = case
    img = RC.image(hh, ww, out)
    tails = 0
    for name, top, left, pb, pr in RC.placements(hh, ww):
        clip, box = RC.embed(img, top, left, pb, pr)
        tails += RC.ends_at_the_last_byte(clip, box)
        got = F.crop_and_resize_video_uint8(clip.to(DEV), box, out, F.RESIZE_FIXED).cpu()
        assert got.shape == (RC.T, 3, out, out) and got.dtype == U8
        want = torch.from_numpy(ro.crop_and_resize_video_uint8(clip.numpy(), box, out, fixed_point=True))
        assert torch.equal(want, _want(hh, ww, out, F.RESIZE_FIXED))
        assert torch.equal(got, want), f"{name}: {_where(got, want)}"
        if HAS_AVX:                                                   # ATen's own uint8 kernel, when this host has it
            x = clip.permute(0, 3, 1, 2)[:, :, box[0]:box[0] + hh, box[1]:box[1] + ww]
            ref = TF.interpolate(x, size=[out, out], mode="bilinear", align_corners=False, antialias=False)
            assert torch.equal(got, ref), f"{name}: against F.interpolate {_where(got, ref)}"
    assert tails == 1, "one placement's box ends at the clip's last byte, off a dword boundary"


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_producer_float_mode_is_the_restatement_over_the_domain(lib, case):
    hh, ww, out = case
    img = RC.image(hh, ww, out)
    want = _want(hh, ww, out, F.RESIZE_FLOAT)
    for name, top, left, pb, pr in RC.placements(hh, ww):
        clip, box = RC.embed(img, top, left, pb, pr)
        got = F.crop_and_resize_video_uint8(clip.to(DEV), box, out).cpu()
        assert torch.equal(got, want), f"{name}: {_where(got, want)}"


# ---------------------------------------------------------------- (c): flips ---------------------------------------------------------------
def _flip_sources(out):
    return [(40, 8), (8, 40), (out, 37), (3 * out, 2 * out + 1)]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("out", [12, 344])
def test_flips_are_flips_of_the_oracle(lib, out, mode):
    """T = 3: the temporal reverse leaves the middle frame where it is and moves the outer two."""
    assert RC.T == 3
    for hh, ww in _flip_sources(out):
        assert (hh, ww) in RC.SOURCES(out)
        want = _want(hh, ww, out, mode)
        assert not torch.equal(want[0], want[2])
        for name, top, left, pb, pr in RC.placements(hh, ww):
            clip, box = RC.embed(RC.image(hh, ww, out), top, left, pb, pr)
            dev = clip.to(DEV)
            for hflip, trev, dims in ((True, False, [-1]), (False, True, [0]), (True, True, [0, -1])):
                got = F.crop_and_resize_video_uint8(dev, box, out, mode, hflip=hflip, trev=trev).cpu()
                ref = torch.flip(want, dims=dims)
                assert torch.equal(got, ref), f"{hh}x{ww} {name} hflip {hflip} trev {trev}: {_where(got, ref)}"


# ---------------------------------------------------------------- (d): out= ----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_out_slice_of_a_poisoned_batch_buffer(lib, mode):
    out = 344
    hh, ww = 3 * out, 2 * out + 1
    clip, box = RC.embed(RC.image(hh, ww, out), *RC.placements(hh, ww)[0][1:])
    batch = torch.full((3, RC.T, 3, out, out), POISON, dtype=U8, device=DEV)
    got = F.crop_and_resize_video_uint8(clip.to(DEV), box, out, mode, out=batch[1])
    assert got.data_ptr() == batch[1].data_ptr()
    host = batch.cpu()
    assert torch.equal(host[1], _want(hh, ww, out, mode)), _where(host[1], _want(hh, ww, out, mode))
    assert bool((host[0] == POISON).all()) and bool((host[2] == POISON).all()), "wrote outside the clip's slice"


# ---------------------------------------------------------------- (e): the tracked kernel ---------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("tail", [1, 2, 3], ids=lambda v: f"tail{v}")
@pytest.mark.parametrize("out", RC.OUTS)
def test_tracked_table_of_every_source_is_the_oracle(lib, out, tail, mode):
    """One table whose 15 rows are the sources of this output size: images of different sizes back to back at byte offsets of every
    residue mod 4, the last box ending at the buffer's last byte ``tail`` bytes past a dword boundary; 0xA5 bytes lie behind the buffer
    in the same allocation.  ``out`` and ``out_flip`` against the oracle and its ``flip(-1)``, frame by frame."""
    c = RC.packed_table(out, tail)
    n = len(c["frames"])
    assert n == 15 and c["src_bytes"] % 4 == tail
    room = torch.full((c["src_bytes"] + 64,), 0xA5, dtype=U8, device=DEV)
    room[:c["src_bytes"]] = c["buf"].to(DEV)
    buf = room[:c["src_bytes"]]
    assert buf.data_ptr() % 4 == 0
    table = track.BoxTable(c["offsets"], c["sizes"], c["boxes"], c["src_bytes"], out, mode, device=DEV)
    if mode == F.RESIZE_FIXED:
        assert len({(int(r[7]), int(r[8])) for r in table.host}) > 1 and any(int(r[7]) != int(r[8]) for r in table.host), "px != py in some row"
    guard = torch.full((2, n + 2, 3, out, out), POISON, dtype=U8, device=DEV)
    got, got_flip = track.crop_resize_boxes_u8(buf, table, out=guard[0, 1:n + 1], out_flip=guard[1, 1:n + 1])
    got, got_flip, host = got.cpu(), got_flip.cpu(), guard.cpu()
    want = _table_want(c, out, mode)
    for i, ((hh, ww), _fi) in enumerate(c["frames"]):
        assert torch.equal(got[i], want[i]), f"frame {i} ({hh}x{ww}): {_where(got[i][None], want[i][None])}"
        ref = torch.flip(want[i], dims=[-1])
        assert torch.equal(got_flip[i], ref), f"mirrored frame {i} ({hh}x{ww}): {_where(got_flip[i][None], ref[None])}"
    assert bool((host[:, 0] == POISON).all()) and bool((host[:, n + 1] == POISON).all()), "wrote outside the destination"
    assert bool((room[c["src_bytes"]:] == 0xA5).all())


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("out", RC.OUTS)
def test_tracked_table_of_the_single_row_1x1(lib, out, mode):
    """A table of one row whose box is one pixel, the last pixel of its image and of the buffer (27 bytes: 3 past a dword boundary)."""
    c = RC.packed_table(out, 3, sources=[(1, 1)])
    assert c["src_bytes"] == 27 and c["boxes"].tolist() == [[2, 2, 1, 1]]
    table = track.BoxTable(c["offsets"], c["sizes"], c["boxes"], c["src_bytes"], out, mode, device=DEV)
    got, got_flip = track.crop_resize_boxes_u8(c["buf"].to(DEV), table, flip=True)
    want = _table_want(c, out, mode)
    assert torch.equal(want, RC.image(1, 1, out)[0, 0, 0].view(1, 3, 1, 1).expand(1, 3, out, out)), "one pixel resizes to a constant plane"
    assert torch.equal(got.cpu(), want) and torch.equal(got_flip.cpu(), want)


# ---------------------------------------------------------------- (f): byte offsets past 2^32 -----------------------------------------------
def test_byte_offsets_past_2_to_the_32(lib):
    """One allocation of 2^32 + 2^20 bytes, never filled.  A truncated offset would read lower in the same allocation: nothing here can
    leave it.  The tracked kernel finds an image at byte 2^32 + 7; the producer finds a crop in the bottom-right corner of frame 2 of three
    frames of 21846 x 21846 (1.43 GB a frame: frame 2 starts above 2^31 and ends above 2^32).  Only what the written bytes define is
    compared."""
    big = 1 << 32
    nbytes = big + (1 << 20)
    out = 12
    room = torch.empty((nbytes,), dtype=U8, device=DEV)
    try:
        assert room.data_ptr() % 4 == 0
        # the tracked kernel: two rows, (63, 79) at byte 5 and (23, 76) at byte 2^32 + 7
        rows = [((63, 79), 5), ((23, 76), big + 7)]
        offsets, sizes, boxes = [], [], []
        for (hh, ww), at in rows:
            clip, box = RC.embed(RC.image(hh, ww, out), *RC.placements(hh, ww)[0][1:])
            h, w = int(clip.shape[1]), int(clip.shape[2])
            assert at + 3 * h * w <= nbytes
            room[at:at + 3 * h * w] = clip[1].reshape(-1).to(DEV)
            offsets.append(at); sizes.append([h, w]); boxes.append(box)
        for mode in MODES:
            table = track.BoxTable(np.asarray(offsets, np.int64), np.asarray(sizes, np.int64), np.asarray(boxes, np.int64), nbytes, out, mode,
                                   device=DEV)
            got = track.crop_resize_boxes_u8(room, table).cpu()
            for i, ((hh, ww), at) in enumerate(rows):
                want = _want(hh, ww, out, mode)[1]
                assert torch.equal(got[i], want), f"mode {mode}, image at byte {at}: {_where(got[i][None], want[None])}"
        # the producer: T = 3 frames of 21846 x 21846, a 40 x 8 crop in the bottom-right corner of frame 2
        side, t, hh, ww = 21846, 3, 40, 8
        frame_bytes = side * side * 3
        assert t * frame_bytes <= nbytes and 2 * frame_bytes > (1 << 31) and t * frame_bytes > big
        clip = room[:t * frame_bytes].view(t, side, side, 3)
        img = RC.image(hh, ww, out)
        clip[2, side - hh:, side - ww:] = img[2].to(DEV)
        box = [side - hh, side - ww, hh, ww]
        for mode in MODES:
            want = _want(hh, ww, out, mode)[2]
            got = F.crop_and_resize_video_uint8(clip, box, out, mode)[2].cpu()
            assert torch.equal(got, want), f"mode {mode}: frame 2 {_where(got[None], want[None])}"
            got = F.crop_and_resize_video_uint8(clip, box, out, mode, trev=True)[0].cpu()
            assert torch.equal(got, want), f"mode {mode}, trev: frame 2 as output frame 0 {_where(got[None], want[None])}"
    finally:
        del room
        clip = None
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- (g): predict under a non-square box ---------------------------------------
def test_predict_under_a_non_square_box(backbone, head, video):  # noqa: F811
    fr, _j2d = video
    fr = fr[:23]
    box = [3, 10, 80, 50]
    p = predict.VideoPredictor(backbone, head, seq_len=SEQ, stride=STRIDE, frame_batch=16)
    pics = p.crops(fr, box, 0, 23).cpu()
    x = np.transpose(fr.numpy(), (0, 3, 1, 2))[:, :, 3:83, 10:60]
    want = torch.from_numpy(ro.resize_bilinear_u8_float_restated(x, 224, 224)).permute(0, 2, 3, 1)
    assert pics.shape == (23, 224, 224, 3) and torch.equal(pics, want), _where(pics.permute(0, 3, 1, 2), want.permute(0, 3, 1, 2))
    res = p.predict(fr, box=box, cam=CAM)
    k = F.adjust_camera_after_crop_and_resize(CAM, box).numpy()
    assert res["box"].tolist() == box and res["K"].shape == (3, 3) and np.array_equal(res["K"], k)
    assert k[0, 0] == np.float32(1100.0) * np.float32(224 / 50) and k[1, 1] == np.float32(1150.0) * np.float32(224 / 80), "two different zooms"
    assert res["joints3d"].shape == (23, 17, 3) and np.isfinite(res["joints3d"]).all()


# ---------------------------------------------------------------- guard bands and stream order ----------------------------------------------
@pytest.mark.parametrize("row", ROWS_FRAMES_DOMAIN, ids=[r.id for r in ROWS_FRAMES_DOMAIN])
def test_frames_domain_between_guard_bands(row):
    run_row(row)


@pytest.mark.parametrize("row", ROWS_FRAMES_DOMAIN, ids=[r.id for r in ROWS_FRAMES_DOMAIN])
def test_frames_domain_late_on_a_side_stream(row):
    run_row_late(row)
