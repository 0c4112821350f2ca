"""Every op on a side stream with late inputs, and which ops hold the host.

The harness is tests/stream_order.py (read its docstring first).  Here:

  controls   the harness sees, on the stream ``choose_stream`` returned, a launch misdirected to stream 0 and a missing join, and passes an
             honest call.  They run first: the table tests use the stream they validate.
  the table  every row of the tables ``r50``, ``smooth`` and ``hal`` of tests/rows/ (the other headers' rows run late from their own
             test files) runs once plainly on the default stream and once in a ``LateArena`` on the side
             stream, from the same payloads.  Every op claims the same bits on every run, so for every result: snapshot bits == final
             bits == plain bits, and no defined output holds the poison.  No tolerance enters.
  blocking   ``BLOCKS_HOST`` lists the rows that may hold the host until the sleep has ended.  A row outside it that does fails; an
             entry that does not is stale and fails too.  No op of the per-step hot paths (tests/golden/train_launch_sequences.json,
             tests/golden/backbone_launch_plan.json) may be listed, and at most 10 % of the rows.
  wrappers   the Python entry points, default stream against side stream with late tensor inputs, bit-equal.

What this cannot see: a write-side race that happens to finish in time (the snapshot and the overwritten inputs can only fail, never
prove); for a row in ``BLOCKS_HOST``, the launches after the op's internal synchronisation: by then the input has arrived; and, among the
wrappers, whatever follows a host read: ``add_protocol_sums`` / ``add_detail_sums`` / ``add_dtw_sums`` (they read ``group`` before they
launch) and, in ``train_step``, everything after step 1's overflow-flag read.  There only the bits on a side stream are held.
"""
import pytest
import torch

from tests import guard_bands as G
from tests import stream_order as SO
from tests.guard_bands import DEV, lib
from tests.rows import TABLES as EVERY_TABLE
from tests.stream_order import check_blocking_table, run_row_late, side_against_default

pytestmark = pytest.mark.gpu

TABLES = tuple((name, dict(EVERY_TABLE)[name]) for name in ("r50", "smooth", "hal"))
ALL_ROWS = [row for _name, table in TABLES for row in table]
FAMILIES = sorted({row.family for row in ALL_ROWS})

# ------------------------------------------------------------------------------------------------------------------------------
# a. controls (first in the module: the table tests use the stream they validate)
# ------------------------------------------------------------------------------------------------------------------------------
def test_control_a_launch_misdirected_to_stream_0_shows():
    side, tried = SO.choose_stream(lib())
    print(f"choose_stream: {tried} candidate(s) tried")
    late, want = SO.cast_rows_probe(lib(), side, SO.calibrate(), "stream0")
    snap = late.snapshots["dst"]
    assert not late.blocked
    assert torch.isnan(snap).any(), "the op ran on stream 0 during the sleep and still saw its input"
    assert not torch.equal(G.bits(snap), want), "a launch on stream 0 gave the default-stream bits: the harness would not see it"


def test_control_a_missing_join_shows():
    side, _ = SO.choose_stream(lib())
    second, tried = SO.choose_second_stream(lib())
    print(f"choose_second_stream: {tried} candidate(s) tried")
    late, want = SO.cast_rows_probe(lib(), side, SO.calibrate(), "no_join", other=second)
    snap = late.snapshots["dst"]
    assert not late.blocked
    assert G.holds_fill(snap, late.fill) == snap.numel(), "the snapshot on the side stream already holds what the unjoined stream wrote"
    assert torch.equal(G.bits(late.results["dst"]), want), "the unjoined stream never wrote the result"


def test_control_an_honest_call_passes():
    side, _ = SO.choose_stream(lib())
    late, want = SO.cast_rows_probe(lib(), side, SO.calibrate(), "honest")
    assert not late.blocked, "the host was held until the sleep ended: the sleep is too short, see calibrate()"
    assert torch.equal(G.bits(late.snapshots["dst"]), want) and torch.equal(G.bits(late.results["dst"]), want)


# ------------------------------------------------------------------------------------------------------------------------------
# b. + c. every row, late on the side stream; which rows hold the host
# ------------------------------------------------------------------------------------------------------------------------------
def _rows_of(family):
    rows = [r for r in ALL_ROWS if r.family == family]
    return pytest.mark.parametrize("row", rows, ids=[r.id for r in rows])


def _table_test(family):
    @_rows_of(family)
    def test(row):
        run_row_late(row)
    test.__name__ = test.__qualname__ = f"test_late_on_a_side_stream_{family}"
    test.__doc__ = f"Family `{family}`: side stream, late inputs: the default-stream bits, and no host synchronisation outside BLOCKS_HOST."
    return test


for _family in FAMILIES:
    globals()[f"test_late_on_a_side_stream_{_family}"] = _table_test(_family)


def test_the_blocking_table_keeps_its_conditions():
    check_blocking_table(ALL_ROWS)


# ------------------------------------------------------------------------------------------------------------------------------
# e. the Python entry points: side stream with late tensor inputs against the default stream, bit-equal
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_head_forward_and_rollout_on_a_side_stream(precision):
    from tests.test_rollout_gpu import _head
    head, _sd = _head(128, 2, 7, precision)
    feats = torch.rand(3, 7, 2048, generator=torch.Generator().manual_seed(3))
    other = torch.rand(3, 7, 2048, generator=torch.Generator().manual_seed(4)).to(DEV)
    late = side_against_default(f"PHDFor3DJoints.forward {precision}", lambda _w, d: head.forward(d["feats"], predict_future=True), {"feats": feats},
                                scrub=lambda: head.forward(other, predict_future=True))
    assert not late.blocked, "the head's forward held the host"
    late = side_against_default(f"PHDFor3DJoints.rollout {precision}", lambda _w, d: head.rollout(d["feats"], 4, 3), {"feats": feats},
                                scrub=lambda: head.rollout(other, 4, 3))
    assert not late.blocked, "the head's rollout held the host"


def test_two_eager_train_steps_on_a_side_stream():
    """Flat parameters, optimiser state and the loss after two eager steps with explicit dropout masks, from two heads built alike before
    either run.  Late are the launches of step 1 up to its first host read: the whole ``forward_backward`` (asserted: the sleep had not
    ended when it returned) and ``_finish_step``'s finite check.  ``_finish_step`` then reads the overflow flag on the host, as the
    reference's scaler does, and ``train_step`` the loss: the optimiser launch of step 1 and all of step 2 run with their inputs
    complete, and for them the check is the bits on a side stream alone."""
    from implementation_phd_lab_vision_amd import train
    from tests.test_head_train_gpu import _head
    b, t = 2, 5
    g = torch.Generator().manual_seed(11)
    inputs, steps = {}, 2
    heads = {}
    for which in ("default", "side"):
        m, _sd = _head((128, 2), 5)
        heads[which] = (m, train.AdamW(m, lr=3e-4), train.GradScaler(init_scale=1024.0))
    dg = torch.Generator(device=DEV).manual_seed(12)
    for s in range(steps):
        inputs[f"feats{s}"] = torch.rand(b, t, 2048, generator=g)
        inputs[f"gt{s}"] = torch.randn(b, t, 17, 3, generator=g) * 0.3
        for name, mask in heads["default"][0].make_dropout_masks(b, t, generator=dg).items():
            inputs[f"mask{s}:{name}"] = mask.cpu()
    torch.cuda.synchronize()                          # both heads' uploads are complete before either run
    losses, sleep_over = {}, []

    def call(late, d):
        which = "default" if late is None else "side"
        m, optim, scaler = heads[which]
        if late is not None:
            inner = m.forward_backward

            def watched(*args, **kwargs):
                out = inner(*args, **kwargs)
                sleep_over.append(bool(late.sleep_done.query()))
                return out
            m.forward_backward = watched
        out = []
        for s in range(steps):
            masks = {k.split(":", 1)[1]: v for k, v in d.items() if k.startswith(f"mask{s}:")}
            out.append(m.train_step(d[f"feats{s}"], d[f"gt{s}"], optim, scaler, masks=masks))
        losses[which] = out
        return {"flat_master": m.flat_master, "flat_w16": m.flat_w16, "flat_grad": m.flat_grad, "exp_avg": optim.exp_avg,
                "exp_avg_sq": optim.exp_avg_sq}

    side_against_default("TrainableHead.train_step x 2", call, inputs)
    assert len(sleep_over) == steps and not sleep_over[0], \
        f"step 1's forward_backward returned after the sleep had ended {sleep_over}: it held the host, and its launches were not late"
    assert losses["side"] == losses["default"] and not any(skipped for _l, _m, skipped in losses["default"]), losses


def test_backbone_features_on_a_side_stream():
    from implementation_phd_lab_vision_amd.backbone import ResNet50Backbone
    from implementation_phd_lab_vision_amd.weights import synthetic_state_dict
    bb = ResNet50Backbone(state_dict=synthetic_state_dict(0), max_batch=4).to(DEV).eval()
    try:
        g = torch.Generator().manual_seed(21)
        u8 = torch.randint(0, 256, (3, 3, 224, 224), generator=g, dtype=torch.uint8)
        other = torch.randint(0, 256, (3, 3, 224, 224), generator=g, dtype=torch.uint8).to(DEV)
        late = side_against_default("ResNet50Backbone.features_u8 n 3", lambda _w, d: bb.features_u8(d["x_u8"]), {"x_u8": u8},
                                    scrub=lambda: bb.features_u8(other))
        assert not late.blocked, "features_u8 held the host"
        # the two forks inside r50_forward, which the default options do not take: the batch split over the handle's `side[k]` streams
        # (streams = 2 needs m >= 4 frames), and the downsample convs of layer2.0 / 3.0 / 4.0 on `ds_stream` (overlap_ds, with the
        # conv3 + downsample fusion off).  Both streams are non-blocking: without the fork event they would read the frames, or the block
        # input, before the caller's stream has produced them.
        u8_4 = torch.randint(0, 256, (4, 3, 224, 224), generator=g, dtype=torch.uint8)
        other4 = torch.randint(0, 256, (4, 3, 224, 224), generator=g, dtype=torch.uint8).to(DEV)
        bb.set_option("streams", 2)
        late = side_against_default("ResNet50Backbone.features_u8 n 4, streams 2", lambda _w, d: bb.features_u8(d["x_u8"]), {"x_u8": u8_4},
                                    scrub=lambda: bb.features_u8(other4))
        assert not late.blocked, "features_u8 over two internal streams held the host"
        bb.set_option("streams", 1)
        bb.set_option("overlap_ds", 1)
        bb.set_option("fuse_ds_cat", 0)
        late = side_against_default("ResNet50Backbone.features_u8 n 3, overlap_ds", lambda _w, d: bb.features_u8(d["x_u8"]), {"x_u8": u8},
                                    scrub=lambda: bb.features_u8(other))
        assert not late.blocked, "features_u8 with the downsample branch on its own stream held the host"
        bb.set_option("streams", 2)
        late = side_against_default("ResNet50Backbone.features_u8 n 4, overlap_ds + streams 2", lambda _w, d: bb.features_u8(d["x_u8"]), {"x_u8": u8_4},
                                    scrub=lambda: bb.features_u8(other4))
        assert not late.blocked
        bb.set_option("streams", 1)
        bb.set_option("overlap_ds", 0)
        bb.set_option("fuse_ds_cat", 1)
        video = torch.randint(0, 256, (4, 300, 320, 3), generator=g, dtype=torch.uint8)
        late = side_against_default("ResNet50Backbone.features_from_video 4 x 300 x 320",
                                    lambda _w, d: bb.features_from_video(d["frames"], [20, 30, 250, 250]), {"frames": video},
                                    scrub=lambda: bb.features_u8(other))
        assert not late.blocked, "features_from_video held the host"
    finally:
        bb.close()


def test_evaluation_wrappers_on_a_side_stream():
    """sequences' stitch + metrics, baselines' row norm + search and smooth.PostProcess with late inputs; protocols, detail_metrics and dtw
    read ``group.min()`` / ``max()`` on the host BEFORE their one launch, so their inputs have arrived when it is enqueued: for these three
    the late-input side checks nothing, and what is held is the bits on a side stream (their ops are late in the table above)."""
    import numpy as np
    from implementation_phd_lab_vision_amd import baselines, detail_metrics, dtw, protocols, sequences, smooth
    from tests import baselines_reference as br
    from tests import detail_reference as dr
    from tests.rows.r50 import _detail_make, _dtw_make, _seq_make, _stitch_make
    F64 = torch.float64

    b, p, t_gt, i0, j, ng, root, n_thr = case = (5, 3, 7, 2, 17, 4, 0, 31)
    pred, gt, group = _detail_make(case)

    def proto(_w, d):
        protocols.add_protocol_sums(d["pred"], d["gt"], i0, d["group"], ng, d["acc"], root)
        return d["acc"]
    side_against_default("protocols.add_protocol_sums", proto, {"pred": pred, "gt": gt, "group": group, "acc": torch.zeros(2 * ng * p + ng, dtype=F64)})

    def detail(_w, d):
        detail_metrics.add_detail_sums(d["pred"], d["gt"], i0, d["group"], ng, d["acc"], root, n_thr, dr.THR_MAX)
        return d["acc"]
    side_against_default("detail_metrics.add_detail_sums", detail,
                         {"pred": pred, "gt": gt, "group": group, "acc": torch.zeros(dr.acc_size(ng, p, j), dtype=F64)})

    b, p, q, t_gt, i0d, j, ngd, rootd, band = dcase = (4, 5, 3, 3, 0, 17, 2, 0, 2)
    dpred, dgt, dgroup = _dtw_make(dcase)

    def warp(_w, d):
        clip = dtw.add_dtw_sums(d["pred"], d["gt"], i0d, q, d["group"], ngd, d["acc"], band, rootd)
        return {"acc": d["acc"], "clip_out": clip}
    side_against_default("dtw.add_dtw_sums", warp, {"pred": dpred, "gt": dgt, "group": dgroup, "acc": torch.zeros(dtw.acc_size(ngd, p), dtype=F64)})

    spred, sgt, offsets, src = _stitch_make()
    index = sequences.StitchIndex(offsets.numpy(), src.numpy(), spred.shape[0] * spred.shape[1], DEV)      # host tables: checked and uploaded once
    torch.cuda.synchronize()
    late = side_against_default("sequences.stitch_poses", lambda _w, d: sequences.stitch_poses(d["pred"], d["gt"], index, "context", 5),
                                {"pred": spred, "gt": sgt})
    assert not late.blocked, "stitch_poses held the host"
    seq = _seq_make()
    late = side_against_default("sequences.sequence_metrics",
                                lambda _w, d: sequences.sequence_metrics(d["fused"], d["gt"], d["spread"], d["offsets"], d["seq"], d["idx"], d["group"], 4),
                                seq)
    assert not late.blocked, "sequence_metrics held the host"

    def search(_w, d):
        xn = baselines.row_norm2(d["x"])
        idx, dist2 = baselines.nn_search(d["q"], d["x"], xn, 3)
        return {"x_norm2": xn, "idx": idx, "dist2": dist2}
    late = side_against_default("baselines.row_norm2 + nn_search", search, {"q": br.rows16((5, 64), 1, "fp16"), "x": br.rows16((300, 64), 0, "fp16")})
    assert not late.blocked, "row_norm2 + nn_search held the host"

    seq_start, idx = np.array([0, 30, 60], dtype=np.int32), np.concatenate([np.arange(30), np.arange(30)]).astype(np.int32)
    tables = smooth.DeviceTables(seq_start, idx, DEV)
    post = smooth.PostProcess(kind="gauss", fix_bones=True)
    poses = torch.randn((60, 17, 3), generator=torch.Generator().manual_seed(9)) * 0.3 + torch.tensor([0.0, 0.0, 5.0])

    def smoothed(_w, d):
        out, info = post.apply(d["poses"], tables)
        return {"out": out, "short_rows": info["short_rows"], "stats": info["stats"]}
    late = side_against_default("smooth.PostProcess gauss + bones", smoothed, {"poses": poses})       # the FIR table went up in the default run
    assert not late.blocked, "PostProcess.apply held the host"
