"""Dense evaluation without a GPU: the host sequence table against the loop oracle of
``tests/stitch_reference.py``, its invariants, the chunking, the host-side refusals and the CLI flags."""
import random

import numpy as np
import pytest

from tests import results_data as rd
from tests import stitch_reference as ref


def _clip(subject, action, cam, start, t):
    return {"subject": subject, "action": action, "cam": cam, "start": start, "end": start + t, "shard_id": 0, "row": 0}


def ragged_clips(t=6):
    """Two sequences: (9, walk, 1) with starts 0, 2, 2 (a duplicate clip), 4 and then a gap (start 20), cam given as 1 and "1";
    (9, sit, 2) is a single clip.  Shuffled."""
    clips = [_clip(9, "walk", 1, 0, t), _clip(9, "walk", "1", 2, t), _clip(9, "walk", "1", 2, t), _clip(9, "walk", 1, 4, t),
             _clip(9, "walk", "1", 20, t), _clip(9, "sit", 2, 7, t)]
    random.Random(3).shuffle(clips)
    return clips


def _assert_table_equals_oracle(clips, t):
    from implementation_phd_lab_vision_amd.sequences import SequenceTable
    got, want = SequenceTable.from_clips(clips, t), ref.table(clips, t)
    for name in ("seq", "idx", "seq_start", "offsets", "src"):
        g = getattr(got, name)
        assert g.dtype == np.int32 and np.array_equal(g, want[name]), name
    assert got.seq_keys == want["seq_keys"]
    return got


def results_layout_clips(n=rd.N_S9):
    """``tests/results_data``'s layout -- clip c shows video c % 6 from frame 4 * (c // 6) -- with one spelling of cam per video."""
    videos = list(rd.VIDEOS)
    return [_clip(9, videos[c % 6][0], videos[c % 6][1], 4 * (c // 6), rd.SEQ_LEN) for c in range(n)]


def test_table_on_the_results_layout():
    own = _assert_table_equals_oracle([rd.clip_meta(c) for c in range(rd.N_S9)], rd.SEQ_LEN)
    assert len(own.seq_keys) == rd.N_S9 and own.frames == rd.N_S9 * rd.SEQ_LEN      # cam 1 and "cam_1": str(cam) keeps them apart
    tbl = _assert_table_equals_oracle(results_layout_clips(), rd.SEQ_LEN)
    assert len(tbl.seq_keys) == 6 and tbl.seq_keys[0] == (9, "act0", "1")          # six videos
    counts = np.diff(tbl.offsets)
    assert set(counts.tolist()) == {1, 2}                                           # stride 4 of 8 frames: halves overlap
    assert tbl.frames == 5 * 12 + 8 and tbl.clips == rd.N_S9                        # five videos with two clips, one with one


def test_table_on_a_ragged_case():
    t = 6
    clips = ragged_clips(t)
    tbl = _assert_table_equals_oracle(clips, t)
    assert tbl.seq_keys == [(9, "sit", "2"), (9, "walk", "1")]
    walk = tbl.idx[tbl.seq_start[1]:tbl.seq_start[2]].tolist()
    assert walk == list(range(0, 10)) + list(range(20, 26))                         # the gap stays a gap
    assert int(np.diff(tbl.offsets).max()) == 4                                     # frames 4, 5: starts 0, 2, 2, 4


@pytest.mark.parametrize("case", ["results", "ragged"])
def test_table_invariants(case):
    from implementation_phd_lab_vision_amd.sequences import SequenceTable
    t = rd.SEQ_LEN if case == "results" else 6
    clips = results_layout_clips() if case == "results" else ragged_clips(t)
    tbl = SequenceTable.from_clips(clips, t)
    assert sorted(tbl.src.tolist()) == list(range(len(clips) * t))                  # every (item, t) once
    assert tbl.offsets[0] == 0 and tbl.offsets[-1] == len(clips) * t and np.all(np.diff(tbl.offsets) >= 1)
    for r in range(tbl.frames):
        rows = tbl.src[tbl.offsets[r]:tbl.offsets[r + 1]]
        items, ts = rows // t, rows % t
        starts = [int(clips[i]["start"]) for i in items]
        assert all(s + k == tbl.idx[r] for s, k in zip(starts, ts))                 # each contributor shows this very frame
        assert all(tbl.seq_keys[tbl.seq[r]][1] == clips[i]["action"] for i in items)
        order = list(zip(starts, items.tolist()))
        assert order == sorted(order) and ts.tolist() == sorted(ts.tolist(), reverse=True)


@pytest.mark.parametrize("max_clips", [1, 2, 4, 5, 100])
def test_chunks_keep_sequences_whole(max_clips):
    from implementation_phd_lab_vision_amd.sequences import SequenceTable
    t = 6
    clips = ragged_clips(t) + [_clip(11, "walk", 1, 3 * k, t) for k in range(3)]
    tbl = SequenceTable.from_clips(clips, t)
    chunks = tbl.chunks(max_clips)
    assert [c.seq0 for c in chunks] == sorted(c.seq0 for c in chunks) and chunks[0].seq0 == 0
    assert sum(len(c.table.seq_keys) for c in chunks) == len(tbl.seq_keys)
    assert sorted(np.concatenate([c.items for c in chunks]).tolist()) == list(range(len(clips)))
    per_seq = np.bincount(tbl.item_seq)
    for c in chunks:
        n = len(c.items)
        assert n <= max_clips or len(c.table.seq_keys) == 1                         # a longer sequence is a run of its own
        assert n == per_seq[c.seq0:c.seq0 + len(c.table.seq_keys)].sum()
        assert c.table.src.min() >= 0 and c.table.src.max() < n * t                 # inside the chunk's own buffer
        assert sorted(c.table.src.tolist()) == list(range(n * t))
        want = ref.table([clips[i] for i in c.items], t)                            # the chunk alone, tabled afresh
        for name in ("seq", "idx", "seq_start", "offsets", "src"):
            assert np.array_equal(getattr(c.table, name), want[name]), name
        assert c.table.seq_keys == want["seq_keys"] == tbl.seq_keys[c.seq0:c.seq0 + len(want["seq_keys"])]
        f1 = c.frame0 + c.table.frames
        assert np.array_equal(tbl.idx[c.frame0:f1], c.table.idx) and np.array_equal(tbl.seq[c.frame0:f1] - c.seq0, c.table.seq)
    if max_clips >= len(clips):
        assert len(chunks) == 1
    if max_clips == 1:
        assert len(chunks) == len(tbl.seq_keys)


def test_refusals_on_the_host():
    from implementation_phd_lab_vision_amd import sequences as sq
    with pytest.raises(ValueError, match="seq_len"):
        sq.SequenceTable.from_clips([_clip(9, "walk", 1, 0, 6), _clip(9, "walk", 1, 2, 5)], 6)
    with pytest.raises(ValueError):
        sq.SequenceTable.from_clips([], 6)
    with pytest.raises(ValueError):
        sq.SequenceTable.from_clips(ragged_clips(6), 6).chunks(0)

    class Augmented:
        augment = True

    with pytest.raises(ValueError, match="augment"):
        sq.evaluate_dense(None, Augmented())
    i32 = lambda *v: np.array(v, dtype=np.int32)                                    # noqa: E731
    for offsets, src in ((i32(0, 2, 1, 3), i32(0, 1, 2)),                          # a decreasing offset
                         (i32(1, 2, 3), i32(0, 1, 2)),                              # not from 0
                         (i32(0, 2, 2), i32(0, 1, 2)),                              # not to len(src)
                         (i32(0, 1, 3), i32(0, 1, 8)),                              # src past the rows
                         (i32(0, 1, 3), i32(0, -1, 2)),
                         (np.array([0, 3]), i32(0, 1, 2))):                          # not int32
        with pytest.raises(ValueError):
            sq.StitchIndex(offsets, src, 8, "cpu")
    ok = sq.StitchIndex(i32(0, 1, 1, 3), i32(7, 0, 7), 8, "cpu")                    # an empty list and a repeat are allowed
    assert ok.frames == 3 and ok.rows == 8


def test_item_clips_accessor(tmp_path):
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from implementation_phd_lab_vision_amd.sequences import SequenceTable
    store = DeviceFeatureStore(str(rd.make_results_cache(tmp_path / "features")), subjects=[9], test_set=True, device="cpu")
    clips = store.item_clips()
    assert len(clips) == len(store) == rd.N_S9 and [str(c["action"]) for c in clips] == store.item_actions()
    for i, c in enumerate(clips):
        meta = store[i][4]
        assert (c["subject"], c["action"], c["cam"], c["start"], c["end"]) == tuple(meta[k] for k in ("subject", "action", "cam", "start", "end"))
    assert SequenceTable.from_clips(clips, rd.SEQ_LEN).clips == rd.N_S9


def test_dense_flags_parse(capsys):
    from implementation_phd_lab_vision_amd import results
    base = ["--features_root", "f", "--preprocessed_root", "p", "--model_path", "m"]
    args = results.parse_args(base)
    assert (args.dense, args.dense_fuse, args.dense_out) == (False, "context", None)
    args = results.parse_args(base + ["--dense", "--dense-fuse", "last", "--dense-out", "seq.npz"])
    assert (args.dense, args.dense_fuse, args.dense_out) == (True, "last", "seq.npz")
    assert results.parse_args(base + ["--dense", "--dense-fuse", "mean"]).dense_fuse == "mean"
    for bad in (["--dense", "--dense-fuse", "median"], ["--dense-out", "seq.npz"]):  # another word; an export without the pass
        with pytest.raises(SystemExit):
            results.parse_args(base + bad)
    capsys.readouterr()
