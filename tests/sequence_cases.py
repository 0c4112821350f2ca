"""The clips, poses and frame tables of tests/test_sequences_gpu.py, which the evaluation rows of tests/rows/r50.py run as well."""
import numpy as np

T = 8
# 23 clips of 8 frames in two sequences: strides 1, 3 and 8 and a gap; frames with 1, 2, 3, ... 8 contributors, 91 frames (not a
# multiple of the 4 waves of a workgroup)
STARTS_A = [0, 1, 2, 3, 4, 5, 6, 7, 10, 13, 16, 24, 32, 50]
STARTS_B = [0, 8, 16, 19, 22, 23, 24, 27, 40]


def _clip(subject, action, cam, start, t=T):
    return {"subject": subject, "action": action, "cam": cam, "start": start, "end": start + t}


def _stitch_clips():
    clips = [_clip(9, "walk", 1, s) for s in STARTS_A] + [_clip(9, "sit", 2, s) for s in STARTS_B]
    order = np.random.default_rng(5).permutation(len(clips))
    return [clips[i] for i in order]


def _poses(clips, joints, seed):
    """pred (N, T, J, 3) random fp32; gt the same pose wherever two clips show one video frame, on a 2^-10 grid (so that + 0.25 is exact)."""
    rng = np.random.default_rng(seed)
    pred = (rng.standard_normal((len(clips), T, joints, 3)) * 0.4).astype(np.float32)
    truth = {}
    gt = np.zeros_like(pred)
    for i, c in enumerate(clips):
        for t in range(T):
            key = (c["action"], c["start"] + t)
            if key not in truth:
                truth[key] = (np.round(rng.standard_normal((joints, 3)) * 512.0) / 1024.0).astype(np.float32)
            gt[i, t] = truth[key]
    return pred, gt


# ------------------------------------------------------------------ sequence metrics ----------------------------------------------
def _metric_case(lengths, groups_of_seq, joints, seed, gap_in=None):
    """Frame rows of sequences of the given lengths (consecutive idx from a random first frame; ``gap_in = (s, k)`` skips one frame
    before row k of sequence s), random poses, spreads and contributor counts."""
    rng = np.random.default_rng(seed)
    seq, idx = [], []
    for s, n in enumerate(lengths):
        first = int(rng.integers(0, 50))
        frames = list(range(first, first + n))
        if gap_in is not None and gap_in[0] == s:
            frames = frames[:gap_in[1]] + [f + 1 for f in frames[gap_in[1]:]]
        seq += [s] * n
        idx += frames
    f = len(seq)
    counts = rng.integers(1, 4, size=f)
    return {"seq": np.array(seq, dtype=np.int32), "idx": np.array(idx, dtype=np.int32),
            "group": np.array([groups_of_seq[s] for s in seq], dtype=np.int32),
            "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
            "fused": (rng.standard_normal((f, joints, 3)) * 0.5).astype(np.float32),
            "gt": (rng.standard_normal((f, joints, 3)) * 0.5).astype(np.float32),
            "spread": rng.random(f).astype(np.float32)}
