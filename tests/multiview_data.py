"""Fixtures of the multi-view tests: rigid ground truths seen by several cameras, as a fabricated ``evaluate_dense`` result and as a small
S9 feature cache written with the project's shard packer (two takes of three cameras each, videos of unequal length).

The ground truth of camera c is ``world @ R_c^T + t_c`` rounded to fp32: the cameras' poses are rigid images of each other to within
that rounding, as Human3.6M's are."""
from pathlib import Path

import numpy as np
import torch

from implementation_phd_lab_vision_amd.shards import ShardPacker
from tests import multiview_reference as MR

SEQ_LEN = 8
STRIDE = 4
FRAME_SKIP = 2
# (action, cam) -> frames of the video; the clips start every STRIDE frames
VIDEOS = {("act0", 1): 20, ("act0", 2): 20, ("act0", 3): 16, ("act1 1", 1): 12, ("act1 1", 2): 16, ("act1 1", 3): 12}


def world_motion(frames: int, joints: int, rng: np.random.Generator, scale: float = 0.3) -> np.ndarray:
    """(frames, joints, 3) fp64: a body of about ``scale`` spread that turns and drifts smoothly."""
    body = rng.standard_normal((joints, 3)) * scale
    t = np.arange(frames)[:, None, None]
    return body + 0.15 * scale * np.sin(0.3 * t + rng.uniform(0, 6.28, (joints, 3))) + 0.02 * scale * t * rng.standard_normal(3)


def camera(rng: np.random.Generator, depth: float = 5.0):
    """(R, t): a random rotation and a translation that puts the body about ``depth`` in front of the camera."""
    return MR.random_rotation(rng), np.array([0.0, 0.0, depth]) + 0.1 * depth * rng.standard_normal(3) * [1.0, 1.0, 0.2]


def make_dense(seed: int = 0, joints: int = 17, common: float = 0.03, noise: float = 0.02, shifted=None):
    """A fabricated ``evaluate_dense(keep_poses=True)`` result in metres: take (9, "walk") with four cameras over frames 10..59 (one
    starts late, one ends early, one has a gap), take (9, "sit 1") with two cameras, take (11, "walk") with one.  pred = gt + a common
    error (the same world-space error seen by every camera: fusion cannot remove it) + independent noise per view (fusion averages it).
    ``shifted = (take index, camera index)``: that camera's ground truth and prediction are those of the NEXT frame, a wrong index."""
    rng = np.random.default_rng(seed)
    spec = [((9, "walk"), [np.arange(10, 60), np.arange(14, 60), np.arange(10, 51), np.concatenate([np.arange(10, 30), np.arange(34, 60)])]),
            ((9, "sit 1"), [np.arange(0, 30), np.arange(5, 25)]), ((11, "walk"), [np.arange(0, 12)])]
    seq_keys, frame_idx, gts, preds = [], [], [], []
    for ti, ((subject, action), cams) in enumerate(spec):
        world = world_motion(80, joints, rng)
        err = world_motion(80, joints, rng, common)
        for ci, frames in enumerate(cams):
            r, t = camera(rng)
            at = frames + 1 if shifted == (ti, ci) else frames
            gt = (world[at] @ r.T + t).astype(np.float32)
            pred = (gt.astype(np.float64) + err[at] @ r.T + noise * rng.standard_normal((len(frames), joints, 3))).astype(np.float32)
            seq_keys.append((subject, action, str(ci + 1)))
            frame_idx.append(frames)
            gts.append(gt)
            preds.append(pred)
    order = sorted(range(len(seq_keys)), key=lambda s: seq_keys[s])                # evaluate_dense sorts the sequence keys
    seq_keys = [seq_keys[s] for s in order]
    lens = [len(frame_idx[s]) for s in order]
    from implementation_phd_lab_vision_amd import protocols
    return {"seq_keys": seq_keys, "seq_start": np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
            "frame_idx": np.concatenate([frame_idx[s] for s in order]).astype(np.int32), "pred": np.concatenate([preds[s] for s in order]),
            "gt": np.concatenate([gts[s] for s in order]), "group_names": sorted({protocols.action_name(k[1]) for k in seq_keys})}


def dense_metrics(dense):
    """The single-view ``p1 / p2 / mpjve / accel`` entries ``multiview_lines`` prints beside the fused ones, from the restatements."""
    from implementation_phd_lab_vision_amd import protocols, sequences
    from tests import protocols_reference as pr
    from tests import stitch_reference as sr
    names = dense["group_names"]
    seq = np.repeat(np.arange(len(dense["seq_keys"])), np.diff(dense["seq_start"]))
    group = np.array([names.index(protocols.action_name(k[1])) for k in dense["seq_keys"]])[seq]
    f = dense["pred"].shape[0]
    sums = sr.metrics(dense["pred"], dense["gt"], np.zeros(f), np.arange(f + 1), seq, dense["frame_idx"], group, len(names))
    p2 = np.zeros(len(names))
    for r in range(f):
        p2[group[r]] += pr.p2_pose(dense["pred"][r], dense["gt"][r])
    return sequences.metric_values(sums, p2)


def make_multiview_cache(root, seed: int = 0) -> Path:
    """index.pt + shards under ``root``: the clips of VIDEOS for S9 (joints3d in millimetres, as the shards hold them), plus 2 clips of
    S1 (filtered out by the test set)."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    packer = ShardPacker(root, n_vars=1, shard_size=4, shuffle_pool=5, shuffle_seed=seed)
    worlds = {}
    groups = []
    for (action, cam), n in VIDEOS.items():
        if action not in worlds:
            worlds[action] = world_motion(24, 17, rng, 300.0)
        r, t = camera(rng, 5000.0)
        pose = torch.from_numpy((worlds[action][:n] @ r.T + t).astype(np.float32))
        for start in range(0, n - SEQ_LEN + 1, STRIDE):
            groups.append((pose[start:start + SEQ_LEN], {"subject": 9, "action": action, "cam": cam, "start": start, "end": start + SEQ_LEN,
                                                         "aug": "orig", "box": None}))
    for _ in range(2):
        groups.append((torch.randn(SEQ_LEN, 17, 3, generator=g) * 300.0, {"subject": 1, "action": "act0", "cam": 1, "start": 0, "end": SEQ_LEN,
                                                                          "aug": "orig", "box": None}))
    for joints3d, meta in groups:
        k = torch.eye(3)
        k[0, 0], k[1, 1] = 1000.0 + 100.0 * torch.rand(2, generator=g)
        k[0, 2], k[1, 2] = 500.0 + 20.0 * torch.rand(2, generator=g)
        packer.add_group([{"feat": torch.randn(SEQ_LEN, 2048, generator=g).abs(), "joints3d": joints3d.clone(),
                           "joints2d": torch.rand(SEQ_LEN, 17, 2, generator=g) * 1000.0, "K": k, "meta": meta}])
    packer.finish()
    packer.write_index(seq_len=SEQ_LEN, frame_skip=FRAME_SKIP, save_fp16=False, augment=False)
    return Path(root)


def make_preprocessed_tree(root) -> Path:
    """``S9/<action>/cam_<k>/a.mp4`` placeholders for the dumped batch's videos."""
    for action, cam in VIDEOS:
        d = Path(root) / "S9" / action / f"cam_{cam}"
        d.mkdir(parents=True, exist_ok=True)
        (d / "a.mp4").write_bytes(b"")
    return Path(root)


def read_video(path) -> torch.Tensor:
    """(N, 40, 56, 3) uint8 frames of a placeholder video (``--video-reader tests.multiview_data:read_video``)."""
    parts = Path(path).parts[-4:]
    n = VIDEOS[(parts[1], int(parts[2][len("cam_"):]))]
    g = torch.Generator().manual_seed(n + len(parts[1]))
    return torch.randint(0, 256, (FRAME_SKIP * n, 40, 56, 3), dtype=torch.uint8, generator=g)
