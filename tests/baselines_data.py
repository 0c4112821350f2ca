"""Fixture of the forecast-baseline tests: a small feature cache written with the project's shard packer, following
tests/results_data.py: its 11 S9 clips (the same metas, so its preprocessed tree and fake video reader serve the CLI runs) and 40 S1
clips as the nearest-neighbour database.  SEQ_LEN 8.  Poses are smooth random walks in mm, so holding the last pose is a sensible
opponent; features are non-negative like pooled ResNet features."""
from pathlib import Path

import torch

from implementation_phd_lab_vision_amd.shards import ShardPacker
from tests.results_data import FRAME_SKIP, N_S9, SEQ_LEN, clip_meta

N_S1 = 40
_ACTIONS = ("act0", "act1", "act2")


def _clip(g: torch.Generator, meta: dict) -> dict:
    k = torch.eye(3)
    k[0, 0], k[1, 1] = 1000.0 + 100.0 * torch.rand(2, generator=g)
    k[0, 2], k[1, 2] = 500.0 + 20.0 * torch.rand(2, generator=g)
    pose0 = torch.randn(1, 17, 3, generator=g) * 300.0
    walk = torch.cumsum(torch.randn(SEQ_LEN, 17, 3, generator=g) * 20.0 + torch.randn(1, 17, 3, generator=g) * 15.0, dim=0)
    return {"feat": torch.randn(SEQ_LEN, 2048, generator=g).abs(), "joints3d": pose0 + walk,
            "joints2d": torch.rand(SEQ_LEN, 17, 2, generator=g) * 1000.0, "K": k, "meta": meta}


def make_baselines_cache(root, n_s9: int = N_S9, n_s1: int = N_S1, seed: int = 0) -> Path:
    """index.pt + shards under ``root``: ``n_s9`` S9 clips (the test set) and ``n_s1`` S1 clips (the database)."""
    g = torch.Generator().manual_seed(seed)
    packer = ShardPacker(root, n_vars=1, shard_size=8, shuffle_pool=5, shuffle_seed=seed)
    metas = [clip_meta(c) for c in range(n_s9)] + \
            [{"subject": 1, "action": _ACTIONS[c % 3], "cam": 1 + c % 2, "start": 4 * (c // 6), "end": 4 * (c // 6) + SEQ_LEN, "aug": "orig",
              "box": None} for c in range(n_s1)]
    for meta in metas:
        packer.add_group([_clip(g, meta)])
    packer.finish()
    packer.write_index(seq_len=SEQ_LEN, frame_skip=FRAME_SKIP, save_fp16=False, augment=False)
    return Path(root)
