"""A small synthetic feature cache for the geometric-loss driver tests, in the on-disk layout of
tests/train_driver_data.py.  That one has ``K = I`` and random ``joints2d``, which no projection explains; here every clip carries
camera-frame poses at 4-5 m (stored in mm, as the preprocessor writes them), an H3.6M-like ``K`` of its own and ``joints2d`` = the
projection of its poses plus a pixel of noise.  Subjects 1, 5, 6, 7, 8 and 11 as tests/train_driver_data.py writes them; subject 9
(the results CLI's test subject) with tests/results_data.py's metas, so its placeholder videos and reader serve."""
from pathlib import Path

import torch

from implementation_phd_lab_vision_amd.shards import AUG_NAMES, ShardPacker
from tests import results_data as rd
from tests.golden.make_golden_geo import intrinsics, poses, project64

SUBJECTS = (1, 5, 6, 7, 8, 9, 11)


def make_geo_feature_cache(root, n_vars: int = 1, seq_len: int = rd.SEQ_LEN, clips_per_subject: int = 4, val_clips: int = 10,
                           shard_size: int = 4, seed: int = 0) -> Path:
    g = torch.Generator().manual_seed(seed)
    packer = ShardPacker(root, n_vars=n_vars, shard_size=shard_size, shuffle_pool=6, shuffle_seed=seed)
    for subject in SUBJECTS:
        n = rd.N_S9 if subject == 9 else val_clips if subject == 5 else clips_per_subject
        for c in range(n):
            base = poses(1, seq_len, g)[0]                                         # (T,17,3) metres
            k = intrinsics(1, g)[0]
            j2d = (project64(base[None], k[None])[0] + torch.randn(seq_len, 17, 2, generator=g).double()).float()
            group = []
            for v in range(n_vars):
                meta = rd.clip_meta(c) if subject == 9 else \
                    {"subject": subject, "action": f"act{c % 3}", "cam": c % 4, "start": 10 * c, "end": 10 * c + seq_len}
                meta = dict(meta, aug=AUG_NAMES[v] if n_vars > 1 else "orig")
                group.append({"feat": torch.randn(seq_len, 2048, generator=g).abs(), "joints3d": base * 1000.0, "joints2d": j2d, "K": k,
                              "meta": meta})
            packer.add_group(group)
    packer.finish()
    packer.write_index(seq_len=seq_len, frame_skip=rd.FRAME_SKIP, save_fp16=False, augment=n_vars > 1)
    return Path(root)
