"""Small synthetic feature caches for the training-driver tests, written with the project's shard packer (shards.py) in the
on-disk layout the reference's reader and the driver read: every subject of H36M, ``clips_per_subject`` clips each (subject 5,
the validation subject, more, so that the validation pass ends on a short batch), ``shard_size`` clips per shard."""
from pathlib import Path

import torch

from implementation_phd_lab_vision_amd.shards import AUG_NAMES, ShardPacker

SUBJECTS = (1, 5, 6, 7, 8, 9, 11)


def make_feature_cache(root, n_vars: int, seq_len: int = 8, clips_per_subject: int = 4, val_clips: int = 10, shard_size: int = 4,
                       seed: int = 0) -> Path:
    """Write index.pt + shard_*.pt under ``root``; features ~ |N(0,1)| (post-ReLU means), joints3d in mm, as the preprocessor writes
    them.  Returns ``root``."""
    g = torch.Generator().manual_seed(seed)
    packer = ShardPacker(root, n_vars=n_vars, shard_size=shard_size, shuffle_pool=6, shuffle_seed=seed)
    for subject in SUBJECTS:
        for c in range(val_clips if subject == 5 else clips_per_subject):
            base = torch.randn(seq_len, 17, 3, generator=g) * 300.0
            group = []
            for v in range(n_vars):
                meta = {"subject": subject, "action": f"act{c % 3}", "cam": c % 4, "start": 10 * c, "end": 10 * c + seq_len,
                        "aug": AUG_NAMES[v] if n_vars > 1 else "orig"}
                group.append({"feat": torch.randn(seq_len, 2048, generator=g).abs(), "joints3d": base + 20.0 * v,
                              "joints2d": torch.rand(seq_len, 17, 2, generator=g) * 1000.0, "K": torch.eye(3), "meta": meta})
            packer.add_group(group)
    packer.finish()
    packer.write_index(seq_len=seq_len, frame_skip=2, save_fp16=False, augment=n_vars > 1)
    return Path(root)
