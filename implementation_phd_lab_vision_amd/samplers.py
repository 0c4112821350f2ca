"""Batch order of the reference's phase-1 training (``MixedShardBatchSampler``, src/samplers.py; used at src/train.py:323-329).

Items are bucketed by the shard that holds their clip, so a batch touches few shards, and each batch mixes
``shards_per_batch`` of them.  One epoch, driven by ``random.Random(seed)``:

1. shuffle the shard ids (first-appearance order of ``dataset._items``);
2. shuffle each shard's item list, in that shard order;
3. while at least ``shards_per_batch`` shards have items left: draw that many of them (``rng.sample``; without shuffling, the
   first ones), take up to ``batch_size / shards_per_batch`` items from the front of each, and drop a shard once it is empty.
   A batch that came out short is skipped with ``drop_last`` and yielded otherwise.

Without ``shuffle`` no random number is drawn.  ``set_epoch(e)`` makes ``e`` the seed, as in the reference.  These are the
reference's draws in the reference's order, so the batches are the same for every (seed, epoch, shuffle, drop_last)
(tests/test_train_driver_cpu.py against batches recorded from the reference's class).  It works over anything with the
reference dataset's ``_items`` list of ``(clip record, variant)`` pairs: ``feature_store.DeviceFeatureStore`` has it.
"""
from __future__ import annotations

import random
from typing import Dict, Iterator, List


class MixedShardBatchSampler:
    def __init__(self, dataset, batch_size: int, shards_per_batch: int = 4, shuffle: bool = True, drop_last: bool = True,
                 seed: int = 0):
        if batch_size % shards_per_batch:
            raise ValueError(f"batch_size ({batch_size}) must be a multiple of shards_per_batch ({shards_per_batch})")
        self.dataset = dataset
        self.batch_size = batch_size
        self.K = shards_per_batch
        self.per_shard = batch_size // shards_per_batch
        self.shuffle = shuffle
        self.drop_last = drop_last
        self.seed = seed
        self.buckets: Dict[int, List[int]] = {}
        for i, (clip, _variant) in enumerate(dataset._items):
            self.buckets.setdefault(clip["shard_id"], []).append(i)

    def set_epoch(self, epoch: int) -> None:
        self.seed = epoch

    def __iter__(self) -> Iterator[List[int]]:
        rng = random.Random(self.seed)
        order = list(self.buckets)
        if self.shuffle:
            rng.shuffle(order)
        queues: Dict[int, List[int]] = {}
        for sid in order:
            q = list(self.buckets[sid])
            if self.shuffle:
                rng.shuffle(q)
            queues[sid] = q
        live = [sid for sid in order if queues[sid]]
        while len(live) >= self.K:
            picked = rng.sample(live, self.K) if self.shuffle else live[: self.K]
            batch: List[int] = []
            for sid in picked:
                q = queues[sid]
                batch += q[: self.per_shard]
                del q[: self.per_shard]
                if not q:
                    live.remove(sid)
            if len(batch) == self.batch_size or not self.drop_last:
                yield batch

    def __len__(self) -> int:
        """The reference's estimate (items / batch_size, rounded down with ``drop_last``, up otherwise), not the exact count."""
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size
