"""Golden items of the training-side reader: what the REFERENCE's ``Human36MFeatureClips`` (src/dataset_features.py,
imported from /root/reference; it needs torch only) returns for the golden shard directories ``ref_plain`` / ``ref_aug``
under several constructor configurations.  The file holds the configurations and the returned items only.

``reader_golden_digest.pt`` holds the same for EXTRA_CONFIGS, with every tensor of more than 1024 elements (the features) kept as
its sha256 digest, dtype and shape, so that the file stays small.

It also writes ``reader_roundtrip_golden.pt``: what the reference's ``Human36MFeatureClips`` and ``MixedShardBatchSampler``
(src/samplers.py) return when they read the cache that tests/test_reader_roundtrip_cpu.py has our CLI write (per ``augment``:
item count, the (clip record, variant) list, every item with its features as a sha256 digest, the subject-filtered list and the
sampler's batches).

    python tests/golden/make_golden_reader.py        # run in the build container (needs /root/reference)
"""
import hashlib
import importlib.util
import os
import sys
import tempfile
from pathlib import Path

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.environ.get("H36M_REFERENCE_SRC", "/root/reference/src")

CONFIGS = [("ref_plain", {"test_set": True}), ("ref_plain", {"max_clips": 3}), ("ref_aug", {"augment": True}),
           ("ref_aug", {"augment": True, "subjects": [9, 11]})]
# the remaining configurations of tests/test_feature_store_cpu.py::test_store_items_equal_reference_reader
EXTRA_CONFIGS = [("ref_plain", {}), ("ref_plain", {"subjects": [1, 5]}), ("ref_aug", {"augment": False, "test_set": True})]
DIGEST_ABOVE = 1024            # reader_golden_digest.pt: tensors with more elements are kept as digest, dtype and shape


def feats_digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().float().numpy().tobytes()).hexdigest()


def digested(v):
    if isinstance(v, torch.Tensor):
        if v.numel() > DIGEST_ABOVE:
            return {"sha256": feats_digest(v), "dtype": str(v.dtype), "shape": list(v.shape)}
        return v.clone()
    return v


def roundtrip():
    """The reference's reader and sampler on the cache of tests/test_reader_roundtrip_cpu.py (written by our CLI)."""
    root = Path(HERE).parents[1]
    sys.path.insert(0, str(root))
    sys.path.insert(0, REF_SRC)
    sys.dont_write_bytecode = True
    from dataset_features import Human36MFeatureClips
    from samplers import MixedShardBatchSampler
    from tests.test_reader_roundtrip_cpu import _make
    out = {}
    for augment in (False, True):
        with tempfile.TemporaryDirectory() as d:
            _make(Path(d), augment)
            reader = Human36MFeatureClips(d, subjects=None, test_set=True, augment=augment, shard_cache_size=1)
            items = []
            for i in range(len(reader)):
                feats, j3d, j2d, k, meta = reader[i]
                items.append({"feats_sha256": feats_digest(feats), "feats_dtype": str(feats.dtype), "feats_shape": list(feats.shape),
                              "j3d": j3d.clone(), "j2d": j2d.clone(), "k": k.clone(), "meta": meta})
            sub = Human36MFeatureClips(d, subjects=[9, 11], augment=augment)
            batches = list(MixedShardBatchSampler(reader, batch_size=4, shards_per_batch=2, drop_last=False, seed=0))
            out[augment] = {"len": len(reader), "index": [(dict(c), v) for c, v in reader._items], "items": items,
                            "sub_index": [(dict(c), v) for c, v in sub._items], "batches": [list(b) for b in batches]}
        print("roundtrip augment", augment, "->", out[augment]["len"], "items,", len(out[augment]["batches"]), "batches")
    torch.save(out, os.path.join(HERE, "reader_roundtrip_golden.pt"))


def main():
    spec = importlib.util.spec_from_file_location("ref_dataset_features", os.path.join(REF_SRC, "dataset_features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = []
    for name, kw in CONFIGS:
        try:
            ds = mod.Human36MFeatureClips(os.path.join(HERE, name), **kw)
            items = [tuple(ds[i]) for i in range(len(ds))]
        except RuntimeError as e:
            items = None
        out.append({"dir": name, "kwargs": kw, "items": items})
        print(name, kw, "->", "error" if items is None else len(items), "items")
    torch.save(out, os.path.join(HERE, "reader_golden.pt"))
    extra = []
    for name, kw in EXTRA_CONFIGS:
        try:
            ds = mod.Human36MFeatureClips(os.path.join(HERE, name), **kw)
            items = [tuple(digested(v) for v in ds[i]) for i in range(len(ds))]
        except RuntimeError:
            items = None
        extra.append({"dir": name, "kwargs": kw, "items": items})
        print(name, kw, "->", "error" if items is None else len(items), "items (digests)")
    torch.save(extra, os.path.join(HERE, "reader_golden_digest.pt"))
    roundtrip()


if __name__ == "__main__":
    main()
