"""Golden batches of the REFERENCE's ``MixedShardBatchSampler`` (src/samplers.py, imported from /root/reference; torch only) for the
training driver's tests (tests/test_train_driver_cpu.py).  The sampler only reads ``dataset._items`` (its ``clip["shard_id"]``) and
``len(dataset)``, so each layout is recorded as the shard id of every item, in item order: the layouts of the synthetic caches of
tests/train_driver_data.py (n_variants 4 and 1, training subjects) and a ragged hand-made one.  Per case: layout, batch_size,
shards_per_batch, shuffle, drop_last, seed / epoch, the batches and ``len()``.

The file also records two facts of the reference's src/train.py that the driver restates:
``trainable``: ``[n for n, p in model.named_parameters() if p.requires_grad]`` of ``PHDFor3DJoints(1024, 17, 2)`` with f_AR frozen
(:370-388; ``torchvision``, unused by the head, replaced by an empty stub) -- the numbering of torch.optim.AdamW's state;
``parser_defaults``: the defaults of main()'s argument parser (:283-299, with src/config.py), captured by stopping at parse_args.

    python tests/golden/make_golden_sampler.py        # run in the build container (needs /root/reference)
"""
import argparse
import itertools
import os
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = os.environ.get("H36M_REFERENCE_SRC", "/root/reference/src")


class Items:
    """Stand-in dataset: ``_items`` of (clip record, variant) with the given shard ids."""

    def __init__(self, shard_ids):
        self._items = [({"shard_id": int(s)}, 0) for s in shard_ids]

    def __len__(self):
        return len(self._items)


CONFIGS = [(8, 4), (6, 2), (4, 1)]             # (batch_size, shards_per_batch)
EPOCHS = [0, 1, 2, 5]


def layouts():
    sys.path.insert(0, ROOT)
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from tests.train_driver_data import make_feature_cache
    out = []
    for n_vars in (4, 1):
        with tempfile.TemporaryDirectory() as d:
            make_feature_cache(d, n_vars)
            store = DeviceFeatureStore(d, subjects=[1, 6, 7, 8], augment=True, device="cpu")
            out.append([c["shard_id"] for c, _ in store._items])
    out.append([3] * 5 + [0] * 2 + [7] * 9 + [1] * 1 + [3] * 2 + [2] * 6 + [5] * 3)     # ragged, a shard split in two runs
    return out


def sampler_cases(Sampler, lays):
    cases = []
    for li, lay in enumerate(lays):
        for (bs, k), shuffle, drop_last in itertools.product(CONFIGS, (True, False), (True, False)):
            for epoch in EPOCHS:
                s = Sampler(Items(lay), batch_size=bs, shards_per_batch=k, shuffle=shuffle, drop_last=drop_last, seed=0)
                s.set_epoch(epoch)
                cases.append({"layout": li, "batch_size": bs, "shards_per_batch": k, "shuffle": shuffle, "drop_last": drop_last,
                              "epoch": epoch, "seed": None, "batches": [list(b) for b in s], "len": len(s)})
            s = Sampler(Items(lay), batch_size=bs, shards_per_batch=k, shuffle=shuffle, drop_last=drop_last, seed=7)
            cases.append({"layout": li, "batch_size": bs, "shards_per_batch": k, "shuffle": shuffle, "drop_last": drop_last,
                          "epoch": None, "seed": 7, "batches": [list(b) for b in s], "len": len(s)})
    return cases


def reference_trainable():
    tv = types.ModuleType("torchvision"); tv.models = types.ModuleType("torchvision.models")
    sys.modules.setdefault("torchvision", tv); sys.modules.setdefault("torchvision.models", tv.models)
    import model as ref_model
    m = ref_model.PHDFor3DJoints(latent_dim=1024, joints_num=17, number_blocks=2)
    for p in m.f_AR.parameters():
        p.requires_grad = False
    return [n for n, p in m.named_parameters() if p.requires_grad]


def reference_parser_defaults():
    import train as ref_train
    captured = {}

    def stop(self, args=None, namespace=None):
        captured["defaults"] = vars(argparse.ArgumentParser.parse_known_args(self, [])[0])
        raise SystemExit(0)

    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = stop
    try:
        ref_train.main()
    except SystemExit:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    return captured["defaults"]


def main():
    sys.path.insert(0, REF_SRC)
    sys.dont_write_bytecode = True
    from samplers import MixedShardBatchSampler
    lays = layouts()
    cases = sampler_cases(MixedShardBatchSampler, lays)
    out = {"layouts": lays, "cases": cases, "trainable": reference_trainable(), "parser_defaults": reference_parser_defaults()}
    torch.save(out, os.path.join(HERE, "sampler_golden.pt"))
    print(len(lays), "layouts,", len(cases), "cases,", len(out["trainable"]), "trainable parameters; defaults", out["parser_defaults"])


if __name__ == "__main__":
    main()
