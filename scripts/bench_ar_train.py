"""Phase-2 (f_AR) training step against phase 1's, timed the same way in one process: PHD(1024, 17, 2), batch 32 x 40 frames,
fp16, eager launches, dropout on, AdamW + GradScaler.  A warmed, synchronised host clock over --steps steps per head; the two
heads are timed in alternating rounds so that drift on a shared host hits both.  Prints one JSON line.
    python scripts/bench_ar_train.py [--steps 200] [--rounds 2]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq-len", type=int, default=40)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--precision", default="fp16")
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import train, train_ar
    dev = "cuda:0"
    sd = train.default_state_dict(1024, 17, 2, seed=0)
    heads = {}
    for name, cls in (("phase1", train.TrainableHead), ("phase2", train_ar.ARTrainableHead)):
        h = cls(1024, 17, 2, precision=a.precision)
        h.load_state_dict(sd); h.to(dev).train()
        heads[name] = (h, train.AdamW(h, lr=1e-4), train.GradScaler(init_scale=1024.0))
    g = torch.Generator().manual_seed(100)
    feats = torch.randn(a.batch, a.seq_len, 2048, generator=g).abs().to(dev)
    gt = (torch.randn(a.batch, a.seq_len, 17, 3, generator=g) * 0.5).to(dev)
    for h, optim, scaler in heads.values():
        for _ in range(a.warmup):
            h.train_step(feats, gt, optim, scaler)
    torch.cuda.synchronize()
    ms = {k: [] for k in heads}
    skipped = {k: 0 for k in heads}
    for _ in range(a.rounds):
        for name, (h, optim, scaler) in heads.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                skipped[name] += h.train_step(feats, gt, optim, scaler)[2]
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    print(json.dumps({"batch": a.batch, "seq_len": a.seq_len, "latent_dim": 1024, "precision": a.precision, "eager": True,
                      "steps_per_round": a.steps, "ms_per_step": ms, "skipped": skipped,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
