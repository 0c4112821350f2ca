"""Step time of the rollout objective (``ARTrainableHead.rollout_train_step``) against phase 2's teacher
step, timed the same way in one process: PHD(1024, 17, 2), fp16, eager launches, dropout on, AdamW + GradScaler, clips of I + P
frames.  For each batch size and k, the two steps are timed in alternating rounds (a warmed, synchronised host clock over --steps
steps each) so that drift on a shared host hits both.  GEMM GFLOP per step are counted from shapes: the forward's GEMMs (input_proj
and f_movie over the observed and the full clip, f_AR over the growing sequence at every step with the last conv2 over B rows, the
regressor over the k*B predicted rows) and, for the trained parts, twice that again (dX and dW; the regressor: dX only).  Prints one
JSON line.
    python scripts/bench_rollout_train.py [--batches 32 256] [--ks 1 5 25] [--steps 5] [--rounds 2]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, BLOCKS, AR_BLOCKS, HIDDEN, DP, OP = 1024, 2, 3, 1024, 1088, 64


def gemm_gflop(b: int, i_len: int, k: int, t: int) -> float:
    """GEMM GFLOP of one rollout step (2 * M * N * K per product)."""
    conv = 2 * 3 * D * D                                                    # per row of one causal conv
    fwd = 2 * 2048 * D * b * (i_len + t) + BLOCKS * 2 * conv * b * (i_len + t)        # input_proj + f_movie, observed + teacher
    ar_fwd = ar_bwd = 0
    for j in range(k):
        rows = (i_len + j) * b
        f = AR_BLOCKS * 2 * conv * rows - conv * (rows - b)               # the last conv2 runs over B rows
        ar_fwd += f
        ar_bwd += 2 * f
    reg = 3 * 2 * k * b * (DP * HIDDEN + HIDDEN * HIDDEN + HIDDEN * OP)
    return (fwd + ar_fwd + ar_bwd + 2 * reg) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 5, 25])
    ap.add_argument("--input-len", type=int, default=15)
    ap.add_argument("--pred-len", type=int, default=25)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--precision", default="fp16")
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import train, train_ar
    dev = "cuda:0"
    t = a.input_len + a.pred_len
    sd = train.default_state_dict(D, 17, BLOCKS, seed=0)
    h = train_ar.ARTrainableHead(D, 17, BLOCKS, precision=a.precision)
    h.load_state_dict(sd); h.to(dev).train()
    optim, scaler = train.AdamW(h, lr=1e-4), train.GradScaler(init_scale=1024.0)
    results = []
    for b in a.batches:
        g = torch.Generator().manual_seed(100 + b)
        feats = torch.randn(b, t, 2048, generator=g).abs().to(dev)
        gt = (torch.randn(b, t, 17, 3, generator=g) * 0.5).to(dev)
        steps = {"teacher": lambda: h.train_step(feats, gt, optim, scaler)}
        for k in a.ks:
            steps[f"rollout_k{k}"] = (lambda k=k: h.rollout_train_step(feats, gt, a.input_len, k, optim, scaler))
        for fn in steps.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in steps}
        skipped = {name: 0 for name in steps}
        for _ in range(a.rounds):
            for name, fn in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    skipped[name] += fn()[2]
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        row = {"batch": b, "ms_per_step": ms, "skipped": skipped, "gflop": {}, "tflops": {},
               "max_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}
        for k in a.ks:
            gf = gemm_gflop(b, a.input_len, k, t)
            row["gflop"][f"rollout_k{k}"] = round(gf, 1)
            row["tflops"][f"rollout_k{k}"] = round(gf / min(ms[f"rollout_k{k}"]), 2)
        results.append(row)
        torch.cuda.reset_peak_memory_stats(dev)
    print(json.dumps({"latent_dim": D, "blocks": BLOCKS, "precision": a.precision, "input_len": a.input_len, "clip_len": t, "eager": True,
                      "steps_per_round": a.steps, "results": results, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
