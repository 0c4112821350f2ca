"""The joint training step against phase 1's and phase 2's, timed the same way in one process:
PHD(1024, 17, 2), T 40 frames, fp16, eager launches (phase 1's HIP graphs off), dropout on, AdamW + GradScaler, at B 32 and
B 256.  Per batch size the three steps run in alternating rounds so that drift on a shared host hits all of them; each step is
timed on a synchronised host clock (every train_step ends on a device read).  Reports per step kind the median and min ms over
the timed steps and the GEMM GFLOP of one step from the shapes (the GEMMs' padded K / N, as they run), and for each the peak
``torch.cuda.max_memory_allocated`` over one step.  Prints one JSON line.
    python scripts/bench_train_joint.py [--batches 32 256] [--rounds 5] [--steps 10]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gemm_gflop(b: int, t: int, d: int = 1024, nb: int = 2, ar_blocks: int = 3, dp: int = 1088, op: int = 64, hidden: int = 1024):
    """GEMM GFLOP of one step of each kind, from the shapes the launches run (the regressor's K padded to dp, N to op)."""
    rows = b * t
    proj, conv, reg = 2048 * d, 2 * 3 * d * d, 3 * (dp * hidden + hidden * hidden + hidden * op)    # MACs per row
    movie, far = nb * conv, ar_blocks * conv
    phase1 = rows * (proj + movie + reg) + rows * (2 * reg + 2 * movie + proj)         # forward; regressor / f_movie dX + dW, input_proj dW
    phase2 = rows * (proj + movie + far + reg) + rows * (reg + 2 * far)                # forward; regressor dX, f_AR dX + dW
    joint = rows * (proj + movie + far + 2 * reg) + rows * (4 * reg + 2 * far + 2 * movie + proj)
    return {"joint": 2e-9 * joint, "phase1": 2e-9 * phase1, "phase2": 2e-9 * phase2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--seq-len", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per head and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import train, train_ar, train_joint
    dev = "cuda:0"
    sd = train.default_state_dict(1024, 17, 2, seed=0)
    heads = {}
    for name, cls in (("joint", train_joint.JointTrainableHead), ("phase1", train.TrainableHead), ("phase2", train_ar.ARTrainableHead)):
        h = cls(1024, 17, 2, precision=a.precision)
        h.load_state_dict(sd); h.to(dev).train()
        heads[name] = (h, train.AdamW(h, lr=1e-4), train.GradScaler(init_scale=1024.0))
    assert not heads["phase1"][0]._use_graphs
    result = {"workload": f"PHD(1024,17,2) train steps, T {a.seq_len}, {a.precision}, eager, dropout on, AdamW + GradScaler",
              "rounds": a.rounds, "steps_per_round": a.steps, "device": torch.cuda.get_device_name(0), "by_batch": {}}
    for b in a.batches:
        g = torch.Generator().manual_seed(100 + b)
        feats = torch.randn(b, a.seq_len, 2048, generator=g).abs().to(dev)
        gt = (torch.randn(b, a.seq_len, 17, 3, generator=g) * 0.5).to(dev)
        peak = {}
        for name, (h, optim, scaler) in heads.items():
            for _ in range(a.warmup):
                h.train_step(feats, gt, optim, scaler)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            h.train_step(feats, gt, optim, scaler)
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated()
        ms = {k: [] for k in heads}
        skipped = {k: 0 for k in heads}
        for _ in range(a.rounds):
            for name, (h, optim, scaler) in heads.items():
                for _ in range(a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    skipped[name] += h.train_step(feats, gt, optim, scaler)[2]
                    torch.cuda.synchronize()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        flop = gemm_gflop(b, a.seq_len)
        med = {k: float(torch.tensor(v).median()) for k, v in ms.items()}
        result["by_batch"][str(b)] = {
            "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()}, "gemm_gflop": flop,
            "max_memory_allocated_mb": {k: v / 2 ** 20 for k, v in peak.items()}, "skipped": skipped,
            "joint_over_phase1_plus_phase2": med["joint"] / (med["phase1"] + med["phase2"]),
            "gemm_gflop_joint_over_pair": flop["joint"] / (flop["phase1"] + flop["phase2"])}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
