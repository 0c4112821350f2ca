"""Autoregressive rollout against the naive program, timed the same way in one process: PHD(1024, 17, 2),
fp16, observe 15 frames, predict 25, at batch 32 and 256.  The new path is ``PHDFor3DJoints.rollout`` (one time-major buffer, the
last block's conv2 over the new frame's rows only, its GEMM's store is the append); the naive path reruns the existing batch-major
``_temporal_net`` over a ``torch.cat``-grown sequence every step.  A warmed, synchronised host clock over --iters rollouts per path;
the paths alternate round by round so that drift on a shared host hits both.  GFLOP per rollout are counted from the GEMM shapes
(f_AR's share separately); TFLOP/s = that over the measured time.  Prints one JSON line.
    python scripts/bench_rollout.py [--iters 20] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gemm_gflop(b, i_len, p_len, d, nb, out_dim, dp, op, naive):
    """GEMM work of one rollout from shapes: 2 * rows * K * N per launch."""
    conv = 2.0 * 3 * d * d                                          # per row of a causal conv (K = 3D, N = D)
    fixed = b * i_len * 2.0 * 2048 * d + nb * 2 * b * i_len * conv  # input_proj + f_movie
    fixed += 3 * b * p_len * 2.0 * (dp * 1024 + 1024 * 1024 + 1024 * op)   # regressor on the P future strips
    ar = 0.0
    for k in range(p_len):
        rows = (i_len + k) * b
        ar += (6 * rows if naive else 5 * rows + b) * conv
    return (fixed + ar) / 1e9, ar / 1e9


def naive_rollout(head, feats, i_len, p_len):
    """The program as written: f_AR over the whole batch-major sequence, keep its last strip, torch.cat it on."""
    from implementation_phd_lab_vision_amd import _lib
    from implementation_phd_lab_vision_amd.model import _AR_BLOCKS
    b, d = feats.shape[0], head.latent_dim
    lib = _lib.load_library()
    f = feats[:, :i_len].contiguous()
    x0 = torch.empty((b * i_len, 2048), dtype=head._dtype, device=head._device)
    _lib.check(lib.r50_op_cast_rows(f.data_ptr(), b * i_len, 2048, x0.data_ptr(), 2048, head._et, head._stream()), None, "cast")
    seq = head._temporal_net(head._gemm(x0, "input_proj", relu=False), b, i_len, "f_movie", head.number_blocks).view(b, i_len, d)
    for k in range(p_len):
        n = i_len + k
        ar = head._temporal_net(seq.reshape(b * n, d), b, n, "f_AR", _AR_BLOCKS).view(b, n, d)
        seq = torch.cat([seq, ar[:, -1:]], dim=1)
    future = seq[:, i_len:].contiguous()
    return future.float(), head._regressor(future.view(b * p_len, d), b, p_len)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--input-len", type=int, default=15)
    ap.add_argument("--pred-len", type=int, default=25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="fp16")
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, 17, nb, precision=a.precision)
    head.load_state_dict(train.default_state_dict(d, 17, nb, seed=0))
    head.to(dev).eval()
    out = {"latent_dim": d, "number_blocks": nb, "precision": a.precision, "input_len": a.input_len, "pred_len": a.pred_len,
           "iters_per_round": a.iters, "rounds": a.rounds, "eager": True, "device": torch.cuda.get_device_name(0), "by_batch": {}}
    for b in a.batches:
        feats = torch.randn(b, a.input_len + a.pred_len, 2048, generator=torch.Generator().manual_seed(b)).abs().to(dev)
        paths = {"new": lambda: head.rollout(feats, a.input_len, a.pred_len), "naive": lambda: naive_rollout(head, feats, a.input_len, a.pred_len)}
        new_out, naive_out = paths["new"](), paths["naive"]()
        agree = float((new_out[0] - naive_out[0]).norm() / naive_out[0].norm())
        for fn in paths.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(a.rounds):
            for name, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    fn()
                torch.cuda.synchronize()
                ms[name].append(round((time.perf_counter() - t0) * 1e3 / a.iters, 3))
        row = {"ms_per_rollout": ms, "rel_diff_new_vs_naive": agree}
        for name in paths:
            total, ar = gemm_gflop(b, a.input_len, a.pred_len, d, nb, head.out_dim, head._dp, head._op, naive=(name == "naive"))
            row[name] = {"gemm_gflop": round(total, 2), "f_ar_gemm_gflop": round(ar, 2), "tflops": round(total / min(ms[name]), 2)}
        out["by_batch"][str(b)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
