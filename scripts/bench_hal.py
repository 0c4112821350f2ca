"""The hallucinator's pieces, timed in one process on one MI355X.  Prints one JSON line:

* ``op``: ``r50_op_hal_latent_grad`` beside the torch composition it replaces,
  ``(dh_reg + coef * (h.float() - phi.float())).to(dt)`` + ``(h.float() - phi.float()).pow(2).mean()``, at 1280 x 1024 and 10240 x 1024
  (B 32 and B 256 x 40 frames, D 1024, fp16): microseconds per call, and the op's bytes (rows * d * 10: h, phi and dh 2 bytes each, dh_reg
  4) over its time beside the device-copy rate DESIGN.md quotes for the bench box (``scripts/hbm_copy_probe.py``);
* ``step``: ``HalTrainableHead.train_step`` beside phase 2's teacher step (``ARTrainableHead.train_step``) at B 32 and B 256 x 40,
  PHD(1024, 17, 2), fp16, eager launches, AdamW + GradScaler, alternating rounds;
* ``rollout``: ``hallucinated_rollout(feats, 14, 25)`` beside ``rollout(feats, 15, 25)`` at B 32 and B 256.

Device events around the op's launches (they are two kernels on one stream); a warmed, synchronised host clock around steps and rollouts.
    python scripts/bench_hal.py [--iters 2000] [--steps 30] [--rounds 2]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEVICE_COPY_TBS = (5.14, 5.42)      # torch device copy of 1 GB / 256 MB on the bench box, read + write


def _events_us(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _host_ms(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def bench_op(rows, d, iters, dev):
    from implementation_phd_lab_vision_amd import _lib
    lib = _lib.load_library()
    g = torch.Generator().manual_seed(rows)
    dt = torch.float16
    h, phi = torch.randn(rows, d, generator=g).to(dt).to(dev), torch.randn(rows, d, generator=g).to(dt).to(dev)
    lam, ls = 1.0, 1024.0
    coef = lam * 2.0 / (rows * d) * ls
    dh_reg = (torch.randn(rows, d, generator=g) * coef).to(dev)
    dh, loss, part = torch.empty_like(h), torch.empty(1, device=dev), torch.empty(rows, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def op():
        _lib.check(lib.r50_op_hal_latent_grad(h.data_ptr(), phi.data_ptr(), dh_reg.data_ptr(), rows, d, lam, ls, dh.data_ptr(),
                                              loss.data_ptr(), part.data_ptr(), 1, stream), None, "r50_op_hal_latent_grad")

    def composed():
        diff = h.float() - phi.float()
        return (dh_reg + coef * diff).to(dt), diff.pow(2).mean()

    op()
    ref_dh, ref_loss = composed()
    torch.cuda.synchronize()
    close = bool(torch.allclose(dh.float(), ref_dh.float(), rtol=2 ** -9, atol=2 ** -23)) and abs(float(loss) / float(ref_loss) - 1) < 1e-5
    us_op, us_torch = _events_us(op, iters), _events_us(composed, iters)
    nbytes = rows * d * 10
    return {"rows": rows, "d": d, "op_us": us_op, "torch_us": us_torch, "speedup": us_torch / us_op, "bytes": nbytes,
            "op_tb_per_s": nbytes / (us_op * 1e-6) / 1e12, "device_copy_tb_per_s": list(DEVICE_COPY_TBS), "agrees_with_torch": close}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hal: needs an MI355X; there is no CPU fallback and no CPU timing")
    from implementation_phd_lab_vision_amd import train, train_ar, train_hal
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "precision": "fp16", "latent_dim": 1024, "seq_len": a.seq_len,
           "op": [bench_op(rows, 1024, a.iters, dev) for rows in (1280, 10240)]}

    sd = {**train.default_state_dict(1024, 17, 2, seed=0), **train_hal.fresh_hallucinator_state(1024, 0)}
    heads = {}
    for name, cls in (("hal", train_hal.HalTrainableHead), ("phase2_teacher", train_ar.ARTrainableHead)):
        h = cls(1024, 17, 2, hallucinator=True)
        h.load_state_dict(sd)
        h.to(dev).train()
        heads[name] = (h, train.AdamW(h, lr=1e-4), train.GradScaler(init_scale=1024.0))
    out["step"] = []
    for batch in (32, 256):
        g = torch.Generator().manual_seed(100 + batch)
        feats = torch.randn(batch, a.seq_len, 2048, generator=g).abs().to(dev)
        gt = (torch.randn(batch, a.seq_len, 17, 3, generator=g) * 0.5).to(dev)
        ms = {k: [] for k in heads}
        for r in range(a.rounds):
            for name, (h, optim, scaler) in heads.items():
                ms[name].append(_host_ms(lambda: h.train_step(feats, gt, optim, scaler), a.steps, a.warmup if r == 0 else 1))
        out["step"].append({"batch": batch, "steps_per_round": a.steps, "ms_per_step": ms})

    head = PHDFor3DJoints(1024, 17, 2, hallucinator=True)
    head.load_state_dict(sd)
    head.to(dev).eval()
    out["rollout"] = []
    for batch in (32, 256):
        feats = torch.randn(batch, a.seq_len, 2048, generator=torch.Generator().manual_seed(200 + batch)).abs().to(dev)
        ms = {"hallucinated_rollout_f14_p25": [], "rollout_i15_p25": []}
        for r in range(a.rounds):
            ms["hallucinated_rollout_f14_p25"].append(_host_ms(lambda: head.hallucinated_rollout(feats, 14, 25), 5, 2 if r == 0 else 1))
            ms["rollout_i15_p25"].append(_host_ms(lambda: head.rollout(feats, 15, 25), 5, 2 if r == 0 else 1))
        out["rollout"].append({"batch": batch, "calls_per_round": 5, "ms_per_call": ms})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
