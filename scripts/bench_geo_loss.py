"""The geometric pose loss on the MI355X, T 40, J 17, at B 32 and B 256.  One JSON line:
(a) ``r50_op_geo_pose_loss_grad`` alone (loss + gradient of all four terms; its two launches between a pair of device events),
    median and min over ``--launches`` calls after 3 warm-ups, on random poses at 4-5 m depth with every weight on;
(b) the naive program: the same loss and gradient written with torch ops and autograd on the device, on a (B,T,17,3) fp32 leaf
    (forward, ``autograd.grad``), timed the same way;
(c) phase 1's eager training step with and without ``geo``, and the joint step with and without, PHD(1024, 17, 2), fp16, dropout
    on, AdamW + GradScaler, in alternating rounds in one process, each step on a synchronised host clock (a step ends on a device
    read).  The weights of (c) are small enough that no fp16 step overflows on these inputs.
    python scripts/bench_geo_loss.py [--batches 32 256] [--launches 50] [--rounds 5] [--steps 10]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(b, t, dev, seed):
    """Predictions 5 cm off poses at 4-5 m, an H3.6M-like K per clip, 2D targets = the projected poses plus a pixel of noise."""
    g = torch.Generator().manual_seed(seed)
    root = torch.cat([torch.rand(b, 1, 1, 2, generator=g) - 0.5, 4.0 + torch.rand(b, 1, 1, 1, generator=g)], dim=-1)
    gt = root + 0.25 * torch.randn(b, 1, 17, 3, generator=g) + 0.02 * torch.randn(b, t, 17, 3, generator=g)
    k = torch.zeros(b, 3, 3)
    k[:, 0, 0] = 1145.0 + 4.0 * torch.randn(b, generator=g); k[:, 1, 1] = 1144.0 + 4.0 * torch.randn(b, generator=g)
    k[:, 0, 2] = 112.0 + 3.0 * torch.randn(b, generator=g); k[:, 1, 2] = 112.0 + 3.0 * torch.randn(b, generator=g); k[:, 2, 2] = 1.0
    ph = torch.einsum("bij,btnj->btni", k, gt)
    j2d = ph[..., :2] / ph[..., 2:3] + torch.randn(b, t, 17, 2, generator=g)
    pred = gt + 0.05 * torch.randn(b, t, 17, 3, generator=g)
    return [v.to(dev).contiguous() for v in (pred, gt, j2d, k)]


def naive_loss_grad(pred, gt, j2d, k, ea, eb, lam, eps=1e-6):
    leaf = pred.detach().requires_grad_(True)
    ph = torch.matmul(k[:, None, None], leaf.unsqueeze(-1)).squeeze(-1)
    uv = ph[..., :2] / ph[..., 2:3].clamp(min=eps)
    l3d = (leaf - gt).pow(2).mean()
    l2d = (uv - j2d).pow(2).mean()
    l_vel = ((leaf[:, 1:] - leaf[:, :-1]) - (gt[:, 1:] - gt[:, :-1])).pow(2).mean()
    l_bone = (torch.norm(leaf[:, :, eb] - leaf[:, :, ea], dim=-1) - torch.norm(gt[:, :, eb] - gt[:, :, ea], dim=-1)).pow(2).mean()
    loss = l3d + lam[0] * l2d + lam[1] * l_vel + lam[2] * l_bone
    (grad,) = torch.autograd.grad(loss, leaf)
    return loss, grad


def event_ms(fn, n, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def stats(ms):
    return {"median_ms": float(torch.tensor(ms).median()), "min_ms": min(ms), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--seq-len", type=int, default=40)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.launches < 20:
        ap.error("--launches must be >= 20")
    from implementation_phd_lab_vision_amd import train, train_joint
    dev = "cuda:0"
    geo = train.GeoWeights(1e-6, 1.0, 1.0)
    lam = geo.as_tuple()
    ea = torch.tensor([e[0] for e in train.H36M_EDGES], device=dev)
    eb = torch.tensor([e[1] for e in train.H36M_EDGES], device=dev)
    sd = train.default_state_dict(1024, 17, 2, seed=0)
    y0 = sd["f_3D.y0"].clone().view(-1, 3); y0[:, 2] = 4.5; sd["f_3D.y0"] = y0.view(sd["f_3D.y0"].shape)     # predictions in front of the camera
    heads = {}
    for name, cls in (("phase1", train.TrainableHead), ("joint", train_joint.JointTrainableHead)):
        for variant in ("plain", "geo"):
            h = cls(1024, 17, 2, precision="fp16")
            h.load_state_dict(sd); h.to(dev).train()
            heads[f"{name}_{variant}"] = (h, train.AdamW(h, lr=1e-5), train.GradScaler(init_scale=1024.0), variant == "geo")
    result = {"workload": f"geometric pose loss, T {a.seq_len}, J 17, lambdas {lam}; steps: PHD(1024,17,2), fp16, eager, dropout on",
              "device": torch.cuda.get_device_name(0), "launches": a.launches, "rounds": a.rounds, "steps_per_round": a.steps, "by_batch": {}}
    for b in a.batches:
        pred, gt, j2d, k = inputs(b, a.seq_len, dev, 100 + b)
        dy, out8 = torch.empty_like(pred), torch.empty(8, device=dev)

        def op():
            train.geo_pose_loss_grad(pred, gt, j2d, k, b, a.seq_len, 17, geo, out8, dy=dy)

        def naive():
            return naive_loss_grad(pred, gt, j2d, k, ea, eb, lam)

        op(); loss, grad = naive()
        torch.cuda.synchronize()
        agree = {"loss_rel": abs(float(out8[0]) - float(loss.detach())) / abs(float(loss.detach())),
                 "grad_rel_max": float((dy - grad).abs().max() / grad.abs().max())}
        r_op, r_naive = stats(event_ms(op, a.launches)), stats(event_ms(naive, a.launches))
        feats = torch.randn(b, a.seq_len, 2048, generator=torch.Generator().manual_seed(7 + b)).abs().to(dev)

        def step(key):
            h, optim, scaler, with_geo = heads[key]
            if with_geo:
                return h.train_step(feats, gt, optim, scaler, joints2d=j2d, K=k, geo=geo)
            return h.train_step(feats, gt, optim, scaler)

        for key in heads:
            for _ in range(a.warmup):
                step(key)
        ms, skipped = {key: [] for key in heads}, {key: 0 for key in heads}
        for _ in range(a.rounds):
            for key in heads:
                for _ in range(a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    skipped[key] += step(key)[2]
                    torch.cuda.synchronize()
                    ms[key].append((time.perf_counter() - t0) * 1e3)
        med = {key: float(torch.tensor(v).median()) for key, v in ms.items()}
        result["by_batch"][str(b)] = {
            "op": r_op, "naive_torch": r_naive, "op_over_naive_median": r_op["median_ms"] / r_naive["median_ms"],
            "op_over_naive_min": r_op["min_ms"] / r_naive["min_ms"], "op_vs_naive_agreement": agree,
            "step_median_ms": med, "step_min_ms": {key: min(v) for key, v in ms.items()}, "skipped": skipped,
            "added_ms_phase1": med["phase1_geo"] - med["phase1_plain"], "added_ms_joint": med["joint_geo"] - med["joint_plain"]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
