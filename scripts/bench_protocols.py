"""The H3.6M evaluation protocols on one MI355X.  Three numbers, in one process:

* ``r50_op_pose_protocols`` alone at B 256 x P 40 x J 17 (reconstruction: every frame of a 40-frame clip, i0 0) and B 256 x P 25
  (forecast: i0 15), 15 groups (the H3.6M actions): a warmed host clock over --iters launches that ends in a synchronise;
* one ``protocols.evaluate_protocols`` pass over a synthetic store of --clips clips resident on the device, PHD(1024, 17, 2) fp16, with
  and without the I 15 / P 25 rollout (host clock, synchronised, best of --passes after one warm-up pass);
* for scale, a host numpy restatement of the op over the same poses (batched ``np.linalg.svd`` in fp64, the equations of section L),
  with the largest relative difference of its sums from the kernel's.
Prints one JSON line.
    python scripts/bench_protocols.py [--iters 200] [--clips 1024] [--passes 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS = 15


class SyntheticStore:
    """The part of ``DeviceFeatureStore`` that ``evaluate_protocols`` reads: ``feats`` (N, T, 2048), ``len``, ``get_batch``."""

    def __init__(self, n, t, dev, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.feats = torch.randn(n, t, 2048, generator=g).abs().to(dev)
        self.joints3d = poses(n, t, seed + 1).to(dev)

    def __len__(self):
        return self.feats.shape[0]

    def get_batch(self, idx):
        i = torch.as_tensor(idx, dtype=torch.long, device=self.feats.device)
        return self.feats.index_select(0, i), self.joints3d.index_select(0, i)


def poses(b, t, seed, j=17):
    """(B, T, J, 3) fp32: a person a few metres from the camera, joints spread ~0.3 m."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.randn(b, 1, 1, 3, generator=g) * torch.tensor([1.0, 0.5, 0.5]) + torch.tensor([0.0, 0.0, 4.5])
    return (centre + torch.randn(b, 1, j, 3, generator=g) * 0.3 + torch.randn(b, t, j, 3, generator=g) * 0.02).float()


def numpy_sums(pred, gt, i0, group, n_groups, root=0):
    """The op's accumulator on the host: P1 / P2 per pose in fp64 (an SVD per pose, batched), summed per (group, frame)."""
    b, p, j, _ = pred.shape
    y = pred.astype(np.float64).reshape(b * p, j, 3)
    x = gt[:, i0:i0 + p].astype(np.float64).reshape(b * p, j, 3)
    p1 = np.linalg.norm((y - y[:, root:root + 1]) - (x - x[:, root:root + 1]), axis=-1).mean(axis=1)
    y0, x0 = y - y.mean(axis=1, keepdims=True), x - x.mean(axis=1, keepdims=True)
    u, d, vt = np.linalg.svd(np.einsum("nja,njb->nab", x0, y0))
    s = np.ones((b * p, 3))
    s[:, 2] = np.sign(np.linalg.det(u) * np.linalg.det(vt))
    r = np.einsum("nab,nb,nbc->nac", u, s, vt)
    sy, sx = (y0 ** 2).sum(axis=(1, 2)), (x0 ** 2).sum(axis=(1, 2))
    a = np.where((sy > 0) & (sx > 0), (d * s).sum(axis=1) / np.where(sy > 0, sy, 1.0), 0.0)
    y_hat = a[:, None, None] * np.einsum("nac,njc->nja", r, y0) + x.mean(axis=1, keepdims=True)
    p2 = np.linalg.norm(y_hat - x, axis=-1).mean(axis=1)
    acc = np.zeros(2 * n_groups * p + n_groups)
    per = np.stack([p1, p2], axis=-1).reshape(b, p, 2)
    for g in range(n_groups):
        acc[:2 * n_groups * p].reshape(n_groups, p, 2)[g] = per[group == g].sum(axis=0)
        acc[2 * n_groups * p + g] = float((group == g).sum())
    return acc


def time_op(b, t, i0, p, iters, warmup):
    from implementation_phd_lab_vision_amd import protocols
    dev = "cuda:0"
    gt = poses(b, t, seed=b + p)
    pred = (gt[:, i0:i0 + p] + torch.randn(b, p, 17, 3, generator=torch.Generator().manual_seed(p)) * 0.05).contiguous()
    group = (torch.arange(b) % GROUPS).to(torch.int32)
    pd, gd, grp = pred.to(dev), gt.to(dev), group.to(dev)
    acc = torch.zeros(2 * GROUPS * p + GROUPS, dtype=torch.float64, device=dev)
    protocols.add_protocol_sums(pd, gd, i0, grp, GROUPS, acc)
    got = acc.cpu().numpy()
    for _ in range(warmup):
        protocols._launch(pd, gd, i0, grp, GROUPS, acc, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        protocols._launch(pd, gd, i0, grp, GROUPS, acc, 0)
    torch.cuda.synchronize()
    op_us = (time.perf_counter() - t0) * 1e6 / iters
    t0 = time.perf_counter()
    want = numpy_sums(pred.numpy(), gt.numpy(), i0, group.numpy(), GROUPS)
    host_ms = (time.perf_counter() - t0) * 1e3
    rel = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-30)))
    return {"b": b, "p": p, "i0": i0, "joints": 17, "groups": GROUPS, "poses": b * p, "op_us": round(op_us, 2),
            "host_numpy_ms": round(host_ms, 2), "max_rel_diff_vs_numpy": rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import protocols, train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters,
           "op": [time_op(256, 40, 0, 40, a.iters, a.warmup), time_op(256, 40, 15, 25, a.iters, a.warmup)]}
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, 17, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(d, 17, nb, seed=0))
    head.to(dev).eval()
    store = SyntheticStore(a.clips, 40, dev)
    ids = [i % GROUPS for i in range(a.clips)]
    names = [f"action{g:02d}" for g in range(GROUPS)]
    passes = {}
    for name, (i_len, p_len) in (("recon", (0, 0)), ("recon_and_rollout", (15, 25))):
        protocols.evaluate_protocols(head, store, ids, names, i_len, p_len)
        ms = []
        for _ in range(a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = protocols.evaluate_protocols(head, store, ids, names, i_len, p_len)
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        passes[name] = {"ms_per_pass": ms, "recon_all_mm": [round(float(v) * 1e3, 3) for v in res["recon_all"]]}
    out["evaluate_protocols"] = {"clips": a.clips, "batch_size": 256, "latent_dim": d, "precision": "fp16", **passes}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
