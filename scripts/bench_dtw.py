"""Forecast error after dynamic time warping on one MI355X.  Three things, in one process:

* ``r50_op_dtw_protocols`` at B 256 and B 32, P = Q = 25, J 17, 15 groups, beside ``r50_op_pose_protocols`` on the same ``pred`` / ``gt``
  in the same run: device events around each call, the median of --iters calls after --warmup.  The plain op does B*P similarity fits,
  the warping one B*P*Q, so the time per fit of each is printed too;
* one ``dtw.evaluate_dtw`` pass beside one ``protocols.evaluate_protocols`` pass (I 15 / P 25) over the same synthetic store of --clips
  clips resident on the device, PHD(1024, 17, 2) fp16 (host clock, synchronised, --passes passes after one warm-up pass);
* for scale, a host numpy DTW (the batched SVD costs of bench_protocols.py, then the DP in Python) on 8 clips, with the largest relative
  difference of its totals from the kernel's.
Prints one JSON line.
    python scripts/bench_dtw.py [--iters 50] [--clips 1024] [--passes 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_protocols import GROUPS, SyntheticStore, poses  # noqa: E402

I_LEN, P_LEN, JOINTS = 15, 25, 17


def slowed(gt, i0, p, seed):
    """(B, P, J, 3) fp32: frames i0 .. i0+p-1 of gt shown at a per-clip speed in [0.6, 1.0] (linear interpolation) plus 0.01-m noise."""
    g = torch.Generator().manual_seed(seed)
    b = gt.shape[0]
    pos = torch.arange(p, dtype=torch.float64)[None] * (0.6 + 0.4 * torch.rand(b, 1, generator=g, dtype=torch.float64))
    lo = pos.floor().clamp(max=p - 2).long()
    w = (pos - lo)[:, :, None, None]
    x = gt[:, i0:i0 + p].double()
    idx = lo[:, :, None, None].expand(-1, -1, x.shape[2], 3)
    y = x.gather(1, idx) * (1 - w) + x.gather(1, idx + 1) * w
    return (y + torch.randn(y.shape, generator=g, dtype=torch.float64) * 0.01).float().contiguous()


def walk(b, t, seed):
    """bench_protocols' poses plus a random walk of 0.03-m steps per joint, so the frame order matters."""
    g = torch.Generator().manual_seed(seed + 77)
    return (poses(b, t, seed) + torch.cumsum(torch.randn(b, t, JOINTS, 3, generator=g) * 0.03, dim=1)).float()


def event_median_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e3)
    return statistics.median(times), min(times), max(times)


def numpy_costs(pred, gt):
    """(2, P, Q) fp64 of one clip: P1 / P2 of every (predicted frame, ground-truth frame) pair, one batched SVD."""
    p, q, j = pred.shape[0], gt.shape[0], pred.shape[1]
    y = np.repeat(pred.astype(np.float64), q, axis=0)
    x = np.tile(gt.astype(np.float64), (p, 1, 1))
    p1 = np.linalg.norm((y - y[:, :1]) - (x - x[:, :1]), axis=-1).mean(axis=1)
    y0, x0 = y - y.mean(axis=1, keepdims=True), x - x.mean(axis=1, keepdims=True)
    u, d, vt = np.linalg.svd(np.einsum("nja,njb->nab", x0, y0))
    s = np.ones((p * q, 3))
    s[:, 2] = np.sign(np.linalg.det(u) * np.linalg.det(vt))
    r = np.einsum("nab,nb,nbc->nac", u, s, vt)
    sy, sx = (y0 ** 2).sum(axis=(1, 2)), (x0 ** 2).sum(axis=(1, 2))
    a = np.where((sy > 0) & (sx > 0), (d * s).sum(axis=1) / np.where(sy > 0, sy, 1.0), 0.0)
    y_hat = a[:, None, None] * np.einsum("nac,njc->nja", r, y0) + x.mean(axis=1, keepdims=True)
    p2 = np.linalg.norm(y_hat - x, axis=-1).mean(axis=1)
    return np.stack([p1, p2]).reshape(2, p, q)


def numpy_total(c):
    """D[P-1][Q-1] of the closed-ended DP over one cost matrix (ties: diagonal, up, left)."""
    p, q = c.shape
    d = np.empty((p, q))
    for i in range(p):
        for j in range(q):
            cands = ([d[i - 1, j - 1]] if i and j else []) + ([d[i - 1, j]] if i else []) + ([d[i, j - 1]] if j else [])
            best = cands[0] if cands else 0.0
            for v in cands[1:]:
                if v < best:
                    best = v
            d[i, j] = c[i, j] + best if cands else c[i, j]
    return d[p - 1, q - 1]


def time_op(b, iters, warmup, host_clips=0):
    from implementation_phd_lab_vision_amd import dtw, protocols
    dev = "cuda:0"
    gt = walk(b, I_LEN + P_LEN, seed=b)
    pred = slowed(gt, I_LEN, P_LEN, seed=b + 1)
    grp = (torch.arange(b) % GROUPS).to(torch.int32).to(dev)
    pd, gd = pred.to(dev), gt.to(dev)
    acc = torch.zeros(dtw.acc_size(GROUPS, P_LEN), dtype=torch.float64, device=dev)
    acc_p = torch.zeros(2 * GROUPS * P_LEN + GROUPS, dtype=torch.float64, device=dev)
    clip_out = dtw.add_dtw_sums(pd, gd, I_LEN, P_LEN, grp, GROUPS, acc)
    rec = clip_out.cpu().numpy()
    d_us = event_median_us(lambda: dtw._launch(pd, gd, I_LEN, P_LEN, grp, GROUPS, acc, -1, 0, clip_out, None), iters, warmup)
    p_us = event_median_us(lambda: protocols._launch(pd, gd, I_LEN, grp, GROUPS, acc_p, 0), iters, warmup)
    out = {"b": b, "p": P_LEN, "q": P_LEN, "joints": JOINTS, "groups": GROUPS,
           "dtw_op_us": {"median": round(d_us[0], 2), "min": round(d_us[1], 2), "max": round(d_us[2], 2)},
           "protocols_op_us": {"median": round(p_us[0], 2), "min": round(p_us[1], 2), "max": round(p_us[2], 2)},
           "dtw_fits": b * P_LEN * P_LEN, "protocols_fits": b * P_LEN,
           "dtw_ns_per_fit": round(d_us[0] * 1e3 / (b * P_LEN * P_LEN), 2), "protocols_ns_per_fit": round(p_us[0] * 1e3 / (b * P_LEN), 2),
           "mean_path_len": round(float(rec[:, :, 1].mean()), 2)}
    if host_clips:
        t0 = time.perf_counter()
        totals = np.array([[numpy_total(c) for c in numpy_costs(pred[i].numpy(), gt[i, I_LEN:].numpy())] for i in range(host_clips)])
        out["host_numpy"] = {"clips": host_clips, "ms": round((time.perf_counter() - t0) * 1e3, 2),
                             "max_rel_diff_of_totals": float(np.max(np.abs(totals - rec[:host_clips, :, 0]) / totals))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be >= 20: the reported time is a median")
    from implementation_phd_lab_vision_amd import dtw, protocols, train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "op": [time_op(256, a.iters, a.warmup, host_clips=8),
                                                                             time_op(32, a.iters, a.warmup)]}
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, JOINTS, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(d, JOINTS, nb, seed=0))
    head.to(dev).eval()
    store = SyntheticStore(a.clips, I_LEN + P_LEN, dev)
    ids = [i % GROUPS for i in range(a.clips)]
    names = [f"action{g:02d}" for g in range(GROUPS)]
    passes = {}
    for name, fn in (("evaluate_dtw", lambda: dtw.evaluate_dtw(head, store, ids, names, I_LEN, P_LEN)),
                     ("evaluate_protocols", lambda: protocols.evaluate_protocols(head, store, ids, names, I_LEN, P_LEN))):
        fn()
        ms = []
        for _ in range(a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        passes[name] = {"ms_per_pass": ms}
        if name == "evaluate_dtw":
            passes[name].update(dtw_all_mm=[round(float(v) * 1e3, 3) for v in res["dtw_all"]],
                                plain_all_mm=[round(float(v) * 1e3, 3) for v in res["plain_all"]])
    out["passes"] = {"clips": a.clips, "batch_size": 256, "input_len": I_LEN, "pred_len": P_LEN, "latent_dim": d, "precision": "fp16", **passes}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
