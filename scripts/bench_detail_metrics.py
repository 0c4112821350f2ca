"""The detail metrics on one MI355X, beside the H3.6M protocols they extend.  In one process:

* ``r50_op_pose_detail_metrics`` and ``r50_op_pose_protocols`` on the SAME inputs at B 256 x P 40 x J 17 (reconstruction, i0 0) and
  B 256 x P 25 (forecast, i0 15), 15 groups, 31 thresholds: the two ops alternate in rounds of --iters launches, each round under a
  warmed host clock that ends in a synchronise; the figure is the best round of each and their ratio;
* one ``detail_metrics.evaluate_detail`` pass beside one ``protocols.evaluate_protocols`` pass over a synthetic store of --clips clips
  resident on the device, PHD(1024, 17, 2) fp16, with the I 15 / P 25 rollout (host clock, synchronised, best of --passes after one
  warm-up pass each, alternating);
* the largest relative difference of the op's sums from a host numpy restatement (batched fp64 SVD), and whether its hit counts
  are equal.
Prints one JSON line.
    python scripts/bench_detail_metrics.py [--iters 200] [--rounds 5] [--clips 1024] [--passes 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_protocols import GROUPS, SyntheticStore, poses  # noqa: E402

N_THR, THR_MAX = 31, 0.150


def numpy_sums(pred, gt, i0, group, n_groups, root=0):
    """The op's accumulator on the host, from the definitions of section O (an SVD per pose, batched)."""
    b, p, j, _ = pred.shape
    y = pred.astype(np.float64)
    x = gt[:, i0:i0 + p].astype(np.float64)
    ry, rx = y - y[:, :, root:root + 1], x - x[:, :, root:root + 1]
    d1 = np.linalg.norm(ry - rx, axis=-1)
    y0, x0 = y - y.mean(axis=2, keepdims=True), x - x.mean(axis=2, keepdims=True)
    u, d, vt = np.linalg.svd(np.einsum("bpja,bpjc->bpac", x0, y0))
    s = np.ones((b, p, 3))
    s[..., 2] = np.sign(np.linalg.det(u) * np.linalg.det(vt))
    r = np.einsum("bpac,bpc,bpcd->bpad", u, s, vt)
    sy, sx = (y0 ** 2).sum(axis=(2, 3)), (x0 ** 2).sum(axis=(2, 3))
    a = np.where((sy > 0) & (sx > 0), (d * s).sum(axis=-1) / np.where(sy > 0, sy, 1.0), 0.0)
    d2 = np.linalg.norm(a[..., None, None] * np.einsum("bpac,bpjc->bpja", r, y0) + x.mean(axis=2, keepdims=True) - x, axis=-1)
    tau = np.float64(THR_MAX) * np.arange(N_THR, dtype=np.float64) / np.float64(N_THR - 1)
    per = np.zeros((b, p, 6))
    for m, dist in ((0, d1), (2, d2)):
        per[..., m] = (dist[..., None] < tau).sum(axis=(2, 3))
        per[..., m + 1] = (dist < THR_MAX).sum(axis=2)
    per[:, 1:, 4] = np.linalg.norm((ry[:, 1:] - ry[:, :-1]) - (rx[:, 1:] - rx[:, :-1]), axis=-1).sum(axis=2)
    per[:, 1:-1, 5] = np.linalg.norm((ry[:, :-2] - 2.0 * ry[:, 1:-1] + ry[:, 2:]) - (rx[:, :-2] - 2.0 * rx[:, 1:-1] + rx[:, 2:]),
                                     axis=-1).sum(axis=2)
    sec_a, sec_b, clips = np.zeros((n_groups, p, j, 2)), np.zeros((n_groups, p, 6)), np.zeros(n_groups)
    for g in range(n_groups):
        sec_a[g] = np.stack([d1[group == g].sum(axis=0), d2[group == g].sum(axis=0)], axis=-1)
        sec_b[g] = per[group == g].sum(axis=0)
        clips[g] = float((group == g).sum())
    return np.concatenate([sec_a.ravel(), sec_b.ravel(), clips])


def time_ops(b, t, i0, p, iters, rounds, warmup):
    from implementation_phd_lab_vision_amd import detail_metrics, protocols
    dev = "cuda:0"
    gt = poses(b, t, seed=b + p)
    pred = (gt[:, i0:i0 + p] + torch.randn(b, p, 17, 3, generator=torch.Generator().manual_seed(p)) * 0.05).contiguous()
    group = (torch.arange(b) % GROUPS).to(torch.int32)
    pd, gd, grp = pred.to(dev), gt.to(dev), group.to(dev)
    acc_d = torch.zeros(detail_metrics.acc_size(GROUPS, p, 17), dtype=torch.float64, device=dev)
    acc_p = torch.zeros(2 * GROUPS * p + GROUPS, dtype=torch.float64, device=dev)
    detail_metrics.add_detail_sums(pd, gd, i0, grp, GROUPS, acc_d, n_thr=N_THR, thr_max=THR_MAX)
    got = acc_d.cpu().numpy()
    launch = {"detail": lambda: detail_metrics._launch(pd, gd, i0, grp, GROUPS, acc_d, 0, N_THR, THR_MAX),
              "protocols": lambda: protocols._launch(pd, gd, i0, grp, GROUPS, acc_p, 0)}
    us = {"detail": [], "protocols": []}
    for fn in launch.values():
        for _ in range(warmup):
            fn()
    for _ in range(rounds):                                            # alternate, so drift hits both alike
        for name, fn in launch.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / iters)
    want = numpy_sums(pred.numpy(), gt.numpy(), i0, group.numpy(), GROUPS)
    a_end = 2 * GROUPS * p * 17
    hit = np.zeros(got.size, dtype=bool)
    hit[a_end:a_end + 6 * GROUPS * p].reshape(-1, 6)[:, :4] = True
    hit[a_end + 6 * GROUPS * p:] = True
    soft = ~hit & (want != 0)
    best_d, best_p = min(us["detail"]), min(us["protocols"])
    return {"b": b, "p": p, "i0": i0, "joints": 17, "groups": GROUPS, "n_thr": N_THR, "poses": b * p,
            "detail_op_us": round(best_d, 2), "protocols_op_us": round(best_p, 2), "ratio": round(best_d / best_p, 3),
            "detail_op_us_rounds": [round(v, 2) for v in us["detail"]], "protocols_op_us_rounds": [round(v, 2) for v in us["protocols"]],
            "max_rel_diff_vs_numpy": float(np.max(np.abs(got[soft] - want[soft]) / np.abs(want[soft]))),
            "hit_counts_equal": bool(np.array_equal(got[hit], want[hit]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import detail_metrics, protocols, train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "op": [time_ops(256, 40, 0, 40, a.iters, a.rounds, a.warmup), time_ops(256, 40, 15, 25, a.iters, a.rounds, a.warmup)]}
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, 17, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(d, 17, nb, seed=0))
    head.to(dev).eval()
    store = SyntheticStore(a.clips, 40, dev)
    ids = [i % GROUPS for i in range(a.clips)]
    names = [f"action{g:02d}" for g in range(GROUPS)]
    passes = {"evaluate_detail": lambda: detail_metrics.evaluate_detail(head, store, ids, names, 15, 25),
              "evaluate_protocols": lambda: protocols.evaluate_protocols(head, store, ids, names, 15, 25)}
    ms = {name: [] for name in passes}
    res = {}
    for fn in passes.values():
        fn()
    for _ in range(a.passes):
        for name, fn in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name] = fn()
            ms[name].append(round((time.perf_counter() - t0) * 1e3, 2))
    out["pass"] = {"clips": a.clips, "batch_size": 256, "latent_dim": d, "precision": "fp16", "input_len": 15, "pred_len": 25,
                   "evaluate_detail_ms": ms["evaluate_detail"], "evaluate_protocols_ms": ms["evaluate_protocols"],
                   "p1p2_all_mm": [round(float(v) * 1e3, 3) for v in res["evaluate_detail"]["recon_p1p2_all"]],
                   "protocols_all_mm": [round(float(v) * 1e3, 3) for v in res["evaluate_protocols"]["recon_all"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
