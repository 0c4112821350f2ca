"""Dense evaluation on one MI355X.  In one process:

* ``r50_op_stitch_poses`` (context, ramp 13) and ``r50_op_sequence_metrics`` at N 8192 clips x T 40 x J 17, stride 5 (128 videos of 64
  clips, 15 actions), beside the same fusion written with torch on the device -- ``index_add_`` of the weighted rows and of the
  weights, then a division, in fp32: the naive program, atomics and so not reproducible to the bit.  The three alternate in rounds of
  --iters launches, each round under a warmed host clock that ends in a synchronise; the figure is the best round of each;
* the bytes the stitch op must move (pred and gt read once, the outputs written once) over its time, beside the device copy rate
  of ``scripts/hbm_copy_probe.py`` (its 256 MB ``copy_``: read + write) taken in the same run;
* one ``sequences.evaluate_dense`` pass beside one ``protocols.evaluate_protocols`` pass over the same synthetic store of --clips
  clips resident on the device, PHD(1024, 17, 2) fp16 (host clock, synchronised, best of --passes after a warm-up pass each,
  alternating).
Prints one JSON line.
    python scripts/bench_dense.py [--iters 50] [--rounds 5] [--clips 1024] [--passes 3]
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

from bench_protocols import GROUPS, SyntheticStore  # noqa: E402

T, J, STRIDE, PER_VIDEO, RAMP = 40, 17, 5, 64, 13


def video_clips(n):
    """n index entries: videos of PER_VIDEO clips at STRIDE, one action per video (GROUPS actions in turn)."""
    return [{"subject": 9, "action": f"action{(i // PER_VIDEO) % GROUPS:02d}_{i // PER_VIDEO // GROUPS + 1}", "cam": 1,
             "start": STRIDE * (i % PER_VIDEO), "end": STRIDE * (i % PER_VIDEO) + T} for i in range(n)]


def video_poses(n, seed):
    """gt (n, T, J, 3) fp32 cut from one pose track per video, so that clips agree on every shared frame."""
    g = torch.Generator().manual_seed(seed)
    videos = (n + PER_VIDEO - 1) // PER_VIDEO
    length = STRIDE * (PER_VIDEO - 1) + T
    track = (torch.randn(videos, 1, 1, 3, generator=g) * torch.tensor([1.0, 0.5, 0.5]) + torch.tensor([0.0, 0.0, 4.5]) +
             torch.randn(videos, 1, J, 3, generator=g) * 0.3 + torch.randn(videos, length, J, 3, generator=g) * 0.02).float()
    i = torch.arange(n)
    frames = (STRIDE * (i % PER_VIDEO))[:, None] + torch.arange(T)[None, :]
    return track[(i // PER_VIDEO)[:, None], frames].contiguous()


class DenseStore(SyntheticStore):
    """``SyntheticStore`` with index entries and a ground truth that is one track per video."""
    augment = False

    def __init__(self, n, t, dev, seed=0):
        super().__init__(n, t, dev, seed)
        self.joints3d = video_poses(n, seed + 1).to(dev)
        self._clips = video_clips(n)

    def item_clips(self):
        return self._clips

    def item_actions(self):
        return [c["action"] for c in self._clips]


def copy_probe_tbs(dev, mb=256):
    """``scripts/hbm_copy_probe.py``'s ``copy (read + write)`` figure at 256 MB, TB/s."""
    n = mb * 1024 * 1024 // 4
    a = torch.randn(n, device=dev)
    b = torch.empty_like(a)
    for _ in range(5):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2 * n * 4 / (e0.elapsed_time(e1) / 50) / 1e9


def time_ops(n, iters, rounds, warmup):
    from implementation_phd_lab_vision_amd import sequences as sq
    dev = "cuda:0"
    table = sq.SequenceTable.from_clips(video_clips(n), T)
    gt = video_poses(n, 3)
    pred = (gt + torch.randn(n, T, J, 3, generator=torch.Generator().manual_seed(4)) * 0.05).contiguous()
    pd, gd = pred.to(dev), gt.to(dev)
    index = sq.StitchIndex(table.offsets, table.src, n * T, dev)
    f = table.frames
    out = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in ((f, J, 3), (f, J, 3), (f,), (f,)))
    seq, idx = torch.from_numpy(table.seq).to(dev), torch.from_numpy(table.idx).to(dev)
    group = torch.from_numpy((table.seq % GROUPS).astype(np.int32)).to(dev)
    # the naive program: every pose row scattered to its frame with index_add_, fp32
    dst_host = np.empty(n * T, dtype=np.int64)
    dst_host[table.src] = np.repeat(np.arange(f), np.diff(table.offsets))
    dst = torch.from_numpy(dst_host).to(dev)
    w = torch.clamp(torch.arange(n * T, device=dev) % T + 1, max=RAMP).to(torch.float32)
    rows = pd.view(n * T, J * 3)

    def naive():
        num = torch.zeros((f, J * 3), dtype=torch.float32, device=dev).index_add_(0, dst, rows * w[:, None])
        den = torch.zeros(f, dtype=torch.float32, device=dev).index_add_(0, dst, w)
        return num / den[:, None]

    launch = {"stitch": lambda: sq.stitch_poses(pd, gd, index, 1, RAMP, out=out),
              "metrics": lambda: sq.sequence_metrics(out[0], out[1], out[2], index.offsets, seq, idx, group, GROUPS),
              "index_add": naive}
    us = {name: [] for name in launch}
    for fn in launch.values():
        for _ in range(warmup):
            fn()
    for _ in range(rounds):                                            # alternate, so drift hits all alike
        for name, fn in launch.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / iters)
    gap = float(out[3].max())
    diff = float((naive().view(f, J, 3) - out[0]).abs().max())
    moved = 2 * n * T * J * 3 * 4 + (2 * f * J * 3 + 2 * f) * 4
    best = {name: min(v) for name, v in us.items()}
    copy_tbs = copy_probe_tbs(dev)
    return {"clips": n, "t": T, "joints": J, "stride": STRIDE, "frames": f, "sequences": len(table.seq_keys), "groups": GROUPS,
            "mode": "context", "ramp": RAMP, "stitch_op_us": round(best["stitch"], 2), "metrics_op_us": round(best["metrics"], 2),
            "index_add_us": round(best["index_add"], 2), "index_add_over_stitch": round(best["index_add"] / best["stitch"], 3),
            "stitch_op_us_rounds": [round(v, 2) for v in us["stitch"]], "metrics_op_us_rounds": [round(v, 2) for v in us["metrics"]],
            "index_add_us_rounds": [round(v, 2) for v in us["index_add"]], "stitch_bytes": moved,
            "stitch_tb_per_s": round(moved / best["stitch"] / 1e6, 3), "copy_probe_tb_per_s": round(copy_tbs, 3),
            "stitch_share_of_copy": round(moved / best["stitch"] / 1e6 / copy_tbs, 3), "gt_gap_max": gap,
            "max_abs_diff_vs_index_add_fp32": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--op-clips", type=int, default=8192)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import protocols, sequences, train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds, "op": time_ops(a.op_clips, a.iters, a.rounds, a.warmup)}
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, 17, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(d, 17, nb, seed=0))
    head.to(dev).eval()
    store = DenseStore(a.clips, T, dev)
    names, ids = protocols.action_groups(store.item_actions())
    passes = {"evaluate_dense": lambda: sequences.evaluate_dense(head, store, fuse="context"),
              "evaluate_protocols": lambda: protocols.evaluate_protocols(head, store, ids, names)}
    ms = {name: [] for name in passes}
    res = {}
    for fn in passes.values():
        fn()
    for _ in range(a.passes):
        for name, fn in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name] = fn()
            torch.cuda.synchronize()
            ms[name].append(round((time.perf_counter() - t0) * 1e3, 2))
    dense = res["evaluate_dense"]
    out["pass"] = {"clips": a.clips, "batch_size": 256, "latent_dim": d, "precision": "fp16", "fuse": "context", "ramp": dense["ramp"],
                   "frames": dense["frames_all"], "clip_frames": dense["clip_frames"], "evaluate_dense_ms": ms["evaluate_dense"],
                   "evaluate_protocols_ms": ms["evaluate_protocols"],
                   "dense_all_mm": [round(float(dense[k]) * 1e3, 3) for k in ("p1_all", "p2_all", "mpjve_all", "accel_all", "spread_all")],
                   "protocols_all_mm": [round(float(v) * 1e3, 3) for v in res["evaluate_protocols"]["recon_all"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
