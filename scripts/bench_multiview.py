"""Multi-view fusion on one MI355X.  In one process:

* the two ops of include/r50_multiview.h at the test split's size -- --takes 120 takes of 4 views of --rows 1500 rows, J 17 (7.2e5 rows,
  1,440 pairs of 25,500 points) -- beside a device copy of the poses' bytes (``out.copy_(x)``) and the plain torch composition on the
  device in fp32: the matched rows gathered into a padded batch (every pair has the same length here, the most favourable case for
  it), centred, ``bmm`` for the 3x3 moments, a batched ``torch.linalg.svd`` with the determinant correction (Kabsch); and for the fuse
  ``index_select`` of the peers' rows and transforms, ``bmm`` and ``mean``.  They alternate in rounds of --iters launches (the torch
  fit: --torch-iters), each round under a host clock that ends in a synchronise; the figure is the best round of each;
* one ``sequences.evaluate_dense`` pass over a synthetic four-camera store of --clips clips (rigid ground truths) as ``results
  --dense`` runs it, and the same pass followed by ``multiview.evaluate_multiview`` as ``--multiview`` runs it; PHD(1024, 17, 2) fp16,
  host clock, synchronised, --passes each after a warm-up, alternating;
* with --parent-tree DIR (a checkout of the parent commit with its library built): the dense pass without the flag in fresh child
  processes, this tree and the parent's alternating, --sessions each.
Prints one JSON line.
    python scripts/bench_multiview.py [--iters 100] [--rounds 5] [--clips 1024] [--passes 5] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.path.dirname(HERE)
if "--tree" in sys.argv:                                                         # --dense-only: time another checkout's dense pass
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "scripts"))

from bench_dense import GROUPS, PER_VIDEO, STRIDE, DenseStore, T  # noqa: E402

J, VIEWS = 17, 4


def rotations(n, g):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
    q[:, :, 0] *= torch.sign(torch.linalg.det(q))[:, None]
    return q


def camera_poses(world, g):
    """world (V, L, J, 3) fp64 around the origin -> fp32 poses of one camera per leading entry, about 5 m in front of it."""
    v = world.shape[0]
    t = torch.tensor([0.0, 0.0, 5.0], dtype=torch.float64) + torch.randn(v, 3, generator=g, dtype=torch.float64) * torch.tensor([0.5, 0.5, 0.1])
    return (torch.einsum("vab,vljb->vlja", rotations(v, g), world) + t[:, None, None, :]).float()


class MultiViewStore(DenseStore):
    """``DenseStore`` whose videos are the VIEWS cameras of takes: video v is camera v % VIEWS of take v // VIEWS, its ground truth a
    rigid image of the take's track."""

    def __init__(self, n, t, dev, seed=0):
        super().__init__(n, t, dev, seed)
        g = torch.Generator().manual_seed(seed + 7)
        videos = (n + PER_VIDEO - 1) // PER_VIDEO
        takes = (videos + VIEWS - 1) // VIEWS
        length = STRIDE * (PER_VIDEO - 1) + t
        track = (torch.randn(takes, 1, J, 3, generator=g, dtype=torch.float64) * 0.3 +
                 torch.cumsum(torch.randn(takes, length, J, 3, generator=g, dtype=torch.float64) * 0.01, dim=1))
        seen = camera_poses(track.repeat_interleave(VIEWS, dim=0)[:videos], g)
        i = torch.arange(n)
        frames = (STRIDE * (i % PER_VIDEO))[:, None] + torch.arange(t)[None, :]
        self.joints3d = seen[(i // PER_VIDEO)[:, None], frames].contiguous().to(dev)
        self._clips = [{"subject": 9, "action": f"action{(v // VIEWS) % GROUPS:02d}_{v // VIEWS // GROUPS + 1}", "cam": v % VIEWS + 1,
                        "start": STRIDE * (k % PER_VIDEO), "end": STRIDE * (k % PER_VIDEO) + t} for k in range(n) for v in [k // PER_VIDEO]]


def time_ops(takes, rows, iters, torch_iters, rounds, warmup):
    from implementation_phd_lab_vision_amd import multiview as mv
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    n_seq, f = takes * VIEWS, takes * VIEWS * rows
    world = (torch.randn(takes, 1, J, 3, generator=g, dtype=torch.float64) * 0.3 +
             torch.cumsum(torch.randn(takes, rows, J, 3, generator=g, dtype=torch.float64) * 0.01, dim=1))
    gt = camera_poses(world.repeat_interleave(VIEWS, dim=0), g)
    x = (gt + torch.randn(n_seq, rows, J, 3, generator=g) * 0.03).reshape(f, J, 3).contiguous().to(dev)
    keys = [(9, f"take{s // VIEWS:03d}", s % VIEWS + 1) for s in range(n_seq)]
    table = mv.ViewTable.from_sequences(keys, (np.arange(n_seq + 1) * rows).astype(np.int32), np.tile(np.arange(rows, dtype=np.int32), n_seq))
    views = mv.DeviceViews(table, dev)
    p = table.pairs
    fit = mv.rigid_fit(x, x, views)
    out = torch.empty_like(x)
    src = views.match.view(-1, 2)[:, 0].long().contiguous()
    dst = views.match.view(-1, 2)[:, 1].long().contiguous()
    peer_row, peer_fit = views.peer_row.long(), views.peer_fit.long()

    def torch_fit():
        y, z = x.index_select(0, src).view(p, rows * J, 3), x.index_select(0, dst).view(p, rows * J, 3)
        my, mz = y.mean(dim=1, keepdim=True), z.mean(dim=1, keepdim=True)
        u, _, vt = torch.linalg.svd(torch.bmm((z - mz).transpose(1, 2), y - my))
        sign = torch.sign(torch.linalg.det(u) * torch.linalg.det(vt))
        r = torch.bmm(u * torch.stack([torch.ones_like(sign), torch.ones_like(sign), sign], dim=1)[:, None, :], vt)
        return r, mz.squeeze(1) - torch.bmm(r, my.transpose(1, 2)).squeeze(2)

    rot32, t32 = fit[:, :9].reshape(p, 3, 3).float().contiguous(), fit[:, 9:12].float().contiguous()

    def torch_fuse():
        peers = x.index_select(0, peer_row)                                        # (F * 3, J, 3): every row has VIEWS - 1 peers here
        moved = torch.bmm(peers, rot32.index_select(0, peer_fit).transpose(1, 2)) + t32.index_select(0, peer_fit)[:, None, :]
        return torch.cat([x[:, None], moved.view(f, VIEWS - 1, J, 3)], dim=1).mean(dim=1)

    launch = {"view_rigid_fit": lambda: mv.rigid_fit(x, x, views), "view_fuse_mean": lambda: mv.fuse_views(x, views, fit, 0),
              "view_fuse_median": lambda: mv.fuse_views(x, views, fit, 1), "device_copy": lambda: out.copy_(x),
              "torch_kabsch_svd": torch_fit, "torch_fuse_mean": torch_fuse}
    n_iter = {name: torch_iters if name == "torch_kabsch_svd" else iters for name in launch}
    us = {name: [] for name in launch}
    for name, fn in launch.items():
        for _ in range(min(warmup, n_iter[name])):
            fn()
    for _ in range(rounds):                                                      # alternate, so drift hits all alike
        for name, fn in launch.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_iter[name]):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / n_iter[name])
    res = {"takes": takes, "views": VIEWS, "rows_per_view": rows, "rows": f, "pairs": p, "points_per_pair": rows * J, "joints": J,
           "pose_bytes": f * J * 3 * 4, "iters": iters, "torch_kabsch_iters": torch_iters}
    for name, v in us.items():
        res[name + "_us"] = round(min(v), 2)
        res[name + "_us_rounds"] = [round(t, 2) for t in v]
    r_t, t_t = torch_fit()
    res["max_abs_diff_rotation_vs_torch_fp32"] = float((fit[:, :9].reshape(p, 3, 3) - r_t.double()).abs().max())
    res["max_abs_diff_translation_vs_torch_fp32"] = float((fit[:, 9:12] - t_t.double()).abs().max())
    res["max_abs_diff_fuse_vs_torch_fp32"] = float((mv.fuse_views(x, views, fit, 0)[0] - torch_fuse()).abs().max())
    res["pair_rms_mm_mean"] = round(float(fit[:, 13].mean()) * 1e3, 3)
    return res


def make_head(dev):
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    head = PHDFor3DJoints(1024, 17, 2, precision="fp16")
    head.load_state_dict(train.default_state_dict(1024, 17, 2, seed=0))
    return head.to(dev).eval()


def timed(passes, n):
    ms = {name: [] for name in passes}
    last = {}
    for fn in passes.values():
        fn()
    for _ in range(n):
        for name, fn in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            ms[name].append(round((time.perf_counter() - t0) * 1e3, 2))
    return ms, last


def dense_only(clips, passes):
    """The dense pass without the flag over ``bench_dense.DenseStore``, code that the parent commit has as well."""
    from implementation_phd_lab_vision_amd import sequences
    dev = "cuda:0"
    head, store = make_head(dev), DenseStore(clips, T, dev)
    ms, last = timed({"dense": lambda: sequences.evaluate_dense(head, store, fuse="context")}, passes)
    return {"tree": TREE, "evaluate_dense_ms": ms["dense"], "p1_all": float(last["dense"]["p1_all"]), "frames": int(last["dense"]["frames_all"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--takes", type=int, default=120)
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--parent-tree", type=str, default=None)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--tree", type=str, default=None)
    a = ap.parse_args()
    if a.dense_only:
        print(json.dumps(dense_only(a.clips, a.passes)))
        return
    from implementation_phd_lab_vision_amd import multiview as mv, sequences
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "op": time_ops(a.takes, a.rows, a.iters, a.torch_iters, a.rounds, a.warmup)}
    head, store = make_head(dev), MultiViewStore(a.clips, T, dev)

    def with_flag():
        dense = sequences.evaluate_dense(head, store, fuse="context", keep_poses=True)
        return dense, mv.evaluate_multiview(dense, dev)

    ms, last = timed({"off": lambda: sequences.evaluate_dense(head, store, fuse="context"), "on": with_flag}, a.passes)
    dense, multi = last["on"]
    out["pass"] = {"clips": a.clips, "frames": int(dense["frames_all"]), "sequences": int(dense["sequences"]), "takes": multi["mv_takes"],
                   "pairs": multi["mv_pairs"], "excluded_takes": multi["excluded_takes"], "evaluate_dense_ms": ms["off"],
                   "evaluate_dense_then_multiview_ms": ms["on"],
                   "p1_all_mm_single_fused": [round(float(dense["p1_all"]) * 1e3, 3), round(float(multi["mv_p1_all"]) * 1e3, 3)],
                   "pair_rms_gt_max_mm": round(float(np.max(multi["mv_pair_rms_gt"])) * 1e3, 6)}
    if a.parent_tree:
        trees = {"this": os.path.dirname(HERE), "parent": os.path.abspath(a.parent_tree)}
        runs = {name: [] for name in trees}
        for _ in range(a.sessions):                                              # fresh child processes, alternating
            for name, tree in trees.items():
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--dense-only", "--tree", tree, "--clips", str(a.clips),
                                      "--passes", str(a.passes)], capture_output=True, text=True, timeout=600, cwd=tree)
                if res.returncode != 0:
                    raise SystemExit(f"the dense pass of {tree} failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
                runs[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
        out["dense_without_flag_vs_parent"] = {name: {"evaluate_dense_ms": [r["evaluate_dense_ms"] for r in v],
                                                      "best_ms": min(min(r["evaluate_dense_ms"]) for r in v), "p1_all": v[0]["p1_all"]}
                                               for name, v in runs.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
