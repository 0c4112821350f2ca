"""2D-guided refinement of stitched sequences on one MI355X.  In one process:

* the two ops of include/r50_refine.h at the test split's size -- --sequences 300 sequences of --rows 1000 rows, J 17 (3.0e5 rows), the
  default weights, --sweeps 50 sweeps a call -- beside a device copy of the poses (``out.copy_(x)``: its time tells whether a round ran
  out of the cache) and the plain torch composition of ONE sweep on the device in fp64: the 2D block by broadcasting, the second
  differences by slicing (all sequences have one segment here, so a mask at the sequence ends is all it takes), the 3x3 systems by
  ``torch.linalg.solve``.  They alternate in rounds of --iters calls, each round under a host clock that ends in a synchronise; the
  figure is the best round of each;
* one ``sequences.evaluate_dense(keep_poses=True)`` pass over a synthetic store of --clips clips, without and with
  ``refine.evaluate_refine`` after it (what ``results --dense --dense-refine`` adds), PHD(1024, 17, 2) fp16, host clock, synchronised,
  --passes each after a warm-up, alternating.
Prints one JSON line.
    python scripts/bench_refine.py [--iters 20] [--rounds 5] [--clips 1024] [--passes 5]
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

from bench_dense import DenseStore, T  # noqa: E402

J = 17
FOCAL, CENTRE = 1150.0 * 224.0 / 1000.0, 112.0        # a 1000-pixel person box resized to the 224 crop


class RefineStore(DenseStore):
    """``DenseStore`` with the 2D joints and the camera ``dense_rays`` reads: the projection of the ground truth through one K."""

    def __init__(self, n, t, dev, seed=0):
        super().__init__(n, t, dev, seed)
        self.K = torch.tensor([[FOCAL, 0.0, CENTRE], [0.0, FOCAL, CENTRE], [0.0, 0.0, 1.0]], device=dev).expand(n, 3, 3).contiguous()
        self.joints2d = (self.joints3d[..., :2] / self.joints3d[..., 2:3] * FOCAL + CENTRE).contiguous()

    def get_batch(self, idx):
        i = torch.as_tensor(idx, dtype=torch.long, device=self.feats.device)
        return self.feats.index_select(0, i), self.joints3d.index_select(0, i), self.joints2d.index_select(0, i), self.K.index_select(0, i)


def torch_sweep(x, p0, z0, rays, valid, s):
    """One sweep in fp64 torch: x, p0 (S, R, J, 3), z0 (S, R, J), rays (S, R, J, 2), valid (R,) = 1 at the stencil centres."""
    pz = x[..., 2]
    on = (pz >= s.z_min).to(x.dtype) * s.lambda_2d
    safe = torch.where(pz >= s.z_min, pz, torch.ones_like(pz))
    q = x[..., :2] / safe[..., None]
    r = z0[..., None] * (q - rays)
    sc = z0 / safe
    g = torch.stack([sc * r[..., 0], sc * r[..., 1], -sc * (q * r).sum(-1)], dim=-1) * on[..., None]
    h = torch.zeros(x.shape + (3,), dtype=x.dtype, device=x.device)
    ss = on * sc * sc
    h[..., 0, 0] = h[..., 1, 1] = ss
    h[..., 0, 2] = h[..., 2, 0] = -ss * q[..., 0]
    h[..., 1, 2] = h[..., 2, 1] = -ss * q[..., 1]
    h[..., 2, 2] = ss * (q * q).sum(-1)
    g = g + s.lambda_3d * (x - p0)
    a = torch.zeros_like(x)
    a[:, 1:-1] = (x[:, :-2] - 2.0 * x[:, 1:-1] + x[:, 2:])
    a = a * valid[None, :, None, None]
    ap = torch.nn.functional.pad(a, (0, 0, 0, 0, 1, 1))
    vp = torch.nn.functional.pad(valid, (1, 1))
    g = g + s.lambda_acc * (ap[:, :-2] - 2.0 * ap[:, 1:-1] + ap[:, 2:])
    diag = s.lambda_3d + s.lambda_acc * (vp[:-2] + 4.0 * vp[1:-1] + vp[2:])
    h = h + diag[None, :, None, None, None] * torch.eye(3, dtype=x.dtype, device=x.device)
    return x - s.omega * torch.linalg.solve(h, g[..., None])[..., 0]


def time_ops(n_seq, rows, sweeps, iters, rounds, warmup):
    from implementation_phd_lab_vision_amd import refine as R
    from implementation_phd_lab_vision_amd import smooth
    dev = "cuda:0"
    f = n_seq * rows
    g = torch.Generator().manual_seed(0)
    body = torch.randn(J, 3, generator=g) * 0.25 + torch.tensor([0.0, 0.0, 5.0])
    gt = body + torch.cumsum(torch.randn(n_seq, rows, J, 3, generator=g) * 0.002, dim=1)
    pred = gt + 0.03 * torch.nn.functional.normalize(torch.randn(J, 3, generator=g), dim=1) + torch.randn(gt.shape, generator=g) * 0.0115
    x = pred.reshape(f, J, 3).contiguous().to(dev)
    rays = (gt[..., :2] / gt[..., 2:3]).reshape(f, J, 2).contiguous().to(dev)
    tables = smooth.DeviceTables((np.arange(n_seq + 1) * rows).astype(np.int32), np.tile(np.arange(rows, dtype=np.int32), n_seq), dev)
    s, one = R.RefineSettings(iters=sweeps), R.RefineSettings(iters=1)
    ws = torch.empty(2 * f * J * 3, dtype=torch.float64, device=dev)
    out = torch.empty_like(x)
    x64, rays64 = x.double().view(n_seq, rows, J, 3), rays.double().view(n_seq, rows, J, 2)
    z0 = x64[..., 2].clamp_min(s.z_min)
    valid = torch.ones(rows, dtype=torch.float64, device=dev)
    valid[0] = valid[-1] = 0.0

    launch = {"fit_sweeps": lambda: R.fit_sweeps(x, rays, None, tables, s, workspace=ws),
              "fit_sweeps_1": lambda: R.fit_sweeps(x, rays, None, tables, one, workspace=ws),
              "fit_energy": lambda: R.fit_energy(x, x, rays, None, tables, s.z_min), "device_copy": lambda: out.copy_(x),
              "torch_one_sweep_fp64": lambda: torch_sweep(x64, x64, z0, rays64, valid, s)}
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
    res = {"sequences": n_seq, "rows_per_sequence": rows, "rows": f, "joints": J, "sweeps": sweeps, "bytes_x": f * J * 3 * 4,
           "bytes_one_sweep_fp64_in_plus_out": f * J * (3 * 8 * 2 + (3 + 2) * 4)}
    for name, v in us.items():
        res[name + "_us"] = round(min(v), 2)
        res[name + "_us_rounds"] = [round(t, 2) for t in v]
    res["fit_sweeps_us_per_sweep"] = round(res["fit_sweeps_us"] / max(sweeps, 1), 2)
    refined = R.fit_sweeps(x, rays, None, tables, s, workspace=ws)
    first = R.fit_sweeps(x, rays, None, tables, one, workspace=ws)
    res["max_abs_diff_one_sweep_vs_torch_fp64"] = float((first.double().view_as(x64) - torch_sweep(x64, x64, z0, rays64, valid, s)).abs().max())
    gt_d = gt.reshape(f, J, 3).to(dev)
    res["mean_joint_error_mm_raw_refined"] = [round(float((v - gt_d).norm(dim=2).mean()) * 1e3, 3) for v in (x, refined)]
    en = [R.fit_energy(v, x, rays, None, tables, s.z_min).sum(dim=0).cpu().numpy() for v in (x, refined)]
    res["energy_raw_refined"] = [round(float(e[0] + e[1] + e[2]), 4) for e in en]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sequences", type=int, default=300)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import refine as R
    from implementation_phd_lab_vision_amd import sequences, train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "op": time_ops(a.sequences, a.rows, a.sweeps, a.iters, a.rounds, a.warmup)}
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, 17, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(d, 17, nb, seed=0))
    head.to(dev).eval()
    store = RefineStore(a.clips, T, dev)
    settings = R.RefineSettings(iters=a.sweeps)

    def refine_on():
        dense = sequences.evaluate_dense(head, store, fuse="context", keep_poses=True)
        return dense, R.evaluate_refine(dense, store, dev, settings)

    passes = {"plain": lambda: sequences.evaluate_dense(head, store, fuse="context"),
              "keep_poses": lambda: sequences.evaluate_dense(head, store, fuse="context", keep_poses=True), "refine_on": refine_on}
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
    dense, fitted = res["refine_on"]
    out["pass"] = {"clips": a.clips, "frames": dense["frames_all"], "sequences": dense["sequences"],
                   "evaluate_dense_ms": ms["plain"], "evaluate_dense_keep_poses_ms": ms["keep_poses"],
                   "evaluate_dense_keep_poses_plus_evaluate_refine_ms": ms["refine_on"],
                   "p1_all_mm_raw_refined": [round(float(dense["p1_all"]) * 1e3, 3), round(float(fitted["refine_p1_all"]) * 1e3, 3)],
                   "reprojection_all_mm_raw_refined": [round(float(fitted["refine_residual_raw_all"]) * 1e3, 3),
                                                       round(float(fitted["refine_residual_all"]) * 1e3, 3)],
                   "skipped": fitted["refine_skipped"].tolist()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
