"""Joint rotations on a rigid skeleton on one MI355X.  In one process:

* the two ops of include/r50_kinematics.h at the test split's size -- --sequences 300 sequences of --rows 1000 rows, J 17 (3.0e5 rows) --
  beside a device copy of the same bytes (``out.copy_(x)``: its time tells whether a round ran out of the cache) and the plain torch
  composition of the per-frame pass on the device in fp32: batched cross products for the two frames and the aims, ``bmm`` down the
  edge list, the rest offsets taken as given.  They alternate in rounds of --iters launches, each round under a host clock that ends in
  a synchronise; the figure is the best round of each;
* the same per-frame pass as a host numpy loop over the joints, vectorised over the frames, fp64, once, for scale;
* one ``sequences.evaluate_dense(keep_poses=True)`` pass over a synthetic store of --clips clips, without and with
  ``kinematics.evaluate_rigid`` after it (what ``results --dense --dense-rigid`` adds), PHD(1024, 17, 2) fp16, host clock,
  synchronised, --passes each after a warm-up, alternating.
Prints one JSON line.
    python scripts/bench_kinematics.py [--iters 100] [--rounds 5] [--clips 1024] [--passes 5]
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


def _unit(v, xp):
    return v / xp.linalg.norm(v, axis=-1, keepdims=True) if xp is np else v / v.norm(dim=-1, keepdim=True)


def per_frame_pass(xw, rest, sk, xp):
    """The per-frame pass without its degenerate branches, vectorised over the frames: xw (F, J, 3) world-frame poses, rest (F, J, 3)
    each frame's rest offsets.  ``xp`` is numpy (fp64, the host loop) or torch (fp32, the device composition).  Returns the global
    rotations (F, J, 3, 3) and the rebuilt positions (F, J, 3)."""
    tor = xp is not np
    cross = (lambda a, b: torch.linalg.cross(a, b)) if tor else (lambda a, b: np.cross(a, b))
    stack = (lambda v: torch.stack(v, dim=-1)) if tor else (lambda v: np.stack(v, axis=-1))
    mv = (lambda m, v: torch.bmm(m, v.unsqueeze(-1)).squeeze(-1)) if tor else (lambda m, v: np.einsum("fij,fj->fi", m, v))
    mm = (lambda a, b: torch.bmm(a, b)) if tor else (lambda a, b: a @ b)
    f = xw.shape[0]
    eye = (torch.eye(3, dtype=xw.dtype, device=xw.device) if tor else np.eye(3)).reshape(1, 3, 3)
    eye = eye.expand(f, 3, 3) if tor else np.broadcast_to(eye, (f, 3, 3))
    framed = {int(r[0]): [int(v) for v in r[1:]] for r in sk.frames}
    rot, pos = {}, {}
    for j in [sk.root] + [int(c) for c in sk.edges[:, 1]]:
        p = int(sk.parent[j])
        rp = eye if p < 0 else rot[p]
        pos[j] = xw[:, j] if p < 0 else pos[p] + mv(rp, rest[:, j])
        if j in framed:
            a0, a1, b0, b1 = framed[j]
            ex = _unit(xw[:, a1] - xw[:, a0], xp)
            ez = _unit(cross(ex, xw[:, b1] - xw[:, b0]), xp)
            rot[j] = stack([ex, cross(ez, ex), ez])
        elif len(sk.children[j]) == 1:
            c = sk.children[j][0]
            d = torch.from_numpy(sk.rest_dirs[c]).to(xw) if tor else sk.rest_dirs[c]
            u = mv(rp, d.expand(f, 3) if tor else np.broadcast_to(d, (f, 3)))
            v = _unit(xw[:, c] - pos[j], xp)
            k = cross(u, v)
            zero = k[:, 0] * 0
            kx = stack([stack([zero, k[:, 2], -k[:, 1]]), stack([-k[:, 2], zero, k[:, 0]]), stack([k[:, 1], -k[:, 0], zero])])
            dot = (u * v).sum(-1).reshape(f, 1, 1)
            rot[j] = mm(eye + kx + mm(kx, kx) / (1.0 + dot), rp)
        else:
            rot[j] = rp
    order = range(sk.joints)
    return (torch.stack([rot[j] for j in order], dim=1), torch.stack([pos[j] for j in order], dim=1)) if tor else \
        (np.stack([rot[j] for j in order], axis=1), np.stack([pos[j] for j in order], axis=1))


def time_ops(n_seq, rows, iters, rounds, warmup):
    from implementation_phd_lab_vision_amd import kinematics as K
    from implementation_phd_lab_vision_amd import smooth
    dev = "cuda:0"
    sk = K.H36M_SKELETON
    f = n_seq * rows
    g = torch.Generator().manual_seed(0)
    # a T-pose figure that sways: every frame keeps the frames and the aims well conditioned
    tpose = torch.zeros(J, 3)
    off = {1: (-0.13, 0, 0), 4: (0.13, 0, 0), 7: (0, 0.24, 0), 8: (0, 0.26, 0), 9: (0, 0.11, 0), 10: (0, 0.12, 0), 11: (0.17, 0, 0), 14: (-0.17, 0, 0),
           12: (0.28, 0, 0), 13: (0.25, 0, 0), 15: (-0.28, 0, 0), 16: (-0.25, 0, 0), 2: (0, -0.45, 0), 3: (0, -0.45, 0), 5: (0, -0.45, 0), 6: (0, -0.45, 0)}
    for p, c in sk.edges.tolist():
        tpose[c] = tpose[p] + torch.tensor(off[c], dtype=torch.float32)
    world = tpose + torch.tensor([0.0, 0.0, -5.0]) + torch.cumsum(torch.randn(n_seq, rows, J, 3, generator=g) * 0.002, dim=1)
    x_host = (world * torch.from_numpy(sk.sign).float()).reshape(f, J, 3).contiguous()
    x = x_host.to(dev)
    seq_start = (np.arange(n_seq + 1) * rows).astype(np.int32)
    tables = smooth.DeviceTables(seq_start, np.tile(np.arange(rows, dtype=np.int32), n_seq), dev)
    rest = K.rest_offsets(x, tables, sk)
    out = torch.empty_like(x)
    sign32 = torch.from_numpy(sk.sign).float().to(dev)
    rest_rows32 = rest.float().repeat_interleave(rows, dim=0)

    def torch_pass():
        return per_frame_pass(x * sign32, rest_rows32, sk, torch)

    launch = {"rest_offsets": lambda: K.rest_offsets(x, tables, sk), "pose_rotations": lambda: K.pose_rotations(x, tables, sk, rest),
              "device_copy": lambda: out.copy_(x), "torch_cross_bmm_fp32": torch_pass}
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
    res = {"sequences": n_seq, "rows_per_sequence": rows, "rows": f, "joints": J, "bytes_x": f * J * 3 * 4,
           "bytes_pose_rotations_in_plus_out": f * J * (3 + 4 + 3 + 3) * 4 + 2 * f * 4}
    for name, v in us.items():
        res[name + "_us"] = round(min(v), 2)
        res[name + "_us_rounds"] = [round(t, 2) for t in v]
    rot = K.pose_rotations(x, tables, sk, rest)
    res["flagged_frames"] = int(torch.count_nonzero(rot.flags))
    res["mean_residual_mm"] = round(float(rot.resid.double().mean()) * 1e3, 4)
    res["max_abs_diff_rigid_vs_torch_fp32"] = float((rot.rigid * sign32 - torch_pass()[1]).abs().max())
    xs = x_host.numpy().astype(np.float64) * sk.sign
    rest_rows = np.repeat(rest.cpu().numpy(), rows, axis=0)
    t0 = time.perf_counter()
    host = per_frame_pass(xs, rest_rows, sk, np)[1]
    res["per_frame_pass_host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["max_abs_diff_rigid_vs_host_fp64"] = float(np.abs(rot.rigid.cpu().numpy().astype(np.float64) * sk.sign - host).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sequences", type=int, default=300)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import kinematics as K
    from implementation_phd_lab_vision_amd import sequences, train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "op": time_ops(a.sequences, a.rows, a.iters, a.rounds, a.warmup)}
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, 17, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(d, 17, nb, seed=0))
    head.to(dev).eval()
    store = DenseStore(a.clips, T, dev)

    def rigid_on():
        dense = sequences.evaluate_dense(head, store, fuse="context", keep_poses=True)
        return dense, K.evaluate_rigid(dense, None, dev)

    passes = {"plain": lambda: sequences.evaluate_dense(head, store, fuse="context"),
              "keep_poses": lambda: sequences.evaluate_dense(head, store, fuse="context", keep_poses=True), "rigid_on": rigid_on}
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
    dense, rigid = res["rigid_on"]
    out["pass"] = {"clips": a.clips, "frames": dense["frames_all"], "sequences": dense["sequences"],
                   "evaluate_dense_ms": ms["plain"], "evaluate_dense_keep_poses_ms": ms["keep_poses"],
                   "evaluate_dense_keep_poses_plus_evaluate_rigid_ms": ms["rigid_on"],
                   "p1_all_mm_raw_rigid": [round(float(dense["p1_all"]) * 1e3, 3), round(float(rigid["rigid_p1_all"]) * 1e3, 3)],
                   "residual_all_mm": round(float(rigid["rigid_residual_all"]) * 1e3, 3), "flagged": rigid["rigid_flagged"].tolist()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
