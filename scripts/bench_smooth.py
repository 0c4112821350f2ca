"""Smoothing and constant bone lengths of stitched sequences on one MI355X.  In one process:

* the four ops of include/r50_smooth.h at the test split's size -- --sequences 300 sequences of --rows 1000 rows, J 17 (3.0e5 rows) --
  beside a device copy of the same bytes (``out.copy_(x)``) and the plain torch composition of the FIR and the bone step on the
  device in fp32: ``F.pad(mode="replicate")`` + a depthwise ``conv1d`` over the sequences as one batch (every sequence has the same
  length here, the most favourable case for it; its edges are replicate-padded, not refitted), and ``index_select`` + ``norm`` + a mean
  per sequence, then the rebuild edge by edge.  They alternate in rounds of --iters launches, each round under a host clock that ends in
  a synchronise; the figure is the best round of each;
* the One-Euro recurrence as a host numpy loop over time, vectorised over sequences and coordinates, once, for scale;
* one ``sequences.evaluate_dense`` pass over a synthetic store of --clips clips with ``post`` off and with ``post`` on (gauss + bones),
  PHD(1024, 17, 2) fp16, host clock, synchronised, --passes each after a warm-up, alternating.
Prints one JSON line.
    python scripts/bench_smooth.py [--iters 300] [--rounds 5] [--clips 1024] [--passes 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dense import DenseStore, T  # noqa: E402

J = 17


def time_ops(n_seq, rows, iters, rounds, warmup):
    from implementation_phd_lab_vision_amd import smooth
    from implementation_phd_lab_vision_amd.train import H36M_EDGES
    dev = "cuda:0"
    f, c = n_seq * rows, 3 * J
    g = torch.Generator().manual_seed(0)
    x_host = (torch.randn(n_seq, 1, J, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 5.0]) +
              torch.cumsum(torch.randn(n_seq, rows, J, 3, generator=g) * 0.01, dim=1)).reshape(f, J, 3).contiguous()
    x = x_host.to(dev)
    seq_start = (np.arange(n_seq + 1) * rows).astype(np.int32)
    tables = smooth.DeviceTables(seq_start, np.tile(np.arange(rows, dtype=np.int32), n_seq), dev)
    gauss, savgol = smooth.upload_coef(smooth.gauss_table(1.5), dev), smooth.upload_coef(smooth.savgol_table(9, 2), dev)
    wide = smooth.upload_coef(smooth.gauss_table(31 / 3.0), dev)
    stats = smooth.bone_stats(x, tables, H36M_EDGES)
    out = torch.empty_like(x)
    edges = torch.tensor(H36M_EDGES, device=dev)
    kernel = torch.from_numpy(smooth.gauss_table(1.5)[5].astype(np.float32)).to(dev).view(1, 1, -1).repeat(c, 1, 1)

    def torch_fir():
        xs = x.view(n_seq, rows, c).permute(0, 2, 1)
        return F.conv1d(F.pad(xs, (5, 5), mode="replicate"), kernel, groups=c).permute(0, 2, 1).contiguous()

    def torch_bones():
        xs = x.view(n_seq, rows, J, 3)
        d = xs.index_select(2, edges[:, 1]) - xs.index_select(2, edges[:, 0])
        n = d.norm(dim=-1, keepdim=True)
        unit = d / n
        mean = n.mean(dim=1, keepdim=True)
        pos = xs.clone()
        for b, (pa, ch) in enumerate(H36M_EDGES):
            pos[:, :, ch] = pos[:, :, pa] + mean[:, :, b] * unit[:, :, b]
        return pos

    launch = {"fir_gauss_w11": lambda: smooth.fir_sequences(x, tables, gauss), "fir_savgol_w9": lambda: smooth.fir_sequences(x, tables, savgol),
              "fir_gauss_w63": lambda: smooth.fir_sequences(x, tables, wide), "one_euro": lambda: smooth.one_euro_sequences(x, tables, beta=0.01),
              "bone_stats": lambda: smooth.bone_stats(x, tables, H36M_EDGES),
              "bone_rebuild": lambda: smooth.fix_bone_lengths(x, tables, H36M_EDGES, stats),
              "device_copy": lambda: out.copy_(x), "torch_conv1d_w11": torch_fir, "torch_bones": torch_bones}
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
    res = {"sequences": n_seq, "rows_per_sequence": rows, "rows": f, "joints": J, "bytes_in_plus_out": 2 * f * c * 4}
    for name, v in us.items():
        res[name + "_us"] = round(min(v), 2)
        res[name + "_us_rounds"] = [round(t, 2) for t in v]
    interior = slice(5, rows - 5)
    a = smooth.fir_sequences(x, tables, gauss)[0].view(n_seq, rows, c)[:, interior]
    res["max_abs_diff_fir_vs_conv1d_interior"] = float((a - torch_fir().view(n_seq, rows, c)[:, interior]).abs().max())
    res["max_abs_diff_bones_vs_torch_fp32"] = float((smooth.fix_bone_lengths(x, tables, H36M_EDGES, stats)[0].view(n_seq, rows, J, 3) -
                                                     torch_bones()).abs().max())
    # the One-Euro recurrence on the host, vectorised over (sequence, coordinate), one step of time after the other
    xs = x_host.view(n_seq, rows, c).numpy().astype(np.float64)
    t0 = time.perf_counter()
    te, beta = 1.0 / 25.0, 0.01
    alpha = lambda fc: 1.0 / (1.0 + 1.0 / ((6.283185307179586 * fc) * te))  # noqa: E731
    xhat, dxhat = xs[:, 0].copy(), np.zeros((n_seq, c))
    host = np.empty((n_seq, rows, c), dtype=np.float32)
    host[:, 0] = xs[:, 0]
    for t in range(1, rows):
        dxhat = dxhat + alpha(1.0) * ((xs[:, t] - xhat) * 25.0 - dxhat)
        xhat = xhat + alpha(1.0 + beta * np.abs(dxhat)) * (xs[:, t] - xhat)
        host[:, t] = xhat
    res["one_euro_host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    got = smooth.one_euro_sequences(x, tables, beta=0.01).view(n_seq, rows, c).cpu().numpy()
    res["one_euro_bits_equal_host"] = bool(np.array_equal(got.view(np.uint32), host.view(np.uint32)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sequences", type=int, default=300)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    from implementation_phd_lab_vision_amd import sequences, smooth, train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "op": time_ops(a.sequences, a.rows, a.iters, a.rounds, a.warmup)}
    d, nb = 1024, 2
    head = PHDFor3DJoints(d, 17, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(d, 17, nb, seed=0))
    head.to(dev).eval()
    store = DenseStore(a.clips, T, dev)
    post = smooth.PostProcess(kind="gauss", fix_bones=True)
    passes = {"post_off": lambda: sequences.evaluate_dense(head, store, fuse="context"),
              "post_on": lambda: sequences.evaluate_dense(head, store, fuse="context", post=post)}
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
    on = res["post_on"]
    out["pass"] = {"clips": a.clips, "frames": on["frames_all"], "sequences": on["sequences"], "post": on["post"],
                   "evaluate_dense_post_off_ms": ms["post_off"], "evaluate_dense_post_on_ms": ms["post_on"],
                   "accel_all_mm": [round(float(on["accel_all"]) * 1e3, 3), round(float(on["post_accel_all"]) * 1e3, 3)],
                   "bone_std_mm_raw_post_gt": [round(float(on["bone_std_" + k + "_all"]), 5) for k in ("raw", "post", "gt")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
