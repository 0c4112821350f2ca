"""Resampling of pose sequences (INTEGRATION.md section AB) on one MI355X.  Every timing runs in a fresh child process of a tree:

* ``ops``: ``r50_op_resample_sequences`` at the test split's size -- --sequences 300 sequences of --rows 1000 rows, J 17, upsampled by 2
  (a time on every stamp and on every midpoint: 1999 output rows a sequence) -- linear and cubic, beside (1) torch's form of the linear
  case, two ``index_select`` and one ``lerp`` in fp32 (three launches, two gathered temporaries; not the op's fp64 bits), and (2) a device
  copy of the output's bytes, the floor of anything that writes them.  The forms alternate in rounds of --iters launches, each round
  under a host clock that ends in a synchronise; per form the best round and all rounds (the spread) are reported.
* ``pass``: one ``sequences.evaluate_dense`` pass over a synthetic store of --clips clips (scripts/bench_dense.py's), PHD(1024, 17, 2)
  fp16, without the holdout and with ``resample.evaluate_holdout(K = 2)`` after it (what ``results --dense --dense-holdout 2`` adds); with
  ``--parent-tree DIR`` (a built checkout of the parent commit) also the plain pass there: this tree and the parent alternate, --passes
  children each.  That last pair is the proof that the default path did not move.
Prints one JSON line.
    python scripts/bench_resample.py [--iters 20] [--rounds 5] [--clips 1024] [--passes 3] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = 17
DEV = "cuda:0"


def _rounds(forms, iters, rounds, warmup):
    us = {name: [] for name in forms}
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    for _ in range(rounds):                                                              # alternate, so drift hits all alike
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / iters)
    return {name: {"best_us": round(min(v), 2), "rounds_us": [round(x, 2) for x in v]} for name, v in us.items()}


def child_ops(a):
    from implementation_phd_lab_vision_amd import resample
    n_seq, rows = a.sequences, a.rows
    f = n_seq * rows
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(J, 3, generator=g) * 0.25 + torch.tensor([0.0, 0.0, 5.0]) +
         torch.cumsum(torch.randn(n_seq, rows, J, 3, generator=g) * 0.002, dim=1)).reshape(f, J, 3).contiguous().to(DEV)
    seq_start = (np.arange(n_seq + 1) * rows).astype(np.int32)
    idx = np.tile(np.arange(rows, dtype=np.int32), n_seq)
    tau, seq = resample.uniform_times(seq_start, idx, 0.5, 1)
    table = resample.ResampleTable(seq_start, idx, tau, seq)
    left = torch.from_numpy(table.out_left.astype(np.int64)).to(DEV)
    right = torch.from_numpy(np.minimum(table.out_left.astype(np.int64) + 1, seq_start[table.out_seq + 1] - 1)).to(DEV)
    u = torch.from_numpy((tau - idx[table.out_left]).astype(np.float32)).to(DEV)[:, None, None]
    y_l, _ = resample.resample_sequences(x, table, "linear", 1)
    copy_dst = torch.empty_like(y_l)
    forms = {
        "op_linear": lambda: resample.resample_sequences(x, table, "linear", 1),
        "op_cubic": lambda: resample.resample_sequences(x, table, "cubic", 1),
        "torch_index_select_lerp_fp32": lambda: torch.lerp(x.index_select(0, left), x.index_select(0, right), u),
        "device_copy_of_the_output": lambda: copy_dst.copy_(y_l),
    }
    diff = float((forms["torch_index_select_lerp_fp32"]() - y_l).abs().max())
    res = _rounds(forms, a.iters, a.rounds, a.warmup)
    res.update({"sequences": n_seq, "rows_per_sequence": rows, "rows": f, "output_rows": table.outputs, "joints": J,
                "bytes_x": f * J * 3 * 4, "bytes_y": table.outputs * J * 3 * 4, "max_abs_diff_linear_op_vs_torch_fp32": diff})
    return res


def child_pass(a):
    from implementation_phd_lab_vision_amd import _lib, sequences, train            # the tree's package first: bench_dense extends sys.path
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    sys.path.insert(0, os.path.join(a.tree, "scripts"))
    from bench_dense import DenseStore, T
    head = PHDFor3DJoints(1024, 17, 2, precision="fp16")
    head.load_state_dict(train.default_state_dict(1024, 17, 2, seed=0))
    head.to(DEV).eval()
    store = DenseStore(a.clips, T, DEV)
    if a.holdout:
        from implementation_phd_lab_vision_amd import resample

        def run():
            dense = sequences.evaluate_dense(head, store, fuse="context", keep_poses=True)
            return dense, resample.evaluate_holdout(dense, a.holdout, "cubic", DEV)
    else:
        def run():
            return sequences.evaluate_dense(head, store, fuse="context"), None
    run()
    ms = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dense, held = run()
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    out = {"ms": ms, "frames": int(dense["frames_all"]), "sequences": int(dense["sequences"]), "library": str(_lib.LIB_PATH)}
    if held is not None:
        out.update({"held_out_rows": int(held["holdout_rows_all"]), "flagged": held["holdout_flagged"].tolist(),
                    "p1_mm_held_out_full_interpolated": [round(float(held["holdout_full_p1_all"]) * 1e3, 3),
                                                         round(float(held["holdout_p1_all"]) * 1e3, 3)]})
    return out


def spawn(tree, *args):
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, *args]
    done = subprocess.run(cmd, capture_output=True, text=True, cwd=tree)
    if done.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({done.returncode}):\n{done.stdout}\n{done.stderr}")
    print(f"{tree}: {' '.join(args)}: done", file=sys.stderr, flush=True)
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sequences", type=int, default=300)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed passes per child, after one warm-up")
    ap.add_argument("--parent-tree", type=str, default=None)
    ap.add_argument("--tree", type=str, default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--child", choices=("ops", "pass"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--holdout", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.tree)
        print(json.dumps(child_ops(a) if a.child == "ops" else child_pass(a)))
        return
    common = ["--clips", str(a.clips), "--repeats", str(a.repeats)]
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "ops": spawn(HERE, "--child", "ops", "--iters", str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--sequences",
                        str(a.sequences), "--rows", str(a.rows)),
           "pass": {"clips": a.clips, "holdout_2": [], "plain": [], "parent_plain": []}}
    for _ in range(a.passes):
        out["pass"]["holdout_2"].append(spawn(HERE, "--child", "pass", "--holdout", "2", *common))
        out["pass"]["plain"].append(spawn(HERE, "--child", "pass", *common))
        if a.parent_tree:
            out["pass"]["parent_plain"].append(spawn(os.path.abspath(a.parent_tree), "--child", "pass", *common))
    if not a.parent_tree:
        out["pass"]["parent_plain"] = "not measured (no --parent-tree)"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
