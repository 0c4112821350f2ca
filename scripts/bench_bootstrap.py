"""The stratified cluster bootstrap (INTEGRATION.md section AC) on one MI355X.  Every timing runs in a fresh child process of a tree:

* ``ops``: ``r50_op_bootstrap_sums`` at --reps 10000 replicates and M 22 columns for U = 240 units (15 strata of 16: sequence units) and
  U = 110,000 (15 strata of 7,333 or 7,334: clip units), beside (1) the torch composition in chunks of replicates -- per stratum
  ``torch.randint`` + ``index_select`` + a sum over the stratum's draws, the chunk sized so that its gathered rows stay under --torch-mb
  megabytes; other draws and another order of the sum, so not the op's bits -- and (2) a device copy of ``v``, for scale.  The forms
  alternate in rounds of --iters launches, each round under a host clock that ends in a synchronise; per form the best round and all
  rounds (the spread) are reported.
* ``pass``: one ``protocols.evaluate_protocols`` pass over a synthetic store of --clips clips (scripts/bench_dense.py's), PHD(1024, 17, 2)
  fp16 -- what ``results --protocols`` runs -- and ``bootstrap.evaluate_bootstrap`` with --reps replicates over the same store (what
  ``--bootstrap 10000`` adds: a pass of its own per model, the sequence-unit and the clip-unit bootstrap); with ``--parent-tree DIR`` (a
  built checkout of the parent commit) also the plain pass there: this tree and the parent alternate, --passes children each.  That last
  pair is the proof that the default path did not move.
Prints one JSON line.
    python scripts/bench_bootstrap.py [--iters 5] [--rounds 5] [--reps 10000] [--clips 1024] [--passes 3] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
M = 22
STRATA = 15


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


def _torch_form(v, start, reps, chunk, gen):
    """(R, G, M): per chunk of replicates and per stratum, n_g uniform draws a replicate, the drawn rows gathered and summed."""
    out = torch.empty((reps, len(start) - 1, v.shape[1]), dtype=torch.float64, device=v.device)
    for r in range(0, reps, chunk):
        c = min(chunk, reps - r)
        for g in range(len(start) - 1):
            a, b = int(start[g]), int(start[g + 1])
            idx = torch.randint(a, b, (c * (b - a),), device=v.device, generator=gen)
            out[r:r + c, g] = v.index_select(0, idx).view(c, b - a, -1).sum(dim=1)
    return out


def child_ops(a):
    from implementation_phd_lab_vision_amd import bootstrap as bs
    res = {"replicates": a.reps, "columns": M, "strata": STRATA}
    gen = torch.Generator(device=DEV).manual_seed(0)
    for name, units in (("U240", 240), ("U110000", 110000)):
        sizes = [units // STRATA + (1 if g < units % STRATA else 0) for g in range(STRATA)]
        table = bs.UnitTable.from_sizes(sizes)
        v = torch.rand((units, M), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(DEV)
        start = table.stratum_start.tolist()
        chunk = max(1, min(a.reps, (a.torch_mb << 20) // (max(sizes) * M * 8)))
        copy_dst = torch.empty_like(v)
        forms = {"op": lambda: bs.bootstrap_sums(v, table, a.reps, 0),
                 "torch_randint_index_select_sum": lambda: _torch_form(v, start, a.reps, chunk, gen),
                 "device_copy_of_v": lambda: copy_dst.copy_(v)}
        first = bs.bootstrap_sums(v, table, 64, 0)
        cut = torch.cat([bs.bootstrap_sums(v, table, 24, 0), bs.bootstrap_sums(v, table, 40, 0, r0=24, window=1024)])
        one = _rounds(forms, a.iters, a.rounds, a.warmup)
        one.update({"units": units, "largest_stratum": max(sizes), "torch_chunk_replicates": chunk, "bytes_v": units * M * 8,
                    "bytes_out": a.reps * STRATA * M * 8, "multiply_adds": a.reps * units * M,
                    "chunked_launches_bit_equal": bool(torch.equal(first, cut)),
                    "mean_of_op_and_torch_sums": [float(forms["op"]().mean()), float(forms["torch_randint_index_select_sum"]().mean())]})
        res[name] = one
    return res


def child_pass(a):
    from implementation_phd_lab_vision_amd import _lib, protocols, train                 # the tree's package first: bench_dense extends sys.path
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    sys.path.insert(0, os.path.join(a.tree, "scripts"))
    from bench_dense import DenseStore, T
    head = PHDFor3DJoints(1024, 17, 2, precision="fp16")
    head.load_state_dict(train.default_state_dict(1024, 17, 2, seed=0))
    head.to(DEV).eval()
    store = DenseStore(a.clips, T, DEV)
    names, ids = protocols.action_groups(store.item_actions())
    if a.bootstrap:
        from implementation_phd_lab_vision_amd import bootstrap as bs

        def run():
            return bs.evaluate_bootstrap(head, store, None, a.bootstrap, "sequence", 0, 0.95)
    else:
        def run():
            return protocols.evaluate_protocols(head, store, ids, names)
    run()
    ms = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    out = {"ms": ms, "clips": a.clips, "library": str(_lib.LIB_PATH)}
    if a.bootstrap:
        out.update({"units": int(res["units"].sum()), "strata": len(res["units"]), "design_effect": res["design_effect"],
                    "all_p1_mm_point_lo_hi": [round(float(res[k][0, 0]) * 1e3, 3) for k in ("point", "lo", "hi")]})
    else:
        out["all_p1_mm"] = round(float(res["recon_all"][0]) * 1e3, 3)
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10000)
    ap.add_argument("--torch-mb", type=int, default=1024, help="the torch composition's gathered rows per chunk, megabytes")
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed passes per child, after one warm-up")
    ap.add_argument("--parent-tree", type=str, default=None)
    ap.add_argument("--tree", type=str, default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--child", choices=("ops", "pass"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--bootstrap", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.tree)
        print(json.dumps(child_ops(a) if a.child == "ops" else child_pass(a)))
        return
    common = ["--clips", str(a.clips), "--repeats", str(a.repeats)]
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "ops": spawn(HERE, "--child", "ops", "--iters", str(a.iters), "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--reps",
                        str(a.reps), "--torch-mb", str(a.torch_mb)),
           "pass": {"clips": a.clips, "bootstrap": [], "plain": [], "parent_plain": []}}
    for _ in range(a.passes):
        out["pass"]["bootstrap"].append(spawn(HERE, "--child", "pass", "--bootstrap", str(a.reps), *common))
        out["pass"]["plain"].append(spawn(HERE, "--child", "pass", *common))
        if a.parent_tree:
            out["pass"]["parent_plain"].append(spawn(os.path.abspath(a.parent_tree), "--child", "pass", *common))
    if not a.parent_tree:
        out["pass"]["parent_plain"] = "not measured (no --parent-tree)"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
