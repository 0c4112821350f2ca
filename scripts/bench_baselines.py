"""Forecast baselines on one MI355X.  Three things, in one process:

* ``r50_op_nn_search`` at nq 256, d 1024, fp16, k 1 and 8, n in --sizes (default 10^4, 10^5, 3 10^5), beside the torch composition it
  replaces on the same operands: ``x_norm2 - 2 q @ x^T`` (``torch.mm`` over database chunks that keep the distance matrix under 1 GB)
  and ``torch.topk`` (per chunk, then over the chunks' candidates).  The two alternate round by round after a warm-up of both; device
  events around each call; the median, minimum and maximum over --rounds rounds.  The op's result is first compared with the
  composition's (the share of equal index lists: fp32 sums in another order may swap near ties);
* the op's database bytes over its time as TB/s: the target is one HBM read of the database per call;
* one ``baselines.evaluate_baselines`` pass (all three baselines, k 1) beside one ``protocols.evaluate_protocols`` pass (I 15 / P 25)
  over the same synthetic store of --clips clips resident on the device, PHD(1024, 17, 2) fp16, and the ``StripDatabase.build`` time
  over --db-clips clips (host clock, synchronised, --passes passes after one warm-up pass).
Prints one JSON line.
    python scripts/bench_baselines.py [--rounds 20] [--sizes 10000 100000 300000] [--clips 1024] [--db-clips 4096] [--passes 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_protocols import GROUPS, SyntheticStore  # noqa: E402

I_LEN, P_LEN, JOINTS, NQ, D = 15, 25, 17, 256, 1024
MATRIX_BYTES = 1 << 30


class Store(SyntheticStore):
    """... plus the item -> row map ``StripDatabase.build`` reads."""

    def __init__(self, n, t, dev, seed=0):
        super().__init__(n, t, dev, seed)
        self._row = torch.arange(n, dtype=torch.long, device=dev)


def composition(q, x, xn, k):
    """The torch form: per database chunk the (NQ, chunk) fp32 scores and their top k, then the top k of the chunks' candidates."""
    step = max(MATRIX_BYTES // (4 * q.shape[0]), 1)
    qf = q.float()
    vals, idxs = [], []
    for s in range(0, x.shape[0], step):
        sc = torch.addmm(xn[s:s + step][None, :].expand(q.shape[0], -1), qf, x[s:s + step].float().t(), alpha=-2.0)
        v, i = torch.topk(sc, min(k, sc.shape[1]), dim=1, largest=False)
        vals.append(v)
        idxs.append(i + s)
    v, pos = torch.topk(torch.cat(vals, dim=1), k, dim=1, largest=False)
    return torch.cat(idxs, dim=1).gather(1, pos), v


def composition16(q, x, xn, k):
    """The same with the 16-bit ``torch.mm`` (fp32 accumulation inside, a 16-bit (NQ, chunk) product): the cheaper composition."""
    step = max(MATRIX_BYTES // (4 * q.shape[0]), 1)
    vals, idxs = [], []
    for s in range(0, x.shape[0], step):
        sc = xn[s:s + step][None, :] - 2.0 * torch.mm(q, x[s:s + step].t()).float()
        v, i = torch.topk(sc, min(k, sc.shape[1]), dim=1, largest=False)
        vals.append(v)
        idxs.append(i + s)
    v, pos = torch.topk(torch.cat(vals, dim=1), k, dim=1, largest=False)
    return torch.cat(idxs, dim=1).gather(1, pos), v


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3


def stats(us):
    return {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}


def time_search(n, k, rounds, warmup):
    from implementation_phd_lab_vision_amd import baselines
    dev = "cuda:0"
    g = torch.Generator().manual_seed(n + k)
    x = torch.randn(n, D, generator=g).to(torch.float16).to(dev)
    q = torch.randn(NQ, D, generator=g).to(torch.float16).to(dev)
    xn = baselines.row_norm2(x)
    arms = {"op": lambda: baselines.nn_search(q, x, xn, k), "torch_fp32": lambda: composition(q, x, xn, k),
            "torch_16bit": lambda: composition16(q, x, xn, k)}
    idx = arms["op"]()[0].long()
    same = {name: round(float((arms[name]()[0] == idx).all(dim=1).float().mean()), 4) for name in ("torch_fp32", "torch_16bit")}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in arms}
    for _ in range(rounds):                                    # alternating rounds in one process
        for name, fn in arms.items():
            us[name].append(timed(fn))
    op = statistics.median(us["op"])
    return {"n": n, "k": k, "nq": NQ, "d": D, "us": {name: stats(v) for name, v in us.items()}, "equal_index_lists": same,
            "database_mb": round(n * D * 2 / 1e6, 1), "op_database_tb_per_s": round(n * D * 2 / (op * 1e-6) / 1e12, 3),
            "op_tflops": round(2.0 * NQ * n * D / (op * 1e-6) / 1e12, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 300_000])
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--db-clips", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be >= 5: the reported time is a median")
    from implementation_phd_lab_vision_amd import baselines, protocols, train
    from implementation_phd_lab_vision_amd.model import PHDFor3DJoints
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "search": [time_search(n, k, a.rounds, a.warmup) for n in a.sizes for k in (1, 8)]}
    nb = 2
    head = PHDFor3DJoints(D, JOINTS, nb, precision="fp16")
    head.load_state_dict(train.default_state_dict(D, JOINTS, nb, seed=0))
    head.to(dev).eval()
    store, train_store = Store(a.clips, I_LEN + P_LEN, dev), Store(a.db_clips, I_LEN + P_LEN, dev, seed=5)
    ids = [i % GROUPS for i in range(a.clips)]
    names = [f"action{g:02d}" for g in range(GROUPS)]
    db = [None]

    def build():
        db[0] = baselines.StripDatabase.build(head, train_store, I_LEN)
        return db[0]

    passes = {}
    for name, fn in (("strip_database_build", build),
                     ("evaluate_baselines", lambda: baselines.evaluate_baselines(head, store, db[0], ids, names, I_LEN, P_LEN)),
                     ("evaluate_protocols", lambda: protocols.evaluate_protocols(head, store, ids, names, I_LEN, P_LEN))):
        fn()
        ms = []
        for _ in range(a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        passes[name] = {"ms_per_pass": ms}
        if name == "evaluate_baselines":
            passes[name]["p1_mean_mm"] = {n: round(float(res[n]["p1"].mean()) * 1e3, 2) for n in res["names"]}
    out["passes"] = {"clips": a.clips, "db_clips": a.db_clips, "batch_size": 256, "input_len": I_LEN, "pred_len": P_LEN, "latent_dim": D,
                     "precision": "fp16", **passes}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
