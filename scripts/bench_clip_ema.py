"""Global-norm gradient clipping and EMA weights on the MI355X.  One JSON line:
(i)  the tail of a step on phase 1's flat buffer at PHD(1024, 17, 2) (16.9 M fp32 parameters), between device events, in alternating
     rounds in one process (per round the median over ``--launches`` calls; the best round and the median round are reported):
       floor        r50_op_check_finite + r50_op_adamw                                    (what a step without the features runs)
       fused_clip   r50_op_grad_norm + r50_op_adamw_clip_ema(clip)
       fused_ema    r50_op_check_finite + r50_op_adamw_clip_ema(ema)
       fused_both   r50_op_grad_norm + r50_op_adamw_clip_ema(clip, ema)
       naive_clip   r50_op_check_finite, torch.linalg.vector_norm, the coefficient in torch ops, g.mul_, r50_op_adamw
       naive_both   naive_clip + torch._foreach_lerp_
     Before any timing the fused tail's bits are compared with the composition's on the same inputs (the composition fed the op's own
     coefficient: torch's fp32 norm differs from the fp64 one in the last bits), and torch's own norm and lerp are compared with the ops'.
(ii) one phase-1 step (HIP graph, as scripts/bench_head_train.py runs it) and one k = 25 rollout step (eager, as
     scripts/bench_rollout_train.py runs it) at B 32 and B 256, fp16, dropout on, with the features off / clip / EMA / both on ONE head
     per kind (the features are attributes of the optimizer), in alternating rounds on a synchronised host clock.
    python scripts/bench_clip_ema.py [--batches 32 256] [--launches 50] [--rounds 5] [--steps 5]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HYPER = (1e-4, 0.9, 0.999, 1e-8, 1e-2)
MAX_NORM, EMA_W = 1.0, 1e-3


def event_ms(fn, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(torch.tensor(out).median())


class Tail:
    """The buffers of one optimizer tail over ``n`` parameters and the six programs on them."""

    def __init__(self, n, dev, seed=0):
        from implementation_phd_lab_vision_amd import _lib
        self._lib, self.lib, self.n = _lib, _lib.load_library(), n
        g = torch.Generator().manual_seed(seed)
        self.p = (torch.randn(n, generator=g) * 0.02).to(dev)
        self.m, self.v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.g = (torch.randn(n, generator=g) * 1e-3).to(dev)
        self.p16 = self.p.half()
        self.ema = self.p.clone()
        self.found = torch.zeros(1, dtype=torch.int32, device=dev)
        self.part = torch.zeros(2048, dtype=torch.float64, device=dev)
        self.clip2 = torch.ones(2, device=dev)
        self.stats4 = torch.zeros(4, dtype=torch.float64, device=dev)
        self.step = 0
        self.stream = torch.cuda.current_stream().cuda_stream

    def state(self):
        return {k: getattr(self, k).clone() for k in ("p", "m", "v", "p16", "ema", "g")}

    def load(self, state, step=0):
        for k, t in state.items():
            getattr(self, k).copy_(t)
        self.step = step

    def check_finite(self):
        self._lib.check(self.lib.r50_op_check_finite(self.g.data_ptr(), self.n, self.found.data_ptr(), self.stream), None, "r50_op_check_finite")

    def grad_norm(self):
        self._lib.check(self.lib.r50_op_grad_norm(self.g.data_ptr(), self.n, MAX_NORM, self.part.data_ptr(), self.part.numel(),
                                                  self.found.data_ptr(), self.clip2.data_ptr(), self.stats4.data_ptr(), self.stream), None,
                        "r50_op_grad_norm")

    def adamw(self):
        self.step += 1
        self._lib.check(self.lib.r50_op_adamw(self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.g.data_ptr(), self.p16.data_ptr(),
                                              self.n, *HYPER, self.step, self.found.data_ptr(), 1, self.stream), None, "r50_op_adamw")

    def adamw_clip_ema(self, clip, ema):
        self.step += 1
        self._lib.check(self.lib.r50_op_adamw_clip_ema(self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.g.data_ptr(),
                                                       self.p16.data_ptr(), self.n, *HYPER, self.step, self.found.data_ptr(),
                                                       self.clip2.data_ptr() if clip else None, self.ema.data_ptr() if ema else None, EMA_W, 1,
                                                       self.stream), None, "r50_op_adamw_clip_ema")

    def torch_clip(self, coef=None):
        """torch.nn.utils.clip_grad_norm_'s device program on the flat buffer (no host read); ``coef``: use this one instead."""
        norm = torch.linalg.vector_norm(self.g)
        c = torch.clamp(MAX_NORM / (norm + 1e-6), max=1.0) if coef is None else coef
        self.g.mul_(c)
        return norm

    def programs(self):
        return {"floor": lambda: (self.check_finite(), self.adamw()),
                "fused_clip": lambda: (self.grad_norm(), self.adamw_clip_ema(True, False)),
                "fused_ema": lambda: (self.check_finite(), self.adamw_clip_ema(False, True)),
                "fused_both": lambda: (self.grad_norm(), self.adamw_clip_ema(True, True)),
                "naive_clip": lambda: (self.check_finite(), self.torch_clip(), self.adamw()),
                "naive_both": lambda: (self.check_finite(), self.torch_clip(), self.adamw(),
                                       torch._foreach_lerp_([self.ema], [self.p], EMA_W))}


def compare_bits(tail):
    """Two steps of fused_both against the composition of existing pieces on the same inputs; returns what agreed."""
    start = tail.state()
    start["g"] = start["g"] * (300.0 / float(torch.linalg.vector_norm(start["g"])))     # norm 300: clipped at MAX_NORM 1
    tail.load(start)
    coefs = []
    for _ in range(2):
        tail.grad_norm(); tail.adamw_clip_ema(True, True)
        coefs.append(tail.clip2.clone())
    fused = tail.state()
    tail.load(start)
    w = torch.tensor(EMA_W, dtype=torch.float32, device=tail.ema.device)
    for s in range(2):
        tail.g.copy_(start["g"])
        tail.check_finite()
        tail.g.mul_(coefs[s][0])                                   # the op's own coefficient
        tail.adamw()
        tail.ema.copy_(tail.ema + w * (tail.p - tail.ema))
    comp = tail.state()
    out = {"coef": float(coefs[0][0]), "norm": float(coefs[0][1]),
           "bits_equal": {k: bool(torch.equal(fused[k], comp[k])) for k in ("p", "m", "v", "p16", "ema")}}
    torch_norm = float(torch.linalg.vector_norm(start["g"]))
    out["torch_fp32_norm_rel_diff"] = abs(torch_norm - out["norm"]) / out["norm"]
    tail.load(start)                                               # torch's own lerp against the op's EMA
    tail.grad_norm(); tail.adamw_clip_ema(True, True)
    e_t = start["ema"].clone()
    torch._foreach_lerp_([e_t], [tail.p], EMA_W)
    out["foreach_lerp_max_abs_diff"] = float((tail.ema - e_t).abs().max())
    torch.cuda.synchronize()
    return out


def bench_tail(a, dev, n):
    tail = Tail(n, dev)
    agree = compare_bits(tail)
    tail.load(Tail(n, dev).state())
    progs = tail.programs()
    for fn in progs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in progs}
    for _ in range(a.rounds):
        for k, fn in progs.items():
            rounds[k].append(event_ms(fn, a.launches))
    best = {k: min(v) for k, v in rounds.items()}
    mid = {k: float(torch.tensor(v).median()) for k, v in rounds.items()}
    return {"n": n, "agreement": agree, "best_round_ms": best, "median_round_ms": mid, "rounds_ms": rounds,
            "ratios_best": {"fused_clip_over_floor": best["fused_clip"] / best["floor"], "fused_ema_over_floor": best["fused_ema"] / best["floor"],
                            "fused_both_over_floor": best["fused_both"] / best["floor"],
                            "fused_clip_over_naive_clip": best["fused_clip"] / best["naive_clip"],
                            "fused_both_over_naive_both": best["fused_both"] / best["naive_both"]},
            "bytes_per_param": {"floor": 4 + 30, "fused_clip": 4 + 30, "fused_ema": 4 + 38, "fused_both": 4 + 38,
                                "naive_clip": 4 + 4 + 8 + 30, "naive_both": 4 + 4 + 8 + 30 + 12}}


VARIANTS = ("off", "clip", "ema", "both")


def bench_steps(a, dev):
    from implementation_phd_lab_vision_amd import train, train_ar
    from implementation_phd_lab_vision_amd.trainable import WeightEMA
    sd = train.default_state_dict(1024, 17, 2, seed=0)
    kinds = {}
    for kind, cls in (("phase1", train.TrainableHead), ("rollout_k25", train_ar.ARTrainableHead)):
        h = cls(1024, 17, 2, precision="fp16")
        h.load_state_dict(sd); h.to(dev).train()
        if kind == "phase1":
            h.enable_graphs(True)
        optim = train.AdamW(h, lr=1e-4)
        kinds[kind] = (h, optim, train.GradScaler(init_scale=1024.0), WeightEMA(h, 0.999))
    out = {}
    for b in a.batches:
        g = torch.Generator().manual_seed(100 + b)
        feats = torch.randn(b, 40, 2048, generator=g).abs().to(dev)
        gt = (torch.randn(b, 40, 17, 3, generator=g) * 0.5).to(dev)

        def step(kind, variant):
            h, optim, scaler, ema = kinds[kind]
            optim.max_grad_norm = MAX_NORM if variant in ("clip", "both") else None
            optim.ema = ema if variant in ("ema", "both") else None
            if kind == "phase1":
                return h.train_step(feats, gt, optim, scaler)[2]
            return h.rollout_train_step(feats, gt, 15, 25, optim, scaler)[2]

        row = {}
        for kind in kinds:
            for v in VARIANTS:
                for _ in range(a.warmup):
                    step(kind, v)
            ms, skipped = {v: [] for v in VARIANTS}, {v: 0 for v in VARIANTS}
            for _ in range(a.rounds):
                for v in VARIANTS:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        skipped[v] += step(kind, v)
                    torch.cuda.synchronize()
                    ms[v].append((time.perf_counter() - t0) * 1e3 / a.steps)
            best = {v: min(x) for v, x in ms.items()}
            row[kind] = {"ms_per_step_rounds": ms, "best_ms": best, "median_ms": {v: float(torch.tensor(x).median()) for v, x in ms.items()},
                         "added_ms_best": {v: best[v] - best["off"] for v in VARIANTS[1:]}, "skipped": skipped,
                         "clip_stats": kinds[kind][0].clip_stats(), "trainable_params": int(kinds[kind][0].flat_master.numel())}
        out[str(b)] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_ema.py measures on an MI355X; there is nothing to time without one")
    from implementation_phd_lab_vision_amd import train
    from implementation_phd_lab_vision_amd.trainable import flat_layout
    from implementation_phd_lab_vision_amd.model import expected_keys
    dev = "cuda:0"
    layout = flat_layout(train.phase1_items(2), expected_keys(1024, 17, 2))
    n = layout[-1][1] + int(torch.Size(layout[-1][2]).numel())
    result = {"workload": "clip + EMA: the optimizer tail on phase 1's flat buffer, and phase-1 / rollout k 25 steps, PHD(1024,17,2), fp16",
              "device": torch.cuda.get_device_name(0), "launches": a.launches, "rounds": a.rounds, "steps_per_round": a.steps,
              "tail": bench_tail(a, dev, n), "steps": bench_steps(a, dev)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
