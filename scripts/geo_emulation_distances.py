"""Distances of the 16-bit storage emulation (tests/geo_reference.py with store16, fp64, loss scale 1024, eval mode) from
tests/golden/geo_golden.pt's step-level cases, on the CPU: the numbers behind the tolerances of tests/test_geo_gpu.py and the table
of INTEGRATION.md section N.  Per precision and case: the largest relative loss error, gradient-norm error, 64-entry gradient-slice
error over the parameters, and of the two-step parameter update the largest error median / lr, relative error and error max / lr.

    python scripts/geo_emulation_distances.py
"""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import geo_reference as gr  # noqa: E402
from tests.golden.make_golden_geo import LAMBDAS, geo_batches_for, geo_state_dict  # noqa: E402


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def distances(c, edges, joint, precision):
    sd = geo_state_dict(c["latent_dim"], c["number_blocks"], c["seed"])
    losses, grads, final = gr.geo_steps_reference(sd, c["trainable"], geo_batches_for(c["seed"], c["b"], c["t"]), edges, LAMBDAS, joint=joint,
                                                  lr=c["lr"], dtype=torch.float64, store16=precision, loss_scale=1024.0)
    d = [0.0] * 6
    for s in range(2):
        for got, want in zip(losses[s], c["losses"][s]):
            d[0] = max(d[0], abs(got - want) / abs(want))
    for i, n in enumerate(c["trainable"]):
        k = c["head_len"][i]
        d[1] = max(d[1], abs(float(grads[n].norm()) - c["grad_norm"][i]) / c["grad_norm"][i])
        d[2] = max(d[2], _rel(grads[n].reshape(-1)[:k], c["grad_head"][i][:k]))
        want = c["param_head"][i][:k].double() - sd[n].reshape(-1)[:k].double()
        got = final[n].reshape(-1)[:k].double() - sd[n].reshape(-1)[:k].double()
        err = (got - want).abs()
        d[3] = max(d[3], float(err.median()) / c["lr"])
        d[4] = max(d[4], _rel(got, want))
        d[5] = max(d[5], float(err.max()) / c["lr"])
    return d


def main():
    gold = torch.load(ROOT / "tests" / "golden" / "geo_golden.pt", map_location="cpu", weights_only=True)
    edges = [tuple(e) for e in gold["edges"]]
    out = {}
    for precision in ("fp16", "bf16"):
        out[precision] = {"phase1": [distances(c, edges, None, precision) for c in gold["steps"]],
                          "joint": [distances(c, edges, (c["lambda_future"], c["lambda_latent"]), precision) for c in gold["joint_steps"]]}
    print(json.dumps(out))
    for precision, stages in out.items():
        for stage, cases in stages.items():
            for i, d in enumerate(cases):
                print(f"{precision} {stage} {i} | " + "  ".join(f"{v:.3g}" for v in d))


if __name__ == "__main__":
    main()
