"""Distances of the 16-bit storage emulation of the hallucinator step (tests/hal_reference.py train_hal_steps_emulated: fp64, loss
scale 1024) from its fp32 restatement, on the CPU, for the cases of tests/test_hal_gpu.py::test_train_steps_equal_the_restatement: the
numbers behind the bars of that test that are not phase 1's, and the table of INTEGRATION.md section V.  Per precision and case, the
largest over the two steps and the four parameters of: relative loss error, relative gradient-norm error, relative error of the
64-entry gradient slice, and of the parameter update the error median / lr, the relative error and the error max / lr.

    python scripts/hal_emulation_distances.py
"""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import hal_reference as HR  # noqa: E402


def main():
    out = {}
    for b, t in HR.STEP_CASES:
        sd, batches = HR.step_case_state(b)
        want = HR.train_hal_steps_reference(sd, batches, lr=HR.STEP_LR, lambda_latent=HR.STEP_LAMBDA, dtype=torch.float32)
        for precision in ("fp16", "bf16"):
            got = HR.train_hal_steps_emulated(sd, batches, precision, lr=HR.STEP_LR, lambda_latent=HR.STEP_LAMBDA,
                                              loss_scale=HR.STEP_LOSS_SCALE)
            out[f"{precision} B{b} T{t}"] = HR.step_distances(got, want, sd, HR.STEP_LR)
    print(json.dumps(out))
    for name, d in out.items():
        print(f"{name} | " + "  ".join(f"{k} {v:.3g}" for k, v in d.items()))


if __name__ == "__main__":
    main()
