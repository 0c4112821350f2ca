"""The guard-band rows of include/r50_hal.h: ``ROWS_HAL`` (tests/test_hal_guard_bands_gpu.py says what they cover)."""
import functools

import torch

from tests import guard_bands as G
from tests.guard_bands import BF, F32, HF, Row, lib

ET = {0: BF, 1: HF}

ROWS_HAL = []


def _rn(seed, shape, dtype, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _hal_make(rows, d, et):
    return (_rn(d, (rows, d), ET[et]), _rn(d + 1, (rows, d), ET[et]), _rn(d + 2, (rows, d), F32, 1.0 / (rows * d)))


def _hal_launch(a, pay, rows, d, lam, ls, et):
    # A workgroup finds its row as blockIdx.x * d and a lane moves 16 bytes of h / phi / dh and 32 of dh_reg per trip; a wrong row or a
    # wrong last trip lands within one row of the widest operand: one row of dh_reg, d * 4 bytes.
    reach = d * 4
    assert G.BAND >= 2 * reach, f"guard band of {G.BAND} bytes is less than twice the reach {reach}"
    a.reach(reach)
    h, phi, dh_reg = pay
    rc = lib().r50_op_hal_latent_grad(a.inp("h", h).data_ptr(), a.inp("phi", phi).data_ptr(), a.inp("dh_reg", dh_reg).data_ptr(), rows, d,
                                       lam, ls, a.out("dh", (rows, d), ET[et]).data_ptr(), a.out("loss_lat", (1,), F32).data_ptr(),
                                       a.ws("row_part", (rows,), F32).data_ptr(), et, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().r50_last_error(None)


for _et in (1, 0):
    for _rows, _d, _lam, _ls in ((5, 1032, 2.5, 1024.0), (3, 64, 1.0, 1.0)):       # 129 vectors: one lane's second trip; 8 of 128 lanes
        ROWS_HAL.append(Row("hal", f"hal_latent_grad-{'fp16' if _et else 'bf16'}-r{_rows}d{_d}", ("r50_op_hal_latent_grad",),
                            functools.partial(_hal_make, _rows, _d, _et),
                            functools.partial(_hal_launch, rows=_rows, d=_d, lam=_lam, ls=_ls, et=_et)))
