"""The ops of include/r50_hal.h between poisoned guard bands, with the harness of tests/test_guard_bands_gpu.py: each row runs plain,
between 0xFF bands and between 0x7B bands from the same payloads; ``dh`` and ``loss_lat`` hold the same bits in the three runs, every
band of every operand (``row_part`` included, a workspace) is intact, and no element of ``dh`` is left at the fill.

tests/test_hal_cpu.py holds this table complete for the header, as tests/test_guard_bands_cpu.py does for include/r50.h."""
import functools

import pytest
import torch

from tests import guard_bands as G
from tests.test_guard_bands_gpu import Arena, Row, run_row  # noqa: F401  (Arena: the type ``launch`` receives)

pytestmark = pytest.mark.gpu
F32 = torch.float32
ET = {0: torch.bfloat16, 1: torch.float16}

ROWS_HAL = []


@functools.lru_cache(maxsize=None)
def _lib():
    from implementation_phd_lab_vision_amd import _lib as L
    L.build_library()
    return L.load_library()


def _rn(seed, shape, dtype, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _hal_make(rows, d, et):
    return (_rn(d, (rows, d), ET[et]), _rn(d + 1, (rows, d), ET[et]), _rn(d + 2, (rows, d), F32, 1.0 / (rows * d)))


def _hal_launch(a, pay, rows, d, lam, ls, et):
    # A workgroup finds its row as blockIdx.x * d and a lane moves 16 bytes of h / phi / dh and 32 of dh_reg per trip; a wrong row or a
    # wrong last trip lands within one row of the widest operand: one row of dh_reg, d * 4 bytes.
    reach = d * 4
    assert G.BAND >= 2 * reach
    a.reach(reach)
    h, phi, dh_reg = pay
    rc = _lib().r50_op_hal_latent_grad(a.inp("h", h).data_ptr(), a.inp("phi", phi).data_ptr(), a.inp("dh_reg", dh_reg).data_ptr(), rows, d,
                                       lam, ls, a.out("dh", (rows, d), ET[et]).data_ptr(), a.out("loss_lat", (1,), F32).data_ptr(),
                                       a.ws("row_part", (rows,), F32).data_ptr(), et, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib().r50_last_error(None)


for _et in (1, 0):
    for _rows, _d, _lam, _ls in ((5, 1032, 2.5, 1024.0), (3, 64, 1.0, 1.0)):       # 129 vectors: one lane's second trip; 8 of 128 lanes
        ROWS_HAL.append(Row("hal", f"hal_latent_grad-{'fp16' if _et else 'bf16'}-r{_rows}d{_d}", ("r50_op_hal_latent_grad",),
                            functools.partial(_hal_make, _rows, _d, _et),
                            functools.partial(_hal_launch, rows=_rows, d=_d, lam=_lam, ls=_ls, et=_et)))


@pytest.mark.parametrize("row", ROWS_HAL, ids=[r.id for r in ROWS_HAL])
def test_hal_ops(row):
    run_row(row)
