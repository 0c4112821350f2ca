"""The ops of include/r50_hal.h between poisoned guard bands, with the harness of tests/guard_bands.py on the rows of tests/rows/hal.py: each row runs plain,
between 0xFF bands and between 0x7B bands from the same payloads; ``dh`` and ``loss_lat`` hold the same bits in the three runs, every
band of every operand (``row_part`` included, a workspace) is intact, and no element of ``dh`` is left at the fill.

tests/test_hal_cpu.py holds this table complete for the header, as tests/test_guard_bands_cpu.py does for include/r50.h."""
import pytest

from tests.guard_bands import run_row
from tests.rows.hal import ROWS_HAL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_HAL, ids=[r.id for r in ROWS_HAL])
def test_hal_ops(row):
    run_row(row)
