"""The ops of include/r50_smooth.h between poisoned guard bands, with the harness of tests/guard_bands.py on the rows of tests/rows/smooth.py: each row runs
plain, between 0xFF bands and between 0x7B bands from the same payloads; every output holds the same bits in the three runs, every band
of every operand (index tables and the FIR table included) is intact, and no output element is left at the fill.

tests/test_smooth_cpu.py holds this table complete for the header, as tests/test_guard_bands_cpu.py does for include/r50.h."""
import pytest

from tests.guard_bands import run_row
from tests.rows.smooth import ROWS_SMOOTH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_SMOOTH, ids=[r.id for r in ROWS_SMOOTH])
def test_smooth_ops(row):
    run_row(row)
