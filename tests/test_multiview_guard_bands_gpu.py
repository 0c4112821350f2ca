"""The ops of include/r50_multiview.h between poisoned guard bands, with the harness of tests/guard_bands.py on the rows of tests/rows/multiview.py: each row runs
plain, between 0xFF bands and between 0x7B bands from the same payloads; every output holds the same bits in the three runs, every band
of every operand (the index tables and the fit table included) is intact, and no output element is left at the fill.

tests/test_multiview_cpu.py holds this table complete for the header, as tests/test_guard_bands_cpu.py does for include/r50.h."""
import pytest

from tests.guard_bands import run_row
from tests.rows.multiview import ROWS_MULTIVIEW

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_MULTIVIEW, ids=[r.id for r in ROWS_MULTIVIEW])
def test_multiview_ops(row):
    run_row(row)
