"""The op of include/r50_resample.h between poisoned guard bands, with the harness of tests/guard_bands.py on the rows of tests/rows/resample.py: each row runs plain,
between 0xFF bands and between 0x7B bands from the same payloads; both outputs hold the same bits in the three runs, every band of every
operand (the poses, the four index tables and both outputs) is intact, and no output element is left at the fill.  The rows: the ragged
table of tests/resample_reference.py (sequences of 1 to 130 rows, times on knots, inside bridged intervals and breaks, before the first
and after the last stamp of the first and of the last sequence, so the stencil's i-1 and i+2 are asked for right at both ends of the
poses), both kinds, J 17, 1 and 64.

tests/test_resample_cpu.py holds this table complete for the header, as tests/test_guard_bands_cpu.py does for include/r50.h."""
import pytest

from tests.guard_bands import run_row
from tests.rows.resample import ROWS_RESAMPLE

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_RESAMPLE, ids=[r.id for r in ROWS_RESAMPLE])
def test_resample_ops(row):
    run_row(row)
