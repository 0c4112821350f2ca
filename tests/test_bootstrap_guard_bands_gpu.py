"""The op of include/r50_bootstrap.h between poisoned guard bands, with the harness of tests/guard_bands.py on the rows of tests/rows/bootstrap.py: each row runs plain,
between 0xFF bands and between 0x7B bands from the same payloads; both outputs hold the same bits in the three runs, every band of every
operand (the unit rows, the stratum table and both outputs) is intact, and no output element is left at the fill.  The rows: strata of 1,
5 and 70 units (a Philox block straddles two strata, the first and the last unit row are read right at both ends of ``v``), ``window`` 16 so
that the 70-stratum takes five passes with a short last one, ``counts`` given and NULL, M 7 and 300 (two column chunks, the second short).

tests/test_bootstrap_cpu.py holds this table complete for the header, as tests/test_guard_bands_cpu.py does for include/r50.h."""
import pytest

from tests.guard_bands import run_row
from tests.rows.bootstrap import ROWS_BOOTSTRAP

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_BOOTSTRAP, ids=[r.id for r in ROWS_BOOTSTRAP])
def test_bootstrap_ops(row):
    run_row(row)
