"""The rows of tests/rows/resample.py late on a side stream, with the harness of tests/stream_order.py: each row
runs once plainly on the default stream and once on the side stream while its poses and its tables are still stale; snapshot bits ==
final bits == plain bits, and the op does not hold the host."""
import pytest

from tests.rows.resample import ROWS_RESAMPLE
from tests.stream_order import run_row_late

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_RESAMPLE, ids=[r.id for r in ROWS_RESAMPLE])
def test_late_on_a_side_stream_resample(row):
    run_row_late(row)
