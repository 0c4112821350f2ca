"""The rows of tests/test_resample_guard_bands_gpu.py late on a side stream, with the harness of tests/test_stream_order_gpu.py: each row
runs once plainly on the default stream and once on the side stream while its poses and its tables are still stale; snapshot bits ==
final bits == plain bits, and the op does not hold the host."""
import pytest

from tests.test_resample_guard_bands_gpu import ROWS_RESAMPLE
from tests.test_stream_order_gpu import run_row_late

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_RESAMPLE, ids=[r.id for r in ROWS_RESAMPLE])
def test_late_on_a_side_stream_resample(row):
    run_row_late(row)
