"""The rows of tests/test_track_guard_bands_gpu.py late on a side stream, with the harness of tests/test_stream_order_gpu.py: each row
runs once plainly on the default stream and once on the side stream while its byte buffer and its table are still stale; snapshot bits
== final bits == plain bits, and the op does not hold the host."""
import pytest

from tests.test_stream_order_gpu import run_row_late
from tests.test_track_guard_bands_gpu import ROWS_TRACK

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_TRACK, ids=[r.id for r in ROWS_TRACK])
def test_late_on_a_side_stream_track(row):
    run_row_late(row)
