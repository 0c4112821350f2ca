"""The rows of tests/rows/track.py late on a side stream, with the harness of tests/stream_order.py: each row
runs once plainly on the default stream and once on the side stream while its byte buffer and its table are still stale; snapshot bits
== final bits == plain bits, and the op does not hold the host."""
import pytest

from tests.rows.track import ROWS_TRACK
from tests.stream_order import run_row_late

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_TRACK, ids=[r.id for r in ROWS_TRACK])
def test_late_on_a_side_stream_track(row):
    run_row_late(row)
