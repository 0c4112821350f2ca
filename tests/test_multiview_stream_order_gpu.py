"""The rows of tests/rows/multiview.py late on a side stream, with the harness of tests/stream_order.py: each
row runs once plainly on the default stream and once on the side stream while its inputs are still stale; snapshot bits == final bits ==
plain bits, no defined output holds the poison, and neither op holds the host."""
import pytest

from tests.rows.multiview import ROWS_MULTIVIEW
from tests.stream_order import run_row_late

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_MULTIVIEW, ids=[r.id for r in ROWS_MULTIVIEW])
def test_late_on_a_side_stream_multiview(row):
    run_row_late(row)
