"""The rows of tests/test_multiview_guard_bands_gpu.py late on a side stream, with the harness of tests/test_stream_order_gpu.py: each
row runs once plainly on the default stream and once on the side stream while its inputs are still stale; snapshot bits == final bits ==
plain bits, no defined output holds the poison, and neither op holds the host."""
import pytest

from tests.test_multiview_guard_bands_gpu import ROWS_MULTIVIEW
from tests.test_stream_order_gpu import run_row_late

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_MULTIVIEW, ids=[r.id for r in ROWS_MULTIVIEW])
def test_late_on_a_side_stream_multiview(row):
    run_row_late(row)
