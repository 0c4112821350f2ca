"""The op of include/r50_track.h between poisoned guard bands, with the harness of tests/guard_bands.py on the rows of tests/rows/track.py: each row runs plain,
between 0xFF bands and between 0x7B bands from the same payloads; both outputs hold the same bits in the three runs and every band of
every operand (the byte buffer, the table and both outputs) is intact.  The rows: the ragged table of tests/track_reference.py (7
images of different sizes at byte offsets of every residue mod 4; the last image ends the buffer 1, 2 or 3 bytes past a dword boundary
and its box ends at the last byte, so the byte-wise tail read runs right in front of the back band), both modes, out 8 and 224, with
and without ``out_flip``.

tests/test_track_cpu.py holds this table complete for the header, as tests/test_guard_bands_cpu.py does for include/r50.h."""
import pytest

from tests.guard_bands import run_row
from tests.rows.track import ROWS_TRACK

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ROWS_TRACK, ids=[r.id for r in ROWS_TRACK])
def test_track_ops(row):
    run_row(row)
