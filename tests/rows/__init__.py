"""The row catalogue: every op of include/r50*.h as a ``Row`` (tests/guard_bands.py), one table module per header, and the one list
of the tables.  tests/test_alignment_gpu.py and tests/test_repeatability_gpu.py run ``ALL_ROWS``; ``run_row`` (tests/guard_bands.py) and
``run_row_late`` (tests/stream_order.py) run a table from its header's own test files.  A new header adds one module here and one line
to ``TABLES``, at the end: the order of tables and of rows is part of the tests' parametrisation."""
from tests.rows.bootstrap import ROWS_BOOTSTRAP
from tests.rows.frames_domain import ROWS_FRAMES_DOMAIN
from tests.rows.hal import ROWS_HAL
from tests.rows.kinematics import ROWS_KINEMATICS
from tests.rows.multiview import ROWS_MULTIVIEW
from tests.rows.r50 import ROWS
from tests.rows.refine import ROWS_REFINE
from tests.rows.resample import ROWS_RESAMPLE
from tests.rows.smooth import ROWS_SMOOTH
from tests.rows.track import ROWS_TRACK

TABLES = (("r50", ROWS), ("hal", ROWS_HAL), ("smooth", ROWS_SMOOTH), ("track", ROWS_TRACK), ("multiview", ROWS_MULTIVIEW),
          ("resample", ROWS_RESAMPLE), ("bootstrap", ROWS_BOOTSTRAP), ("refine", ROWS_REFINE), ("kinematics", ROWS_KINEMATICS),
          ("frames_domain", ROWS_FRAMES_DOMAIN))
ALL_ROWS = [row for _name, table in TABLES for row in table]
assert len({row.id for row in ALL_ROWS}) == len(ALL_ROWS), "row ids must be unique over the tables"
