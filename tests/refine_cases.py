"""The ragged case of tests/test_refine_gpu.py, which the rows of tests/rows/refine.py run as well: computed once and shared."""
import functools

from tests import refine_reference as RR


SEEDS = {17: 1, 3: 2, 64: 3}


@functools.lru_cache(maxsize=None)
def _case(joints, with_conf):
    """The ragged case, computed once and shared (never modified)."""
    return RR.ragged_case(SEEDS[joints], joints, with_conf)
