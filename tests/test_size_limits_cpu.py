"""The size-limit table of tests/size_limits.py against the header it restates -- no device needed.  The GPU half, which runs every case
at n_max and one step beyond, is tests/test_size_limits_gpu.py."""
import re

import pytest

from tests import alignment as A
from tests import size_limits as S

HEADER = (A.ROOT / "include" / "r50.h").read_text()


def test_every_entry_point_has_a_case():
    protos = A.prototypes()
    covered = {c.op for c in S.CASES}
    for fn in S.ENTRY_POINTS:
        assert fn in protos, f"{fn} is not declared in include/r50.h"
        assert fn in covered, f"{fn} has no size case"
    assert covered <= set(S.ENTRY_POINTS), f"cases of entry points the list does not name: {sorted(covered - set(S.ENTRY_POINTS))}"
    assert len({c.id for c in S.CASES}) == len(S.CASES), "case ids repeat"
    # every bneck_tail form of the header, and each (op, shape) refused once
    assert {c.shape for c in S.CASES if c.family == "tail"} == {(64, 64, False), (64, 128, False), (64, 64, True), (128, 128, False),
                                                               (256, 256, False), (256, 0, False)}
    for c in S.CASES:
        if not c.beyond and c.limited_by != "cap":
            assert any(o.beyond and (o.op, o.shape) == (c.op, c.shape) for o in S.CASES), f"{c.id}: nothing refuses its shape"


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_n_max_is_exactly_at_the_edge(case):
    terms = case.terms()
    n = case.n_max
    assert n >= 1 and S.rule(terms, n), f"{case.id}: the rule fails at n_max = {n}: {[(t.name, t.value(n), t.bound) for t in terms]}"
    assert not S.rule(terms, n + 1), f"{case.id}: the rule still holds at n_max + 1 = {n + 1}"
    assert all(t.holds(n) == (t.value(n) < t.bound) and isinstance(t.value(n), int) for t in terms)
    if case.id in S.EXPECTED_N_MAX:
        assert n == S.EXPECTED_N_MAX[case.id], f"{case.id}: n_max {n}, the table says {S.EXPECTED_N_MAX[case.id]}"
    failing = S.decisive(terms)
    if case.limited_by == "cap":
        # the stated limit cannot be reached: the run crosses 2^31 elements and 2^32 bytes instead, and all of it fits the memory cap
        assert case.n_run is not None and case.n_run < n and not case.beyond
        per_image = {"maxpool": 112 * 112 * 64, "avgpool": 49 * 2048, "stem": 112 * 112 * 64}[case.family]
        assert (case.n_run - 1) * per_image < S.P31 <= case.n_run * per_image and case.n_run * per_image * 2 >= 1 << 32
        total = {"maxpool": 112 * 112 * 64 * 2 + 56 * 56 * 64 * 2, "avgpool": 49 * 2048 * 2 + 2048 * 4,
                 "stem": 3 * 224 * 224 * 4 + 230 * 232 * 8 + 112 * 112 * 64 * 2}[case.family] * case.n_run
        assert total < S.MEMORY_CAP * 15 // 16, f"{case.id}: {total} bytes of operands"
    elif case.limited_by == "x_back":
        # the back reach of a padded tap is what tips it: one more image would fit without it
        x = next(t for t in terms if t.name == "x")
        assert failing == ["x"] and x.c > 0 and x.a * (n + 1) < x.bound
    else:
        assert case.limited_by in failing, f"{case.id}: limited by {failing}, the case says {case.limited_by}"
        assert case.n_run is None


def test_x_back_admits_one_image_fewer_than_the_1x1_twin():
    h, w, cin, cout = 7, 7, 512, 512
    assert S.n_max(S.conv_terms(h, w, cin, cout, 3, 1, 1)) == 42798
    assert S.n_max(S.conv_terms(h, w, cin, cout, 1, 1, 0)) == 42799


def test_split_admits_half_the_images():
    assert S.n_max(S.conv_terms(56, 56, 64, 64, 1, 1, 0, "r50_op_conv2d_split")) == S.n_max(S.conv_terms(56, 56, 64, 64, 1, 1, 0)) // 2


@pytest.mark.parametrize("fn", S.ENTRY_POINTS)
def test_header_states_a_limit(fn):
    text = S.comment_blocks(fn, HEADER)
    assert "Size limits" in text, f"{fn}: no limits sentence in its comment"
    assert re.search(r"2\^3[01]", text), f"{fn}: its comment names no 2^31 / 2^30 bound"
    if "Size limits, r50_op_" in text:            # one comment over several prototypes: each is named
        assert f"Size limits, {fn}" in text, f"{fn}: the shared comment has no limits sentence of its own"


def test_comment_blocks_finds_the_right_comment():
    assert "MaxPool2d" in S.comment_blocks("r50_op_maxpool", HEADER) and "Stem:" not in S.comment_blocks("r50_op_maxpool", HEADER)
    assert "Stem:" in S.comment_blocks("r50_op_stem", HEADER)
    assert "r50_op_conv2d_split:" in S.comment_blocks("r50_op_conv2d_split", HEADER)
