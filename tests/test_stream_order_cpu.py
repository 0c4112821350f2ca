"""tests/test_stream_order_gpu.py runs every row of the tables ``r50``, ``smooth`` and ``hal`` of tests/rows/ late on a side stream: held complete here, without a GPU,
as tests/test_guard_bands_cpu.py holds the guard-band table complete for the header."""
import torch

from tests import guard_bands as G


def _parametrised_rows(T):
    """The rows the table tests of tests/test_stream_order_gpu.py are parametrised with, by test name."""
    out = {}
    for name, fn in vars(T).items():
        if not name.startswith("test_late_on_a_side_stream_"):
            continue
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        assert len(marks) == 1 and marks[0].args[0] == "row", name
        rows, ids = list(marks[0].args[1]), list(marks[0].kwargs["ids"])
        assert ids == [r.id for r in rows], f"{name}: the ids are not the guard-band tests' ids"
        out[name] = rows
    return out


def test_every_guard_band_row_runs_late_on_a_side_stream():
    from tests import test_stream_order_gpu as T
    from tests.rows.hal import ROWS_HAL
    from tests.rows.r50 import ROWS
    from tests.rows.smooth import ROWS_SMOOTH
    tables = ROWS + ROWS_SMOOTH + ROWS_HAL
    assert len(tables) > 150 and ROWS_SMOOTH and ROWS_HAL
    by_test = _parametrised_rows(T)
    run = [r for rows in by_test.values() for r in rows]
    assert len(run) == len(tables) and all(any(r is t for t in tables) for r in run), "the parametrisation is not built from the three row tables"
    missing = [t.id for t in tables if not any(t is r for r in run)]
    assert not missing, f"rows that never run late on a side stream: {missing}"
    ids = [r.id for r in run]
    assert len(ids) == len(set(ids)), "row ids must be unique across the three tables"
    for name, rows in by_test.items():
        assert rows and {r.family for r in rows} == {name[len("test_late_on_a_side_stream_"):]}, f"{name} is not one family"
        assert getattr(T, name).__name__ == name
    assert set(T.FAMILIES) == {r.family for r in tables}


def test_the_blocking_table_names_rows_or_ops_and_keeps_off_the_hot_paths():
    from tests import stream_order as SO
    from tests import test_stream_order_gpu as T
    SO.check_blocking_table(T.ALL_ROWS)
    hot = SO.hot_path_ops()
    assert {"r50_op_cast_rows", "r50_op_conv2d", "r50_op_conv2d_f16", "r50_op_gn_relu_causal3", "r50_op_bneck_tail", "r50_op_bneck_block2",
            "r50_op_avgpool", "r50_forward"} <= hot
    ops = {op for row in T.ALL_ROWS for op in row.ops}
    assert hot <= ops, f"hot-path ops without a row: {sorted(hot - ops)}"
    assert "r50_op_resize_frames_u8" in SO.BLOCKS_HOST and "r50_op_stem" in SO.BLOCKS_HOST       # they synchronise: read r50_abi.hip


def test_stale_values_of_every_operand_type():
    """``stale_like``, ``restale_`` and ``poisoned`` on the CPU: NaN in every float format (e4m3 included), 255 as uint8, and 0 -- in
    range -- for the index types; shape and dtype kept; ``restale_`` writes in place."""
    from tests import stream_order as SO
    floats = (torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.float8_e4m3fn)
    for dtype in floats + (torch.uint8, torch.int32, torch.int64):
        src = torch.arange(1, 13).view(3, 4).to(torch.float32).to(dtype)
        stale, work = SO.stale_like(src, device="cpu"), src.clone()
        SO.restale_(work)
        for t in (stale, work):
            assert t.shape == src.shape and t.dtype == dtype and t.is_contiguous()
            if dtype in floats:
                assert bool(torch.isnan(t.to(torch.float64)).all()) and G.holds_fill(t, G.FILL_NAN) == t.numel()
            elif dtype == torch.uint8:
                assert bool((t == 255).all())
            else:
                assert bool((t == 0).all()), "a stale index must stay in range"
        out = SO.poisoned((2, 5), dtype, device="cpu")
        assert out.shape == (2, 5) and out.dtype == dtype and G.holds_fill(out, G.FILL_NAN) == 10
    assert int(SO.poisoned((1,), torch.int32, device="cpu")) == -1          # outputs are poison, not stale: 0xFF as guarded_empty fills them
    row, ms = SO.MEASURED_SLOWEST_ROW
    assert 4 * ms <= SO.SLEEP_MS <= 200.0, f"the sleep of {SO.SLEEP_MS} ms must be four times the slowest row's enqueue time ({row}: {ms} ms), 200 ms at most"


def test_assert_same_bits_sees_nan_payloads_signed_zero_and_shapes():
    import pytest
    from tests import stream_order as SO
    a = torch.tensor([0.0, 1.0, float("nan")])
    SO.assert_same_bits("toy", "x", "snapshot", a.clone(), a)
    with pytest.raises(AssertionError, match=r"toy: the final tensor of `x`.*differs.*in 1 of 3 elements, the first at flat index 0"):
        SO.assert_same_bits("toy", "x", "final tensor", torch.tensor([-0.0, 1.0, float("nan")]), a)
    with pytest.raises(AssertionError, match=r"the snapshot of `x` on the side stream is \(2,\)"):
        SO.assert_same_bits("toy", "x", "snapshot", a[:2], a)
