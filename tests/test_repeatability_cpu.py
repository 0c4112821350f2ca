"""tests/repeatability.py without a GPU: the hot set is the set the source shows, every hot kernel has a row, and the comparator and the
overlap rule say what they should.

The scan reads csrc/*.h as source text and looks for our own synchronisation idiom in our own C++ (a raw workgroup barrier builtin, a
wait count in an asm statement or through ``wait_vmcnt``, a sleep builtin): a new hand-synchronised kernel cannot arrive without joining
``HAND_SYNCED``, and so the hot rows of tests/test_repeatability_gpu.py.
"""
import re

import pytest
import torch

from tests import repeatability as RP


def test_the_scan_finds_exactly_the_hand_synced_kernels():
    found = RP.scan_hand_synced()
    want = set(RP.HAND_SYNCED) - set(RP.SYNCTHREADS_PIPELINES)
    assert set(found) == want, (f"hand-synchronised kernels in csrc/*.h without an entry in HAND_SYNCED: {sorted(set(found) - want)}; "
                                f"entries of HAND_SYNCED that the source no longer shows: {sorted(want - set(found))}")
    for three in ("igemm_bf16_kernel", "igemm_ws_kernel", "gemm8p_kernel"):
        assert three in found
    assert "wait_vmcnt" in found["conv3x3_xres_kernel"], "a wait through the __device__ helper wait_vmcnt must count"
    assert {"G8_BARRIER", "G8_LGKM"} <= set(found["gemm8p_kernel"]), "a barrier or wait through a macro must count"
    assert "__builtin_amdgcn_s_sleep" in found["bneck_catchain_kernel"]
    assert "draw_skeletons_u8_kernel" not in found          # __syncthreads() only: the compiler places its waits


def test_the_pipelines_listed_by_hand_are_what_the_list_says():
    kernels = RP.global_kernels()
    assert len(kernels) >= 90, f"the scan found {len(kernels)} __global__ kernels"
    for name, reason in RP.SYNCTHREADS_PIPELINES.items():
        assert name in RP.HAND_SYNCED and reason.strip()
        assert name in kernels, f"SYNCTHREADS_PIPELINES names {name}, which csrc/*.h does not define"
        assert "__syncthreads" in kernels[name] and not RP.HAND_PLACED.search(kernels[name]), \
            f"{name} no longer synchronises with __syncthreads() alone: move it out of SYNCTHREADS_PIPELINES"
    assert set(RP.HAND_SYNCED) <= set(kernels)


def test_every_hand_synced_kernel_is_reached_by_a_row():
    from tests import alignment as AL
    from tests.rows import ALL_ROWS
    protos = AL.prototypes()
    for kernel, entry_points in RP.HAND_SYNCED.items():
        assert entry_points, f"{kernel}: no entry point"
        for ep in entry_points:
            assert ep in protos, f"{kernel}: {ep} is no entry point of include/r50*.h"
    for op in RP.ALSO_HOT:
        assert op in protos and op not in {e for eps in RP.HAND_SYNCED.values() for e in eps}
    reached = RP.kernels_reached(ALL_ROWS)
    assert all(reached.values()), f"hand-synchronised kernels that no row of ALL_ROWS reaches: {sorted(k for k, v in reached.items() if not v)}"
    for must in ("r50_op_conv2d", "r50_op_conv2d_f16", "r50_op_conv2d_w2", "r50_op_conv2d_split", "r50_op_conv2d_fp8", "r50_op_conv1x1_cat",
                 "r50_op_bneck_tail", "r50_op_bneck_block1", "r50_op_bneck_block1_ds", "r50_op_bneck_block2", "r50_op_bneck_cat_chain",
                 "r50_op_stem", "r50_op_nn_search", "r50_forward", "r50_forward_u8"):
        assert must in RP.hot_ops()
    hot = [r for r in ALL_ROWS if RP.is_hot(r)]
    assert 0 < len(hot) < len(ALL_ROWS) and RP.MEASURED_SLOWEST_ROW[0] in {r.id for r in hot}
    assert not any(RP.is_hot(r) for r in ALL_ROWS if r.family in ("head", "losses", "frames"))


def test_the_scan_on_toy_sources(tmp_path):
    src = tmp_path / "toy.h"
    src.write_text("""
// s_barrier in a comment does not count
__device__ __forceinline__ void settle(int n) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ int twice(int v) { return 2 * v; }
__device__ void outer(int n) { settle(n); }
#define STEP_BARRIER() { __builtin_amdgcn_s_barrier(); }
#define FENCE() __builtin_amdgcn_sched_barrier(0)
template <int N>
__global__ __launch_bounds__(N * 64) void direct_kernel(const float* x) { __builtin_amdgcn_s_barrier(); }
__global__ void through_helper_kernel(float* y) { y[0] = twice(1); outer(3); }
__global__ void through_macro_kernel(float* y) { STEP_BARRIER() }
__global__ void sleeping_kernel(int* p) { while (!*p) __builtin_amdgcn_s_sleep(2); }
__global__ void plain_kernel(float* y) { __syncthreads(); FENCE(); /* s_waitcnt */ __builtin_amdgcn_wave_barrier(); y[0] = twice(2); }
__global__ void declared_only_kernel(float* y);
""")
    found = RP.scan_hand_synced([src])
    assert set(found) == {"direct_kernel", "through_helper_kernel", "through_macro_kernel", "sleeping_kernel"}, found
    assert found["through_helper_kernel"] == ["outer"] and found["through_macro_kernel"] == ["STEP_BARRIER"]
    assert set(RP.global_kernels([src])) == set(found) | {"plain_kernel"}


def test_the_comparator_names_image_row_col_channel():
    shape = (3, 5, 7, 64)
    assert RP.unravel(0, shape) == (0, 0, 0, 0)
    assert RP.unravel(63, shape) == (0, 0, 0, 63)
    assert RP.unravel(64, shape) == (0, 0, 1, 0)
    assert RP.unravel(7 * 64, shape) == (0, 1, 0, 0)
    assert RP.unravel(5 * 7 * 64, shape) == (1, 0, 0, 0)
    assert RP.unravel(3 * 5 * 7 * 64 - 1, shape) == (2, 4, 6, 63)
    for flat in (1, 449, 2240, 6000):
        n, h, w, c = RP.unravel(flat, shape)
        assert ((n * 5 + h) * 7 + w) * 64 + c == flat
    with pytest.raises(AssertionError):
        RP.unravel(3 * 5 * 7 * 64, shape)
    want = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    assert RP.describe_difference(want.clone(), want) is None
    got = want.clone()
    got[1, 2, 3, 4] = -got[1, 2, 3, 4] if float(got[1, 2, 3, 4]) != 0 else 1.0
    got[2, 4, 6, 63] += 1.0
    first, last = ((1 * 5 + 2) * 7 + 3) * 64 + 4, 3 * 5 * 7 * 64 - 1
    with pytest.raises(AssertionError) as e:
        RP.assert_same_bits("row", "y", "noise_mem repetition 7", got, want)
    msg = str(e.value)
    assert "`y` of noise_mem repetition 7" in msg and f"in 2 of {want.numel()} elements" in msg
    assert f"flat indices {first} .. {last}" in msg and "(image, row, col, channel) = (1, 2, 3, 4)" in msg
    # integer views: -0 against +0 and two NaN payloads differ; a 2-D operand gets plain coordinates
    z = torch.zeros((2, 3))
    assert "coordinates (1, 2)" in RP.describe_difference(torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, -0.0]]), z)
    nan_a = torch.tensor([0x7FC00000], dtype=torch.int32).view(torch.float32)
    nan_b = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    assert RP.describe_difference(nan_a, nan_a.clone()) is None and RP.describe_difference(nan_a, nan_b) is not None
    assert "is (2, 3)" in RP.describe_difference(z, torch.zeros((3, 2)))


def test_the_overlap_rule_on_synthetic_event_times():
    assert RP.overlapped(op_end_ms=1.0, noise_end_ms=4.0)
    assert not RP.overlapped(op_end_ms=4.0, noise_end_ms=1.0)
    assert not RP.overlapped(op_end_ms=2.0, noise_end_ms=2.0)          # the burst must end AFTER the row
    assert not RP.overlapped(op_end_ms=-0.1, noise_end_ms=2.0)         # a row that ended before the noise began did not wait for it
    assert RP.intervals_intersect((0.0, 1.0), (0.5, 2.0)) and RP.intervals_intersect((0.5, 2.0), (0.0, 1.0))
    assert RP.intervals_intersect((0.0, 3.0), (1.0, 2.0))
    assert not RP.intervals_intersect((0.0, 1.0), (1.0, 2.0)) and not RP.intervals_intersect((0.0, 1.0), (1.5, 2.0))
    assert RP.enough_overlap([True] * 16) and RP.enough_overlap([True] * 12 + [False] * 4)
    assert not RP.enough_overlap([True] * 11 + [False] * 5), "more than a quarter did not overlap: the row has not been tested"
    assert RP.enough_overlap([True, True, True, False]) and not RP.enough_overlap([True, True, False, False])
    assert not RP.enough_overlap([]) and not RP.enough_overlap([False])
    assert RP.R_HOT >= 16 and RP.BURST_FACTOR >= 4 and RP.NOISE_MEM_BYTES >= 4 * (256 << 20)
    assert RP.MODES == ("quiet", "noise_mem", "noise_mfma", "twin")


def test_the_harness_touches_no_gpu_at_import_and_sets_nothing():
    text = (RP.ROOT / "tests" / "repeatability.py").read_text() + (RP.ROOT / "tests" / "test_repeatability_gpu.py").read_text()
    assert not re.search(r"os\.environ|putenv|graph\(|CUDAGraph|hipGraph", text), "no environment variable is set and nothing is captured"
