"""Multi-view fusion without a GPU: the fourth public header include/r50_multiview.h is bound, exported and
guard-banded; every refusal of its ops returns before any launch; ``ViewTable`` on hand-written sequences against the plain loops of
tests/multiview_reference.py; the restatement itself on an exact rigid transform; the extrinsics-error helper; and the parser."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import multiview_reference as MR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "r50_multiview.h"
OPS = {"r50_op_view_rigid_fit", "r50_op_view_fuse"}


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = re.findall(r"^\s*(?:int|int64_t|size_t)\s+(r50_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    assert protos, "no prototypes parsed from include/r50_multiview.h"
    return [(name, len([a for a in args.split(",") if a.strip()])) for name, args in protos]


def test_every_prototype_of_the_multiview_header_is_bound_exported_and_guard_banded(lib_built):
    from implementation_phd_lab_vision_amd import _lib
    from tests.rows import multiview as T
    protos = _prototypes()
    names = [n for n, _ in protos]
    assert set(names) == OPS == set(_lib._SIGNATURES_MULTIVIEW) and len(names) == len(set(names))
    assert set(re.findall(r"\b(r50_op_[a-z0-9_]+)\s*\(", HEADER.read_text())) == OPS, "a name in a comment is a prototype too"
    covered = set()
    for row in T.ROWS_MULTIVIEW:
        covered.update(row.ops)
    assert covered == OPS
    others = [(ROOT / "include" / h).read_text() for h in ("r50.h", "r50_hal.h", "r50_smooth.h")]
    for name, arity in protos:
        assert len(_lib._SIGNATURES_MULTIVIEW[name][1]) == arity, name
        assert hasattr(lib_built, name), f"{name} declared in r50_multiview.h but not exported by libr50hip.so"
        assert getattr(lib_built, name).argtypes == _lib._SIGNATURES_MULTIVIEW[name][1]
        assert name not in _lib._SIGNATURES and name not in _lib.EXPORTED_SYMBOLS and name not in _lib._SIGNATURES_HAL and \
            name not in _lib._SIGNATURES_SMOOTH
        assert not any(name in text for text in others)
    ids = [row.id for row in T.ROWS_MULTIVIEW]
    assert len(ids) == len(set(ids))
    assert "r50_multiview.h" in (ROOT / "implementation_phd_lab_vision_amd" / "_lib.py").read_text().split("def _source_digest")[1].split("def ")[0]


def test_every_refusal_returns_before_any_launch(lib_built):
    """No device is needed: each call is refused on its arguments, with the op's name in the message.  The pointers are made-up
    addresses that nothing dereferences."""
    y, x, ps, mt, fit, out, dis, t1, t2, t3 = 0x10000, 0x90000, 0x110000, 0x120000, 0x130000, 0x140000, 0x150000, 0x160000, 0x170000, 0x180000
    n_bytes = 12 * 5 * 3 * 4                                                         # F = 12 rows of J = 5

    def refused(name, rc, why):
        assert rc != 0, (name, why)
        assert name.encode() in lib_built.r50_last_error(None), (name, why)

    rf = lib_built.r50_op_view_rigid_fit
    ok = dict(y=y, x=x, ry=12, rx=12, J=5, ps=ps, mt=mt, P=2, fit=fit)
    for kw in (dict(y=None), dict(x=None), dict(ps=None), dict(mt=None), dict(fit=None), dict(ry=0), dict(rx=0), dict(ry=-1), dict(ry=2 ** 31),
               dict(rx=2 ** 31), dict(J=0), dict(J=65), dict(J=-3), dict(P=0), dict(P=-1)):
        a = dict(ok, **kw)
        refused("r50_op_view_rigid_fit", rf(a["y"], a["x"], a["ry"], a["rx"], a["J"], a["ps"], a["mt"], a["P"], a["fit"], None), kw)

    fu = lib_built.r50_op_view_fuse
    ok = dict(pose=y, F=12, J=5, pstart=t1, prow=t2, pfit=t3, fit=fit, P=2, mode=0, fused=out, dis=dis)
    for kw in (dict(pose=None), dict(pstart=None), dict(prow=None), dict(pfit=None), dict(fit=None), dict(fused=None), dict(dis=None), dict(F=0),
               dict(F=-1), dict(F=2 ** 31), dict(J=0), dict(J=65), dict(P=-1), dict(mode=-1), dict(mode=3), dict(fused=y),
               dict(fused=y + n_bytes - 4), dict(fused=y - n_bytes + 4)):
        a = dict(ok, **kw)
        refused("r50_op_view_fuse", fu(a["pose"], a["F"], a["J"], a["pstart"], a["prow"], a["pfit"], a["fit"], a["P"], a["mode"], a["fused"],
                                       a["dis"], None), kw)


def _sequences(spec):
    """spec: [(key, [frame indices])] -> (seq_keys, seq_start, frame_idx)."""
    keys = [k for k, _ in spec]
    seq_start = np.concatenate([[0], np.cumsum([len(fr) for _, fr in spec])]).astype(np.int32)
    return keys, seq_start, np.concatenate([np.asarray(fr, dtype=np.int32) for _, fr in spec])


def _same_as_the_loops(table, spec, cams=None, dropped=()):
    keys, seq_start, frame_idx = _sequences(spec)
    want = MR.view_table(keys, seq_start, frame_idx, cams, dropped=dropped)
    assert table.pairs == len(want["pairs"]) and table.take_keys == want["take_keys"]
    for p, (take, src, dst, rows) in enumerate(want["pairs"]):
        assert (int(table.pair_take[p]), int(table.pair_src[p]), int(table.pair_dst[p])) == (take, src, dst)
        assert table.match[table.pair_start[p]:table.pair_start[p + 1]].tolist() == [list(r) for r in rows]
    for r, peers in enumerate(want["peers"]):
        got = list(zip(table.peer_row[table.peer_start[r]:table.peer_start[r + 1]].tolist(),
                       table.peer_fit[table.peer_start[r]:table.peer_start[r + 1]].tolist()))
        assert got == peers, r
    for a in (table.pair_start, table.match, table.pair_src, table.pair_dst, table.pair_take, table.peer_start, table.peer_row, table.peer_fit):
        assert a.dtype == np.int32
    return want


def test_view_table_on_hand_written_sequences():
    from implementation_phd_lab_vision_amd.multiview import ViewTable
    # one camera: no pair, no peer
    spec = [((9, "walk", 1), [0, 1, 2])]
    t = ViewTable.from_sequences(*_sequences(spec))
    assert t.pairs == 0 and t.match.shape == (0, 2) and t.views().tolist() == [1, 1, 1] and t.pair_start.tolist() == [0]
    _same_as_the_loops(t, spec)
    # two cameras of unequal length, a gap in frame_idx: frames 3, 4 only in camera 1, frame 7 only in camera 2
    spec = [((9, "walk", 1), [0, 1, 2, 3, 4, 6]), ((9, "walk", 2), [1, 2, 6, 7])]
    t = ViewTable.from_sequences(*_sequences(spec))
    assert t.pairs == 2 and t.pair_dst.tolist() == [0, 1] and t.pair_src.tolist() == [1, 0] and t.pair_take.tolist() == [0, 0]
    assert t.match[:3].tolist() == [[6, 1], [7, 2], [8, 5]] and t.match[3:].tolist() == [[1, 6], [2, 7], [5, 8]]
    assert t.views().tolist() == [1, 2, 2, 1, 1, 2, 2, 2, 2, 1]
    _same_as_the_loops(t, spec)
    # four cameras, a second take with two, and a take whose cameras share no frame
    spec = [((9, "sit", c), list(range(c, 10))) for c in (1, 2, 3, 4)] + [((9, "walk", 1), [0, 1]), ((9, "walk", 2), [1, 2]),
                                                                         ((11, "walk", 1), [0, 1]), ((11, "walk", 2), [5, 6])]
    t = ViewTable.from_sequences(*_sequences(spec))
    assert t.pairs == 12 + 2 and t.takes == 3
    # pair order: by target sequence, then source sequence; peer order: by source sequence
    assert list(zip(t.pair_dst.tolist(), t.pair_src.tolist()))[:6] == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3)]
    r = int(np.flatnonzero(_sequences(spec)[2][:9] == 5)[0])                      # frame 5 of the first camera: seen by all four
    assert t.peer_fit[t.peer_start[r]:t.peer_start[r + 1]].tolist() == [0, 1, 2] and t.views()[r] == 4 and t.views()[0] == 1
    assert [int(t.peer_row[k]) for k in range(t.peer_start[r], t.peer_start[r + 1])] == sorted(t.peer_row[t.peer_start[r]:t.peer_start[r + 1]].tolist())
    want = _same_as_the_loops(t, spec)
    assert np.bincount(t.views()).tolist() == np.bincount([1 + len(p) for p in want["peers"]]).tolist()
    # drop_takes: the flagged takes' rows keep zero peers, the pairs are renumbered, pair_origin names where they came from
    d = t.drop_takes(np.array([True, False, False]))
    assert d.pairs == 2 and d.pair_origin.tolist() == [12, 13] and d.views()[:int(t.peer_start.size - 1) - 8].max() == 1
    _same_as_the_loops(d, spec, dropped=(0,))
    d = t.drop_takes(np.array([False, True, True]))
    assert d.pairs == 12 and d.pair_origin.tolist() == list(range(12))
    _same_as_the_loops(d, spec, dropped=(1, 2))
    assert t.drop_takes(np.ones(3, dtype=bool)).pairs == 0 and t.drop_takes(np.ones(3, dtype=bool)).views().max() == 1
    with pytest.raises(ValueError):
        t.drop_takes(np.ones(2, dtype=bool))


def test_view_table_camera_spelling_filter_and_limits():
    from implementation_phd_lab_vision_amd.multiview import ViewTable
    # 1 and "1" are one spelling (they cannot both be sequences), "cam_1" is another camera: two views
    spec = [((9, "walk", 1), [0, 1, 2]), ((9, "walk", "cam_1"), [0, 1, 2]), ((9, "walk", 2), [0, 1, 2])]
    t = ViewTable.from_sequences(*_sequences(spec))
    assert t.pairs == 6 and t.views().tolist() == [3] * 9
    # the cams filter compares str(cam): 1 keeps the sequence keyed 1 (or "1"), not "cam_1"
    f = ViewTable.from_sequences(*_sequences(spec), cams=[1, "2"])
    assert f.pairs == 2 and f.seq_view.tolist() == [True, False, True] and f.views().tolist() == [2, 2, 2, 1, 1, 1, 2, 2, 2]
    assert set(f.pair_src.tolist()) == {0, 2}
    _same_as_the_loops(f, spec, cams=[1, "2"])
    assert ViewTable.from_sequences(*_sequences(spec), cams=["cam_1"]).pairs == 0
    # actions differ by spelling, subjects by value
    spec2 = [((9, "walk", 1), [0]), ((9, "walk 1", 2), [0]), (("9", "walk", 3), [0])]
    t2 = ViewTable.from_sequences(*_sequences(spec2))
    assert t2.takes == 2 and t2.pairs == 2 and sorted(t2.pair_src.tolist()) == [0, 2]
    # nine views of one take are refused; eight pass
    nine = [((9, "walk", c), [0, 1]) for c in range(9)]
    with pytest.raises(ValueError, match="9 views"):
        ViewTable.from_sequences(*_sequences(nine))
    assert ViewTable.from_sequences(*_sequences(nine[:8])).views().tolist() == [8] * 16
    with pytest.raises(ValueError, match="views"):
        ViewTable.from_sequences(*_sequences(nine[:4]), max_views=3)
    with pytest.raises(ValueError):
        ViewTable.from_sequences(*_sequences(nine[:2]), max_views=9)
    # a frame_idx that does not rise inside a sequence, and tables that do not fit
    with pytest.raises(ValueError, match="rise"):
        ViewTable.from_sequences([(9, "walk", 1)], np.array([0, 3]), np.array([0, 2, 2]))
    with pytest.raises(ValueError):
        ViewTable.from_sequences([(9, "walk", 1)], np.array([0, 2]), np.array([0, 1, 2]))


def test_host_validation_refuses_without_a_device():
    import torch
    from implementation_phd_lab_vision_amd import multiview as mv
    spec = [((9, "walk", 1), [0, 1, 2]), ((9, "walk", 2), [0, 1, 2])]
    t = mv.ViewTable.from_sequences(*_sequences(spec))
    bad = mv.ViewTable.from_sequences(*_sequences(spec))
    bad.peer_row = bad.peer_row.copy()
    bad.peer_row[0] = 6
    with pytest.raises(ValueError, match="peer row"):
        mv.DeviceViews(bad, "cpu")
    bad = mv.ViewTable.from_sequences(*_sequences(spec))
    bad.match = bad.match.copy()
    bad.match[0, 0] = -1
    with pytest.raises(ValueError, match="matched row"):
        mv.DeviceViews(bad, "cpu")
    views = mv.DeviceViews(t, "cpu")                                              # the tables themselves are plain tensors
    assert views.pairs == 2 and views.match.dtype == torch.int32 and views.match.numel() == 12
    with pytest.raises(ValueError, match="no CPU fallback"):                    # poses on the host: refused, not computed there
        mv.rigid_fit(torch.zeros(6, 17, 3), torch.zeros(6, 17, 3), views)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mv.fuse_views(torch.zeros(6, 17, 3), views, torch.zeros(2, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="mode"):
        mv.fuse_views(torch.zeros(6, 17, 3), views, torch.zeros(2, 16, dtype=torch.float64), "max")
    for kw in (dict(fit="svd"), dict(fuse="max"), dict(gt_tol_mm=0.0), dict(gt_tol_mm=float("nan"))):
        with pytest.raises(ValueError):
            mv.evaluate_multiview({}, "cuda:0", **kw)
    with pytest.raises(ValueError, match="keep_poses"):
        mv.evaluate_multiview({"group_names": ["walk"]}, "cuda:0")
    with pytest.raises(ValueError, match="no CPU fallback"):
        mv.evaluate_multiview({k: None for k in ("seq_keys", "seq_start", "frame_idx", "pred", "gt", "group_names")}, "cpu")


def test_the_restatement_recovers_an_exact_rigid_transform():
    rng = np.random.default_rng(3)
    for n in (4, 17, 300):
        y = rng.standard_normal((n, 3)) * 0.3 + [0.0, 0.0, 5.0]
        r, t = MR.random_rotation(rng), rng.standard_normal(3)
        fit, cond = MR.kabsch(y, y @ r.T + t)
        assert np.abs(fit[:9].reshape(3, 3) - r).max() < 1e-12 and np.abs(fit[9:12] - t).max() < 1e-11 and cond > 0.05
        assert fit[12] == n and fit[13] < 1e-13 and abs(fit[14] - 1.0) < 1e-12
        assert abs(np.linalg.det(fit[:9].reshape(3, 3)) - 1.0) < 1e-12
    # a reflection is not a rigid transform: the fit stays proper and the residual shows it
    y = rng.standard_normal((50, 3))
    fit, _ = MR.kabsch(y, y * [1.0, 1.0, -1.0])
    assert abs(np.linalg.det(fit[:9].reshape(3, 3)) - 1.0) < 1e-12 and fit[13] > 0.1
    # the three fuse modes and the disagreement on numbers worked by hand: own 0, two peers at 3 and 9 under identity fits
    pose = np.zeros((3, 1, 3), dtype=np.float32)
    pose[1], pose[2] = 3.0, 9.0
    ident = np.concatenate([np.eye(3).reshape(-1), np.zeros(7)])[None]
    peers = [[(1, 0), (2, 0)], [], []]
    for mode, want in ((0, 4.0), (1, 3.0), (2, 6.0)):
        fused, dis = MR.fuse(pose, peers, ident, mode)
        assert np.all(fused[0] == want) and np.all(fused[1] == 3.0) and dis[1] == 0.0
        assert dis[0] == pytest.approx(np.sqrt(3.0 * ((0 - want) ** 2 + (3 - want) ** 2 + (9 - want) ** 2) / 3.0))
    fused, _ = MR.fuse(pose, [[(1, 0)], [], []], ident, 1)
    assert np.all(fused[0] == 1.5)                                                # an even count: half the sum of the two middle values


def test_extrinsics_error_on_known_rotations():
    from implementation_phd_lab_vision_amd.multiview import extrinsics_error

    def rot_z(deg):
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])

    def slots(r, t):
        return np.concatenate([r.reshape(-1), t, np.zeros(4)])

    rng = np.random.default_rng(5)
    base = MR.random_rotation(rng)
    angles = [0.0, 1e-6, 0.5, 30.0, 90.0, 179.0, 180.0]
    a = np.stack([slots(rot_z(d) @ base, np.array([0.001 * k, 0.0, 0.0])) for k, d in enumerate(angles)])
    b = np.stack([slots(base, np.zeros(3)) for _ in angles])
    ang, shift = extrinsics_error(a, b)
    assert np.allclose(ang, angles, rtol=1e-9, atol=1e-12) and np.allclose(shift, np.arange(len(angles)), atol=1e-12)
    ang2, shift2 = extrinsics_error(b, a)                                          # symmetric
    assert np.allclose(ang2, ang, rtol=1e-9, atol=1e-12) and np.allclose(shift2, shift)
    want_ang, want_shift = MR.extrinsics_error(a[2:6], b[2:6])                     # arccos keeps its digits away from 0 and 180 degrees
    assert np.allclose(ang[2:6], want_ang, rtol=1e-9) and np.allclose(shift[2:6], want_shift)
    assert extrinsics_error(np.zeros((0, 16)), np.zeros((0, 16)))[0].shape == (0,)
    with pytest.raises(ValueError):
        extrinsics_error(a, b[:2])


def test_pearson_and_frame_p1():
    from implementation_phd_lab_vision_amd.multiview import frame_p1, pearson_r
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal(50), rng.standard_normal(50)
    assert pearson_r(a, b) == pytest.approx(np.corrcoef(a, b)[0, 1], rel=1e-12) and pearson_r(a, 2 * a + 1) == pytest.approx(1.0)
    assert np.isnan(pearson_r(a[:1], b[:1])) and np.isnan(pearson_r(a, np.ones(50)))
    from tests import protocols_reference as pr
    y, x = rng.standard_normal((4, 17, 3)).astype(np.float32), rng.standard_normal((4, 17, 3)).astype(np.float32)
    assert np.allclose(frame_p1(y, x), [pr.p1_pose(y[i], x[i]) for i in range(4)], rtol=1e-12)


def test_parser_flags_are_absent_unless_given_and_need_dense(capsys):
    from implementation_phd_lab_vision_amd import multiview as mv, results
    base = ["--features_root", "f", "--preprocessed_root", "v", "--model_path", "m"]
    args = results.parse_args(base + ["--dense"])
    assert not any(hasattr(args, k) for k in ("multiview",) + mv.OPTION_FLAGS) and mv.options_from_args(args) is None
    args = results.parse_args(base + ["--dense", "--multiview"])
    assert args.multiview is True and not any(hasattr(args, k) for k in mv.OPTION_FLAGS)
    assert mv.options_from_args(args) == {"fit": "gt", "fuse": "mean", "cams": None, "gt_tol_mm": 1.0}
    args = results.parse_args(base + ["--dense", "--multiview", "--multiview-fit", "pred", "--multiview-fuse", "median", "--multiview-cams", "1",
                                      "cam_2", "--multiview-gt-tol-mm", "0.5"])
    assert mv.options_from_args(args) == {"fit": "pred", "fuse": "median", "cams": ["1", "cam_2"], "gt_tol_mm": 0.5}
    for bad in (["--multiview"], ["--dense", "--multiview-fit", "pred"], ["--dense", "--multiview-fuse", "mean"], ["--dense", "--multiview-cams", "1"],
                ["--dense", "--multiview-gt-tol-mm", "2"], ["--dense", "--multiview", "--multiview-fit", "svd"],
                ["--dense", "--multiview", "--multiview-fuse", "max"], ["--dense", "--multiview", "--multiview-gt-tol-mm", "0"]):
        with pytest.raises(SystemExit):
            results.parse_args(base + bad)
    assert "--multiview needs --dense" in capsys.readouterr().err
