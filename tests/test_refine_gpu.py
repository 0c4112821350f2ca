"""2D-guided refinement on the MI355X (include/r50_refine.h): both ops against the plain numpy definition of
tests/refine_reference.py on ragged tables; the exact cases bit for bit; the energy after 0, 1, 5, 20 and 50 sweeps; the refusals; the ops
between poisoned guard bands and late on a side stream; ``predict --refine-2d`` and ``results --dense --dense-refine`` end to end.

The bars.  Both sides compute a sweep in fp64 from the same fp32 inputs and differ in the order of a few sums and in how the 3x3 system
is solved (L D L^T against LAPACK); H has a condition number under 20 (its smallest eigenvalue is lambda_3d = 1, its largest at most
1 + 6 + 2 bones + the 2D block), so one sweep adds a difference of some 1e-15 m, and the sweep is a contraction, so 50 of them stay
under 1e-13 m.  The store rounds once to fp32: the two results differ by at most 1 fp32 ulp, where the fp64 values straddle a rounding
boundary -- the bar the issue sets, taken at the magnitude of the frame's largest coordinate.  The energies are sums of up to 130 * 64
non-negative terms in two different orders: 1e-12 relative; the issue's bar is 1e-9, and the counts are exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import refine_reference as RR
from tests.guard_bands import run_row
from tests.refine_cases import SEEDS, _case  # noqa: F401
from tests.rows.refine import ROWS_REFINE
from tests.stream_order import run_row_late

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, I32 = torch.float32, torch.float64, torch.int32


@functools.lru_cache(maxsize=None)
def _reference(joints, with_conf, lbone):
    c = _case(joints, with_conf)
    return RR.refine(c["x0"], c["rays"], c["conf"], c["seq_start"], c["idx"], c["edges"], c["bone_len"], iters=50, lbone=lbone)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _tables(c):
    from implementation_phd_lab_vision_amd.smooth import DeviceTables
    return DeviceTables(c["seq_start"], c["idx"], DEV)


def _operands(c, lbone):
    """(x0, rays, conf, tables, bone_len) on the device."""
    return (_dev(c["x0"]), _dev(c["rays"]), None if c["conf"] is None else _dev(c["conf"]), _tables(c),
            _dev(c["bone_len"]) if lbone != 0.0 else None)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("lbone", [0.0, 1.0], ids=["bone0", "bone1"])
@pytest.mark.parametrize("with_conf", [True, False], ids=["conf", "confNULL"])
@pytest.mark.parametrize("joints", [17, 3, 64], ids=["h36m", "chain3", "chain64"])
def test_both_ops_against_the_definition(joints, with_conf, lbone):
    from implementation_phd_lab_vision_amd import refine as R
    c = _case(joints, with_conf)
    settings = R.RefineSettings(lambda_bone=lbone, edges=c["edges"])
    x0, rays, conf, tables, lens = _operands(c, lbone)
    assert tables.segments == 9 and tables.sequences == 6 and sorted(np.diff(tables.seg_start_host)) == [1, 2, 3, 4, 5, 63, 64, 65, 130]
    got_t = R.fit_sweeps(x0, rays, conf, tables, settings, lens)
    ws = torch.full((2 * x0.numel(),), float("nan"), dtype=F64, device=DEV)
    again = R.fit_sweeps(x0, rays, conf, tables, settings, lens, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got_t), _bits(again)), "two calls, the second with a workspace full of NaN: the same bits"
    got = got_t.cpu().numpy()
    ref = _reference(joints, with_conf, lbone)
    assert np.isfinite(got).all()
    want = ref.astype(np.float32)
    ulp = np.spacing(np.abs(want).max(axis=(1, 2), keepdims=True)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
    moved = float(np.abs(ref - c["x0"].astype(np.float64)).max())
    print(f"J {joints} conf {with_conf} lbone {lbone}: poses max error {err.max():.2f} ulp of the frame's largest coordinate (bar 1), "
          f"{int((err > 0).sum())} of {err.size} values differ; the fit moved a coordinate by up to {moved * 1000:.1f} mm")
    assert err.max() <= 1.0 and moved > 0.01
    worst = 0.0
    for name, x_t, x in (("x0", x0, c["x0"]), ("refined", got_t, got)):
        en = R.fit_energy(x_t, x0, rays, conf, tables, settings.z_min, c["edges"], lens).cpu().numpy()
        ref_en = RR.energy(x, c["x0"], c["rays"], c["conf"], c["seq_start"], c["idx"], c["edges"], c["bone_len"] if lbone != 0.0 else None)
        assert en.shape == (6, 6) and np.array_equal(en[:, 5], ref_en[:, 5]), (name, en[:, 5], ref_en[:, 5])
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(ref_en[:, :5] != 0.0, np.abs(en[:, :5] - ref_en[:, :5]) / np.abs(ref_en[:, :5]), np.abs(en[:, :5]))
        worst = max(worst, float(rel.max()))
        assert rel.max() <= 1e-9, (name, rel)
        if name == "x0":                                                            # the case holds what it is meant to hold
            assert en[:, 5].sum() == 12 and np.all(en[:, 1] == 0.0) and np.all(en[:2, 2] == 0.0) and np.all(en[2:, 2] > 0.0)
            assert (en[:, 3] > 0.0).all() if lbone != 0.0 else (en[:, 3] == 0.0).all()
            if with_conf:
                assert (c["conf"] == 0.0).sum() > 100 and en[:, 4].sum() < c["conf"].size
            else:
                assert en[:, 4].sum() == c["x0"].shape[0] * joints - 12
    print(f"J {joints} conf {with_conf} lbone {lbone}: energies max relative error {worst:.2e} (bar 1e-9), counts exact")


def test_the_exact_cases_bit_for_bit():
    from implementation_phd_lab_vision_amd import refine as R
    c = dict(_case(17, True))
    x0_host = c["x0"].copy()
    x0_host.reshape(-1)[::101] = -0.0                                               # a few negative zeros: their sign is a bit too
    c["x0"] = x0_host
    x0, rays, conf, tables, lens = _operands(c, 1.0)
    # iters = 0: a copy, whatever the weights
    out = R.fit_sweeps(x0, rays, conf, tables, R.RefineSettings(iters=0, lambda_bone=1.0), lens)
    assert torch.equal(_bits(out), _bits(x0)) and out.data_ptr() != x0.data_ptr()
    # only the distance to the prediction: g is exactly 0 at every sweep
    out = R.fit_sweeps(x0, rays, conf, tables, R.RefineSettings(iters=7, lambda_2d=0.0, lambda_acc=0.0, lambda_3d=0.3, omega=0.75))
    assert torch.equal(_bits(out), _bits(x0))
    # no temporal and no bone term: a joint that was not detected stays, every detected joint in front of the camera moves
    out = R.fit_sweeps(x0, rays, conf, tables, R.RefineSettings(iters=5, lambda_acc=0.0))
    off = conf == 0.0
    assert bool(off.any()) and torch.equal(_bits(out)[off], _bits(x0)[off])
    seen = (~off) & (x0[..., 2] >= 0.1)
    assert bool((_bits(out)[seen] != _bits(x0)[seen]).any(dim=1).all())
    # the same bits from two calls, and with the workspace full of NaN, with every term on
    s = R.RefineSettings(iters=9, lambda_bone=1.0)
    a = R.fit_sweeps(x0, rays, conf, tables, s, lens)
    b = R.fit_sweeps(x0, rays, conf, tables, s, lens, workspace=torch.full((2 * x0.numel(),), float("nan"), dtype=F64, device=DEV))
    e1 = R.fit_energy(a, x0, rays, conf, tables, 0.1, c["edges"], lens)
    e2 = R.fit_energy(b, x0, rays, conf, tables, 0.1, c["edges"], lens)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(e1.view(torch.int64), e2.view(torch.int64)) and not torch.equal(_bits(a), _bits(x0))
    # refine_sequences: the default bone lengths are the mean column of bone_stats; the energies are the energy op's
    from implementation_phd_lab_vision_amd import smooth
    refined, info = R.refine_sequences(x0, rays, conf, (c["seq_start"], c["idx"]), s)
    want_len = smooth.bone_stats(x0, tables, s.edges)[:, :, 0].contiguous()
    assert torch.equal(info["bone_len"], want_len)
    assert torch.equal(_bits(refined), _bits(R.fit_sweeps(x0, rays, conf, tables, s, want_len)))
    assert torch.equal(info["energy_before"], R.fit_energy(x0, x0, rays, conf, tables, 0.1, s.edges, want_len))
    assert torch.equal(info["energy_after"], R.fit_energy(refined, x0, rays, conf, tables, 0.1, s.edges, want_len))


def test_the_energy_from_the_energy_op_never_rises():
    """The issue's sequence (300 rows, two segments, J 17, defaults): the weighted energy of the op's own result after 0, 1, 5, 20 and 50
    sweeps, scored by the energy op, is non-increasing within 1e-9 of itself, and ends where the definition's ends."""
    from implementation_phd_lab_vision_amd import refine as R
    p = RR.prototype_sequence(0)
    x0, rays = _dev(p["x0"]), _dev(p["rays"])
    tables = _tables(p)
    assert tables.segments == 2 and tables.sequences == 1
    totals = []
    for k in (0, 1, 5, 20, 50):
        x = R.fit_sweeps(x0, rays, None, tables, R.RefineSettings(iters=k))
        en = R.fit_energy(x, x0, rays, None, tables).cpu().numpy()
        assert en.shape == (1, 6) and en[0, 3] == 0.0 and en[0, 4] == 300 * 17 and en[0, 5] == 0.0
        totals.append(RR.total(en))
    print("energy after 0, 1, 5, 20, 50 sweeps: " + ", ".join(f"{v:.6f}" for v in totals))
    assert all(b <= a * (1.0 + 1e-9) for a, b in zip(totals[:-1], totals[1:])) and totals[-1] < 0.25 * totals[0]
    ref = RR.refine(p["x0"], p["rays"], None, p["seq_start"], p["idx"], iters=50)
    want = RR.total(RR.energy(ref.astype(np.float32), p["x0"], p["rays"], None, p["seq_start"], p["idx"]))
    # two fp32 roundings of poses at most 1 ulp (4.8e-7 m at 5 m) apart: a term (d + e)^2 with d of some 20 mm moves by 2 e / d = 5e-5 of itself
    assert abs(totals[-1] - want) <= 1e-4 * want


def test_every_refusal_leaves_poisoned_outputs_and_workspace_untouched():
    from implementation_phd_lab_vision_amd import _lib
    lib = _lib.load_library()
    c = _case(17, True)
    f, j, g, s = 337, 17, 9, 6
    x0, rays, conf, tables, lens = _operands(c, 1.0)
    poison = lambda n, dtype: torch.full((n,), 0x7B, dtype=torch.uint8, device=DEV).view(dtype)      # noqa: E731
    out, ws, energy = poison(f * j * 3 * 4, F32), poison(2 * f * j * 3 * 8, F64), poison(s * 6 * 8, F64)
    ints = lambda v: (ctypes.c_int * len(v))(*v)                                    # noqa: E731
    edges = ints([v for e in RR.EDGES17 for v in e])
    stream = torch.cuda.current_stream().cuda_stream
    nan, inf = float("nan"), float("inf")
    ok = dict(F=f, G=g, S=s, J=j, edges=edges, E=16, lens=lens.data_ptr(), l2d=1.0, l3d=1.0, lacc=1.0, lbone=1.0, omega=0.6, z_min=0.1, iters=5,
              out=out.data_ptr(), ws=ws.data_ptr())
    bad = (dict(l3d=0.0), dict(l3d=-1.0), dict(l3d=nan), dict(l2d=-1.0), dict(l2d=inf), dict(lacc=nan), dict(lbone=-2.0), dict(omega=0.0),
           dict(omega=0.8), dict(omega=nan), dict(z_min=0.0), dict(z_min=-0.1), dict(iters=-1), dict(iters=1001), dict(J=0), dict(J=65),
           dict(F=0), dict(F=2 ** 31 // 192 + 1), dict(G=f + 1), dict(S=g + 1), dict(E=17), dict(edges=ints([1, 2, 0, 1] + list(edges)[4:])),
           dict(edges=ints([0, 17] + list(edges)[2:])), dict(lens=None), dict(E=0, edges=None), dict(out=x0.data_ptr()),
           dict(out=x0.data_ptr() + 8), dict(out=ws.data_ptr() + 16), dict(ws=x0.data_ptr()), dict(out=None), dict(ws=None))
    for kw in bad:
        a = dict(ok, **kw)
        rc = lib.r50_op_pose_fit_sweeps(x0.data_ptr(), rays.data_ptr(), conf.data_ptr(), tables.seg_start.data_ptr(), tables.row_seg.data_ptr(),
                                        tables.row_seq.data_ptr(), a["F"], a["G"], a["S"], a["J"], a["edges"], a["E"], a["lens"], a["l2d"],
                                        a["l3d"], a["lacc"], a["lbone"], a["omega"], a["z_min"], a["iters"], a["ws"], a["out"], stream)
        assert rc == -1 and b"r50_op_pose_fit_sweeps" in lib.r50_last_error(None), kw
    ok = dict(F=f, S=s, J=j, edges=edges, E=16, lens=lens.data_ptr(), z_min=0.1, energy=energy.data_ptr())
    for kw in (dict(z_min=0.0), dict(z_min=nan), dict(J=65), dict(F=0), dict(S=f + 1), dict(E=17), dict(E=0, edges=None),
               dict(edges=ints([1, 2, 0, 1] + list(edges)[4:])), dict(energy=x0.data_ptr()), dict(energy=None)):
        a = dict(ok, **kw)
        rc = lib.r50_op_pose_fit_energy(x0.data_ptr(), x0.data_ptr(), rays.data_ptr(), conf.data_ptr(), tables.seq_start.data_ptr(),
                                        tables.row_seg.data_ptr(), a["F"], a["S"], a["J"], a["edges"], a["E"], a["lens"], a["z_min"], a["energy"],
                                        stream)
        assert rc == -1 and b"r50_op_pose_fit_energy" in lib.r50_last_error(None), kw
    torch.cuda.synchronize()
    for name, t in dict(out=out, workspace=ws, energy=energy).items():
        assert bool((t.view(torch.uint8) == 0x7B).all()), f"a refused call wrote to {name}"
    assert torch.equal(x0.cpu(), torch.from_numpy(c["x0"]))


# ---- both ops (the rows of tests/rows/refine.py) between poisoned guard bands, and late on a side stream ----------------------------------
@pytest.mark.parametrize("row", ROWS_REFINE, ids=[r.id for r in ROWS_REFINE])
def test_refine_ops_between_guard_bands(row):
    run_row(row)


@pytest.mark.parametrize("row", ROWS_REFINE, ids=[r.id for r in ROWS_REFINE])
def test_late_on_a_side_stream_refine(row):
    run_row_late(row)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8) if a.ndim else a, b.view(np.uint8) if b.ndim else b)


def test_predict_cli_with_refine_2d(tmp_path, capsys):
    """11 frames, windows of 8 every 3: two windows; the 2D joints, their confidences and the camera ride in the input ``.npz``."""
    from implementation_phd_lab_vision_amd import predict, refine as R
    from oracle.lifting_oracle import synthetic_head_state_dict
    g = torch.Generator().manual_seed(7)
    video = torch.randint(0, 256, (11, 64, 48, 3), generator=g, dtype=torch.uint8).numpy()
    rng = np.random.default_rng(7)
    joints2d = rng.uniform(4.0, 44.0, (11, 17, 2)).astype(np.float32)
    conf2d = rng.uniform(0.0, 1.0, (11, 17)).astype(np.float32)
    conf2d[::3, ::4] = 0.0
    f, c = np.array([60.0, 62.0], dtype=np.float32), np.array([24.0, 32.0], dtype=np.float32)
    np.savez(tmp_path / "clip.npz", frames=video, joints2d=joints2d, conf2d=conf2d, f=f, c=c, box=np.array([8, 0, 48, 48]))
    torch.save(synthetic_head_state_dict(64, 2, seed=1), tmp_path / "head.pt")
    argv = ["--frames", str(tmp_path / "clip.npz"), "--model_path", str(tmp_path / "head.pt"), "--synthetic-weights", "--seq-len", "8",
            "--stride", "3", "--frame-skip", "1", "--frame-batch", "16"]
    plain = predict.main(argv + ["--out", str(tmp_path / "a")])
    capsys.readouterr()
    fitted = predict.main(argv + ["--out", str(tmp_path / "b"), "--refine-2d", "--refine-iters", "6", "--refine-z-min", "0.001"])
    zero = predict.main(argv + ["--out", str(tmp_path / "c"), "--refine-2d", "--refine-iters", "0", "--smooth", "gauss"])
    a, b, z = np.load(plain[0]), np.load(fitted[0]), np.load(zero[0])
    new = {"joints3d_unrefined", "refine", "refine_energy_before", "refine_energy_after"}
    assert set(b.files) - set(a.files) == new and set(a.files) <= set(b.files)
    for k in a.files:
        if k != "joints3d":
            assert _same(a[k], b[k]), k
    assert _same(b["joints3d_unrefined"], a["joints3d"]) and b["refine_energy_before"].shape == b["refine_energy_after"].shape == (1, 6)
    assert "iters=6" in str(b["refine"]) and "z_min=0.001" in str(b["refine"])
    # the file holds what the library gives on the unrefined poses of the file, and the energy op's terms
    settings = R.RefineSettings(iters=6, z_min=0.001)
    rays = R.rays_from_pixels(joints2d, (f, c))
    refined, info = R.refine_video(torch.from_numpy(b["joints3d_unrefined"]).to(DEV), rays, conf2d, settings)
    assert _same(refined.cpu().numpy(), b["joints3d"]) and not _same(b["joints3d"], a["joints3d"])
    assert _same(info["energy_before"].cpu().numpy(), b["refine_energy_before"]) and _same(info["energy_after"].cpu().numpy(), b["refine_energy_after"])
    tables = (np.array([0, 11], dtype=np.int32), np.arange(11, dtype=np.int32))
    want = RR.energy(b["joints3d"], b["joints3d_unrefined"], rays, conf2d, *tables, z_min=0.001)
    assert np.array_equal(want[:, 5], b["refine_energy_after"][:, 5]) and np.allclose(want[:, :5], b["refine_energy_after"][:, :5], rtol=1e-9, atol=0)
    print(f"predict --refine-2d: energy terms before {b['refine_energy_before'][0].tolist()} after {b['refine_energy_after'][0].tolist()}")
    # --refine-iters 0: the bits of a run without the flag, and joints3d_raw is still the input of the post-process
    assert _same(z["joints3d_unrefined"], a["joints3d"]) and _same(z["joints3d_raw"], a["joints3d"]) and not _same(z["joints3d"], a["joints3d"])
    assert _same(z["refine_energy_before"], z["refine_energy_after"])


def test_predict_refuses_an_input_without_2d_joints_or_camera_before_any_launch(tmp_path):
    from implementation_phd_lab_vision_amd import predict
    from oracle.lifting_oracle import synthetic_head_state_dict
    torch.save(synthetic_head_state_dict(64, 2, seed=1), tmp_path / "head.pt")
    video = np.zeros((11, 64, 48, 3), dtype=np.uint8)
    np.save(tmp_path / "bare.npy", video)
    np.savez(tmp_path / "nocam.npz", frames=video, joints2d=np.zeros((11, 17, 2), dtype=np.float32))
    np.savez(tmp_path / "no2d.npz", frames=video, f=np.ones(2), c=np.ones(2))
    for name in ("bare.npy", "nocam.npz", "no2d.npz"):
        with pytest.raises(ValueError, match="--refine-2d needs `joints2d` and the camera"):
            predict.main(["--frames", str(tmp_path / name), "--model_path", str(tmp_path / "head.pt"), "--synthetic-weights", "--out",
                          str(tmp_path / "o"), "--refine-2d"])
    assert not (tmp_path / "o").exists()                                            # the output folder is made after the backbone is built


def test_results_cli_with_dense_refine(tmp_path, capsys):
    from implementation_phd_lab_vision_amd import refine as R, results
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from tests import multiview_data as MD
    from tests.test_multiview_gpu import _results_base
    features = MD.make_multiview_cache(tmp_path / "features")
    videos = MD.make_preprocessed_tree(tmp_path / "videos")
    base = _results_base(tmp_path, features, videos, "tests.multiview_data:read_video")
    results.main(base + ["--out", str(tmp_path / "plain.npz"), "--dense-out", str(tmp_path / "plain_seq.npz")])
    plain_lines = capsys.readouterr().out.splitlines()
    results.main(base + ["--out", str(tmp_path / "fit.npz"), "--dense-out", str(tmp_path / "fit_seq.npz"), "--dense-refine",
                         "--dense-refine-noise-px", "2", "--dense-refine-seed", "5", "--refine-iters", "10"])
    fit_lines = capsys.readouterr().out.splitlines()
    strip = lambda lines: [l for l in lines if not l.startswith("Dense | refine") and ".npz" not in l and not l.startswith("Results time")]  # noqa: E731
    assert strip(fit_lines) == strip(plain_lines) and not any("refine" in l for l in plain_lines)
    extra = [l for l in fit_lines if l.startswith("Dense | refine")]
    assert len(extra) == 1 + 2 and "ground-truth 2D + 2 px noise (224 crop, seed 5)" in extra[0] and "iters=10" in extra[0]
    assert "reprojection (mm)" in extra[0] and "joints skipped behind z_min" in extra[0]
    a, b = np.load(tmp_path / "plain.npz", allow_pickle=True), np.load(tmp_path / "fit.npz", allow_pickle=True)
    want_keys = {"dense_refine", "dense_refine_skipped", "dense_refine_noise", "dense_refine_energy_before", "dense_refine_energy_after"} | \
        {f"dense_refine_{m}{s}" for m in ("p1", "p2", "mpjve", "accel", "residual_raw", "residual") for s in ("", "_all")}
    assert set(b.files) - set(a.files) == want_keys and set(a.files) <= set(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
    sa, sb = np.load(tmp_path / "plain_seq.npz"), np.load(tmp_path / "fit_seq.npz")
    assert set(sb.files) - set(sa.files) == {"pred_refined", "refine"} and all(np.array_equal(sa[k], sb[k]) for k in sa.files)
    assert b["dense_refine_noise"].tolist() == [2.0, 5.0] and b["dense_refine_energy_after"].shape == (6, 6)
    # the exported poses are the library's on the exported raw poses with the same rays, and the printed P1 is theirs
    store = DeviceFeatureStore(str(features), subjects=[9], test_set=True, device=DEV)
    dense = {k: sa[k] for k in ("pred", "seq_start", "frame_idx")}
    rays, focal = R._dense_rays_focal(store, dense)
    rays = (rays.astype(np.float64) + 2.0 * np.random.default_rng(5).standard_normal(rays.shape) / focal[:, None, :]).astype(np.float32)
    refined, info = R.refine_sequences(_dev(sa["pred"]), _dev(rays), None, (sa["seq_start"], sa["frame_idx"]), R.RefineSettings(iters=10))
    assert _same(refined.cpu().numpy(), sb["pred_refined"])
    assert np.array_equal(info["energy_after"].cpu().numpy(), b["dense_refine_energy_after"])
    rel = lambda x: x.astype(np.float64) - x[:, :1].astype(np.float64)              # noqa: E731  (P1 is root-relative)
    p1 = float(np.linalg.norm(rel(sb["pred_refined"]) - rel(sa["gt"]), axis=2).mean())
    assert abs(float(b["dense_refine_p1_all"]) - p1) <= 1e-6 * p1 and f"-> {float(b['dense_refine_p1_all']) * 1000.0:.2f}" in extra[0]
