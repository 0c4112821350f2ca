"""Joint rotations on a rigid skeleton on the MI355X (include/r50_kinematics.h): both ops against the plain
numpy definition of tests/kinematics_reference.py on articulated figures; the exact cases bit for bit; the refusals; the ops between
poisoned guard bands and late on a side stream; ``predict --bvh`` and ``results --dense --dense-rigid`` end to end.

The bars.  The generator asserts its conditioning on the oracle's side (every frame-defining pair of vectors between 45 and 135 degrees,
every aim with 1 + d >= 0.1, |x_c - P[j]| >= half the bone's rest length), which bounds what one step amplifies an incoming error by:
a normalisation by 1 / 0.5 = 2 bone lengths, the frame's second normalisation by 1 / sin 45 = 1.5, the aim's division by 1 / 0.1 = 10;
30 covers their product with the matrix product that follows.  A joint takes about 200 fp64 roundings of 1.1e-16, and an error
entering at the root passes through at most depth 6 such steps (63 in the chain of 64, whose aims have no frame and amplify by 10):
200 * 1.1e-16 * 30 * 6 = 4e-12 and 200 * 1.1e-16 * 10 * 63 = 1.4e-11, so the fp64 part of every bar is below 1e-10 and the bars are the
fp32 roundings of the outputs:
  quat:  the matrix rebuilt in fp64 from the renormalised fp32 quaternion is within 2^-22 per element of the oracle's local rotation
         (an element is a sum of products like 2 (x y - w z): four components rounded by at most 2^-25 each give 2 * 2^-25 * (|x| + |y| +
         |w| + |z|) <= 2^-23 to first order; the rest is margin); a global rotation, the product of the depth + 1 local ones down to the
         joint, within (depth + 1) * sqrt(3) * 2^-22 (the errors add, and a row of a rotation has norm 1 over three elements);
  euler: the matrix rebuilt from the fp32 angles within 1e-6: three angles of at most 180 degrees, each rounded by at most 2^-24 * 180
         degrees = 1.9e-7 rad, move an element by at most 5.6e-7;
  rigid, resid: within 1 fp32 ulp of the oracle's value rounded to fp32, plus the fp64 part of 1e-10 (metres) as an absolute term: the
         fp64 values differ by that at most, so the two roundings differ only where the value lies that close to a rounding boundary;
         the absolute term is what is left where the value itself is rounding noise and has no ulp to speak of -- the residual of a
         one-row sequence is 5e-17, the sum of seventeen differences that are zero but for their last bits;
  rest:  within 1e-12 of the oracle's, relative to the bone's length (its components are sums of up to 70 signed terms of that size: a
         fixed tree against a running sum, 70 * 1.1e-16 * 2)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import bvh_reader
from tests import kinematics_reference as KR
from tests.guard_bands import run_row
from tests.kinematics_cases import CHAIN_SIGN, SHAPES, _case, _product_skeleton, _skeleton  # noqa: F401
from tests.rows.kinematics import ROWS_KINEMATICS
from tests.stream_order import run_row_late

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, I32 = torch.float32, torch.float64, torch.int32
FP64_PART = 1e-10          # what the two fp64 computations may differ by under the generator's conditioning (the derivation above)


def _tables(seq_start):
    from implementation_phd_lab_vision_amd.smooth import DeviceTables
    return DeviceTables(seq_start, np.concatenate([np.arange(n) for n in np.diff(seq_start)]).astype(np.int32), DEV)


def _ulp_ok(got, want64):
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64) + FP64_PART


@pytest.mark.parametrize("noise", [0.0, 0.005], ids=["rigid", "noise5mm"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_both_ops_against_the_definition(shape, noise):
    from implementation_phd_lab_vision_amd import kinematics as K
    c = _case(shape, noise)
    ref, sk = c["ref"], _product_skeleton(SHAPES[shape][0])
    x = torch.from_numpy(c["x"]).to(DEV)
    tables = _tables(c["seq_start"])
    rest = K.rest_offsets(x, tables, sk)
    rot = K.pose_rotations(x, tables, sk, rest)
    again = K.pose_rotations(x, tables, sk)
    torch.cuda.synchronize()
    for name in ("quat", "euler", "rigid", "resid", "flags", "rest"):             # two runs, the same bits
        a, b = getattr(rot, name), getattr(again, name)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    got_rest = rest.cpu().numpy()
    scale = np.linalg.norm(ref["rest"], axis=2, keepdims=True)
    err = np.abs(got_rest - ref["rest"]).max(axis=2, keepdims=True)
    print(f"{shape} noise {noise}: rest max error / bone length {np.max(err[scale > 0] / scale[scale > 0]):.2e}")
    assert np.all(err <= 1e-12 * scale)
    quat, euler = rot.quat.cpu().numpy(), rot.euler.cpu().numpy()
    rigid, resid, flags = rot.rigid.cpu().numpy(), rot.resid.cpu().numpy(), rot.flags.cpu().numpy()
    assert not np.isnan(quat).any() and not np.isnan(euler).any() and np.all(quat[..., 0] >= 0.0)
    assert np.all(flags == 0) and np.all(ref["flags"] == 0)
    f, joints = quat.shape[:2]
    _, parent, _ = KR.topology(c["edges"], joints)
    order = [j for j in range(joints) if j not in parent] + [ch for _, ch in c["edges"]]
    depth = {order[0]: 0}
    worst = dict(quat=0.0, euler=0.0, glob=0.0)
    for r in range(f):
        glob = {}
        for j in order:
            lq, le = KR.quat_matrix(quat[r, j]), KR.rot_zxy_deg(euler[r, j])
            worst["quat"] = max(worst["quat"], np.abs(lq - ref["L"][r, j]).max())
            worst["euler"] = max(worst["euler"], np.abs(le - ref["L"][r, j]).max())
            if j in parent:
                depth[j] = depth[parent[j]] + 1
                glob[j] = glob[parent[j]] @ lq
            else:
                glob[j] = lq
            worst["glob"] = max(worst["glob"], np.abs(glob[j] - ref["R"][r, j]).max() / (depth[j] + 1))
    print(f"{shape} noise {noise}: local from quat {worst['quat']:.2e} (bar {2.0 ** -22:.2e}), from euler {worst['euler']:.2e} (bar 1e-6), "
          f"global from quat / (depth + 1) {worst['glob']:.2e} (bar {np.sqrt(3.0) * 2.0 ** -22:.2e})")
    assert worst["quat"] <= 2.0 ** -22 and worst["euler"] <= 1e-6 and worst["glob"] <= np.sqrt(3.0) * 2.0 ** -22
    assert np.all(_ulp_ok(rigid, ref["rigid"])), np.abs(rigid - ref["rigid"]).max()
    assert np.all(_ulp_ok(resid, ref["resid"])), (resid, ref["resid"])
    if noise == 0.0:                                                               # exactly rigid but for the fp32 rounding of the input
        extent = float(np.abs(c["offs"]).sum(axis=(1, 2)).max())
        print(f"{shape}: residual on rigid input {resid.max():.2e}, extent {extent:.3f}")
        assert resid.max() <= 1e-6 * extent
    else:
        assert resid.mean() > 1e-3


def _exact_figure():
    """Three one-frame sequences of 17 joints in camera coordinates, every value a small binary fraction: a T-pose on the world axes with
    the pelvis at the origin; the same with the right knee and ankle straight ABOVE the hip; and an all-zero frame."""
    t = np.zeros((17, 3))
    t[[1, 14]] = (-0.125, 0.0, 0.0)
    t[[4, 11]] = (0.125, 0.0, 0.0)
    t[[15, 16]] = (-0.25, 0.0, 0.0)
    t[[12, 13]] = (0.25, 0.0, 0.0)
    t[[2, 3, 5, 6]] = (0.0, -0.5, 0.0)
    t[[7, 8, 9, 10]] = (0.0, 0.25, 0.0)
    up = t.copy()
    up[[2, 3]] = (0.0, 0.5, 0.0)
    poses = []
    for off in (t, up):
        p = np.zeros((17, 3))
        for a, b in KR.EDGES17:
            p[b] = p[a] + off[b]
        poses.append(p * np.asarray(KR.SIGN_H36M))
    poses.append(np.zeros((17, 3)))
    return np.stack(poses).astype(np.float32)


def test_the_exact_cases_bit_for_bit():
    from implementation_phd_lab_vision_amd import kinematics as K
    x = _exact_figure()
    assert np.array_equal(x.astype(np.float64).astype(np.float32), x)
    rot = K.pose_rotations(torch.from_numpy(x).to(DEV), _tables(np.array([0, 1, 2, 3], dtype=np.int32)))
    quat, euler, rigid = rot.quat.cpu().numpy(), rot.euler.cpu().numpy(), rot.rigid.cpu().numpy()
    resid, flags = rot.resid.cpu().numpy(), rot.flags.cpu().numpy()
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)      # noqa: E731
    ident = np.tile(np.array([1.0, 0.0, 0.0, 0.0], dtype=np.float32), (17, 1))
    for a in (quat, euler, rigid, resid, rot.rest.cpu().numpy()):
        assert not np.isnan(a).any()
    # rhip, lhip and spine on the axes: R_0 = I, and so is every other rotation of the T-pose
    assert np.array_equal(bits(quat[0]), bits(ident)) and np.array_equal(bits(euler[0]), bits(np.zeros((17, 3))))
    assert flags[0] == 0 and resid[0] == 0.0 and np.array_equal(rigid[0], x[0])
    # the knee straight above the hip: the antiparallel branch, R_1 = diag(-1, -1, 1), a half turn about z; the shin goes on straight
    want = ident.copy()
    want[1] = (0.0, 0.0, 0.0, 1.0)
    assert np.array_equal(bits(quat[1]), bits(want)), quat[1]
    assert flags[1] == K.FLAG_ANTIPARALLEL and resid[1] == 0.0 and np.array_equal(rigid[1], x[1])
    assert np.array_equal(KR.rot_zxy_deg(euler[1, 1]).round(6), np.diag([-1.0, -1.0, 1.0]))
    assert np.array_equal(bits(np.delete(euler[1], 1, axis=0)), bits(np.zeros((16, 3))))
    # the all-zero frame: both degenerate branches, identity everywhere, nothing undefined
    assert np.array_equal(bits(quat[2]), bits(ident)) and np.array_equal(bits(euler[2]), bits(np.zeros((17, 3))))
    assert flags[2] == (K.FLAG_FRAME | K.FLAG_REACH) and resid[2] == 0.0 and np.array_equal(rigid[2], x[2])
    assert np.array_equal(rot.rest[2].cpu().numpy(), np.zeros((17, 3)))
    # and the definition agrees on all three
    ref = KR.pose_rotations(x, np.array([0, 1, 2, 3]), KR.EDGES17, KR.FRAMES17, KR.rest_dirs17(), KR.SIGN_H36M)
    assert np.array_equal(ref["flags"], flags) and np.array_equal(ref["quat"].astype(np.float32), quat)
    assert np.array_equal(ref["R"][1, 1], np.diag([-1.0, -1.0, 1.0])) and np.array_equal(ref["R"][0, 0], np.eye(3))


def test_every_refusal_leaves_poisoned_outputs_untouched():
    from implementation_phd_lab_vision_amd import _lib, kinematics as K
    lib = _lib.load_library()
    c = _case("h36m-1+5+70", 0.005)
    f, s, j = 76, 3, 17
    x = torch.from_numpy(c["x"]).to(DEV)
    tables = _tables(c["seq_start"])
    good_rest = K.rest_offsets(x, tables)
    poison = lambda shape, dtype: torch.full(shape, 0x7B, dtype=torch.uint8, device=DEV).view(dtype)      # noqa: E731
    rest = poison((s, j, 3 * 8), F64).view(s, j, 3)
    outs = dict(quat=poison((f, j, 16), F32), euler=poison((f, j, 12), F32), rigid=poison((f, j, 12), F32), resid=poison((f * 4,), F32),
                flags=poison((f * 4,), I32))
    edges, e, frames, nf, dirs, sign = K.H36M_SKELETON.c_args()
    ints = lambda v: (ctypes.c_int * len(v))(*v)                                    # noqa: E731
    dbl = lambda v: (ctypes.c_double * len(v))(*v)                                  # noqa: E731
    ok = dict(F=f, S=s, J=j, edges=edges, E=e, frames=frames, NF=nf, dirs=dirs, sign=sign)
    bad = (dict(F=2 ** 31 // 192 + 1), dict(F=0), dict(S=f + 1), dict(J=65), dict(J=0),                       # the size limits
           dict(sign=dbl([1.0, -1.0, 1.0])), dict(sign=dbl([1.0, 0.5, 2.0])),                                   # a bad sign
           dict(edges=ints([1, 2, 0, 1] + list(edges)[4:])),                                                    # a child before its parent
           dict(frames=ints([0, 1, 4, 0, 17, 8, 14, 11, 8, 9])), dict(frames=ints([0, 1, 4, 0, -1, 8, 14, 11, 8, 9])),   # a frame row out of range
           dict(dirs=dbl([v * (1.001 if k == 3 else 1.0) for k, v in enumerate(dirs)])),                        # a rest direction off the unit sphere
           dict(E=15))
    stream = torch.cuda.current_stream().cuda_stream
    for kw in bad:
        a = dict(ok, **kw)
        rc = lib.r50_op_rest_offsets(x.data_ptr(), tables.seq_start.data_ptr(), a["F"], a["S"], a["J"], a["edges"], a["E"], a["frames"], a["NF"],
                                     a["dirs"], a["sign"], rest.data_ptr(), stream)
        assert rc == -1 and b"r50_op_rest_offsets" in lib.r50_last_error(None), kw
        rc = lib.r50_op_pose_rotations(x.data_ptr(), tables.row_seq.data_ptr(), a["F"], a["S"], a["J"], a["edges"], a["E"], a["frames"], a["NF"],
                                       a["dirs"], a["sign"], good_rest.data_ptr(), outs["quat"].data_ptr(), outs["euler"].data_ptr(),
                                       outs["rigid"].data_ptr(), outs["resid"].data_ptr(), outs["flags"].data_ptr(), stream)
        assert rc == -1 and b"r50_op_pose_rotations" in lib.r50_last_error(None), kw
    # an output on top of an input, or of another output
    rc = lib.r50_op_pose_rotations(x.data_ptr(), tables.row_seq.data_ptr(), f, s, j, edges, e, frames, nf, dirs, sign, good_rest.data_ptr(),
                                   outs["quat"].data_ptr(), outs["euler"].data_ptr(), outs["euler"].data_ptr(), outs["resid"].data_ptr(),
                                   outs["flags"].data_ptr(), stream)
    assert rc == -1 and b"overlaps" in lib.r50_last_error(None)
    torch.cuda.synchronize()
    for name, t in dict(outs, rest=rest).items():
        assert bool((t.view(torch.uint8) == 0x7B).all()), f"a refused call wrote to {name}"
    assert torch.equal(x.cpu(), torch.from_numpy(c["x"]))


# ---- both ops (the rows of tests/rows/kinematics.py) between poisoned guard bands, and late on a side stream ------------------------------
@pytest.mark.parametrize("row", ROWS_KINEMATICS, ids=[r.id for r in ROWS_KINEMATICS])
def test_kinematics_ops_between_guard_bands(row):
    run_row(row)


@pytest.mark.parametrize("row", ROWS_KINEMATICS, ids=[r.id for r in ROWS_KINEMATICS])
def test_late_on_a_side_stream_kinematics(row):
    run_row_late(row)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def _fk_bar(sk, rest_scaled, angle_term_rad, position_term):
    """tests/test_kinematics_cpu.py's bar (``_bvh_bar``: the %.6f roundings down the deepest chain) with another angle term, plus the
    rounding of the positions the file is compared with."""
    depth, length = np.zeros(sk.joints, dtype=int), np.zeros(sk.joints)
    for p, c in sk.edges:
        depth[c], length[c] = depth[p] + 1, length[p] + np.linalg.norm(rest_scaled[c])
    d = int(depth.max())
    return (d + 1) * np.sqrt(3.0) * 0.5e-6 + float(length.max()) * 3 * d * angle_term_rad + position_term


def test_predict_cli_writes_a_bvh_file_that_gives_the_rigid_poses_back(tmp_path, capsys):
    """11 frames, windows of 8 every 3: two windows.  The angles of the file are the fp32 ``rotations_euler_zxy_deg`` printed with six
    decimals: per angle 2^-24 * 180 degrees of fp32 rounding and 0.5e-6 degrees of printing; the positions it is compared with,
    ``joints3d_rigid`` * scale, are fp32: half an ulp of the largest coordinate per component."""
    from implementation_phd_lab_vision_amd import kinematics as K, predict
    from oracle.lifting_oracle import synthetic_head_state_dict
    video = torch.randint(0, 256, (11, 64, 48, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    np.save(tmp_path / "clip.npy", video.numpy())
    torch.save(synthetic_head_state_dict(64, 2, seed=1), tmp_path / "head.pt")
    argv = ["--frames", str(tmp_path / "clip.npy"), "--model_path", str(tmp_path / "head.pt"), "--synthetic-weights", "--seq-len", "8",
            "--stride", "3", "--frame-skip", "1", "--frame-batch", "16"]
    plain = predict.main(argv + ["--out", str(tmp_path / "a")])
    plain_out = capsys.readouterr().out
    scale = 10.0
    with_bvh = predict.main(argv + ["--out", str(tmp_path / "b"), "--bvh", "--bvh-scale", str(scale), "--bvh-fps", "50"])
    out = capsys.readouterr().out
    assert plain == [str(tmp_path / "a" / "clip_poses.npz")] and with_bvh == [str(tmp_path / "b" / "clip_poses.npz"), str(tmp_path / "b" / "clip.bvh")]
    assert "rigid skeleton: mean residual" in out and "rigid" not in plain_out and "2 windows" in out
    a, b = np.load(plain[0]), np.load(with_bvh[0])
    new = {"rotations_quat", "rotations_euler_zxy_deg", "rest_offsets", "joints3d_rigid", "rigid_residual", "rigid_flags"}
    assert set(b.files) - set(a.files) == new and set(a.files) <= set(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8) if a[k].ndim else a[k], b[k].view(np.uint8) if b[k].ndim else b[k]), k
    assert b["rotations_quat"].shape == (11, 17, 4) and b["rest_offsets"].shape == (17, 3) and b["rest_offsets"].dtype == np.float64
    sk = K.H36M_SKELETON
    bvh = bvh_reader.parse(open(with_bvh[1]).read())
    assert bvh["frames"] == 11 and bvh["frame_time"] == 0.02 and bvh["names"] == list(K.H36M_NAMES)
    world = b["joints3d_rigid"].astype(np.float64) * sk.sign * scale
    got = bvh_reader.forward_kinematics(bvh)
    angle = np.radians(0.5e-6 + 2.0 ** -24 * 180.0)
    bar = _fk_bar(sk, b["rest_offsets"] * scale, angle, np.sqrt(3.0) * 2.0 ** -24 * np.abs(world).max())
    err = np.linalg.norm(got - world, axis=2).max()
    print(f"predict --bvh: FK of the file against joints3d_rigid * scale: {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    # the file's npz holds what the library gives on the poses of the file
    again = K.video_rotations(b["joints3d"], DEV)
    for k in new:
        assert np.array_equal(again[k], b[k]), k
    # the dump entry point on the plain file computes the same rotations and writes the same text
    K.main(["--npz", plain[0], "--out", str(tmp_path / "later.bvh"), "--bvh-scale", str(scale), "--bvh-fps", "50"])
    assert open(tmp_path / "later.bvh").read() == open(with_bvh[1]).read()


def test_predict_refuses_another_joint_count_before_any_launch(tmp_path):
    """A checkpoint whose ``f_3D.y0`` holds 16 joints: ``--bvh`` is refused when the checkpoint is read, before the backbone exists (no
    other tensor of the state is looked at by then); and the library call refuses the same before it uploads anything."""
    from implementation_phd_lab_vision_amd import kinematics as K, predict
    from oracle.lifting_oracle import synthetic_head_state_dict
    state = synthetic_head_state_dict(64, 2, seed=1)
    state["f_3D.y0"] = state["f_3D.y0"].reshape(-1)[:48].clone()
    torch.save(state, tmp_path / "head16.pt")
    np.save(tmp_path / "clip.npy", np.zeros((11, 64, 48, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="16 joints need a kinematics.Skeleton"):
        predict.main(["--frames", str(tmp_path / "clip.npy"), "--model_path", str(tmp_path / "head16.pt"), "--synthetic-weights", "--out",
                      str(tmp_path / "o"), "--bvh"])
    assert not (tmp_path / "o").exists()
    with pytest.raises(ValueError, match="need a kinematics.Skeleton"):
        K.video_rotations(np.zeros((4, 16, 3), dtype=np.float32), DEV)


def test_results_cli_with_dense_rigid(tmp_path, capsys):
    from implementation_phd_lab_vision_amd import kinematics as K, protocols, results, sequences
    from tests import multiview_data as MD
    from tests.test_multiview_gpu import _results_base
    features = MD.make_multiview_cache(tmp_path / "features")
    videos = MD.make_preprocessed_tree(tmp_path / "videos")
    base = _results_base(tmp_path, features, videos, "tests.multiview_data:read_video")
    results.main(base + ["--out", str(tmp_path / "plain.npz"), "--dense-out", str(tmp_path / "plain_seq.npz")])
    plain_lines = capsys.readouterr().out.splitlines()
    results.main(base + ["--out", str(tmp_path / "rigid.npz"), "--dense-out", str(tmp_path / "rigid_seq.npz"), "--dense-rigid", "--dense-bvh",
                         str(tmp_path / "bvh")])
    rigid_lines = capsys.readouterr().out.splitlines()
    strip = lambda lines: [l for l in lines if not l.startswith("Dense | rigid") and ".npz" not in l and not l.startswith("Results time")]  # noqa: E731
    assert strip(rigid_lines) == strip(plain_lines) and not any("rigid" in l for l in plain_lines)
    extra = [l for l in rigid_lines if l.startswith("Dense | rigid")]
    assert len(extra) == 1 + 2 + 1 and "flagged frames" in extra[0] and "6 BVH files" in extra[-1]
    a, b = np.load(tmp_path / "plain.npz", allow_pickle=True), np.load(tmp_path / "rigid.npz", allow_pickle=True)
    assert set(b.files) - set(a.files) == {"dense_rigid_flagged"} | {f"dense_rigid_{m}{s}" for m in ("p1", "p2", "mpjve", "accel", "residual")
                                                                     for s in ("", "_all")}
    for k in a.files:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
    sa, sb = np.load(tmp_path / "plain_seq.npz"), np.load(tmp_path / "rigid_seq.npz")
    assert set(sa.files) == set(sb.files) and all(np.array_equal(sa[k], sb[k]) for k in sa.files)
    # the printed rigid P1 is sequence_metrics on the definition's rigid poses
    pred, gt, seq_start = sa["pred"], sa["gt"], sa["seq_start"]
    ref = KR.pose_rotations(pred, seq_start, KR.EDGES17, KR.FRAMES17, KR.rest_dirs17(), KR.SIGN_H36M)
    f = pred.shape[0]
    seq = np.repeat(np.arange(len(seq_start) - 1, dtype=np.int32), np.diff(seq_start))
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)               # noqa: E731
    part = sequences.sequence_metrics(dev(ref["rigid"].astype(np.float32)), dev(gt), dev(ref["resid"].astype(np.float32)),
                                      dev(np.arange(f + 1, dtype=np.int32)), dev(seq), dev(sa["frame_idx"].astype(np.int32)),
                                      dev(np.zeros(f, dtype=np.int32)), 1)
    sums = sequences.sum_blocks(part.cpu().numpy().reshape(-1, 1, sequences.METRIC_SLOTS))
    want_p1, want_resid = sums[0, 1] / sums[0, 0], sums[0, 6] / sums[0, 0]
    got_p1 = float(b["dense_rigid_p1_all"])
    print(f"results --dense-rigid: rigid p1 {got_p1!r} against the definition's {want_p1!r}; residual {float(b['dense_rigid_residual_all'])!r} "
          f"against {want_resid!r}")
    assert abs(got_p1 - want_p1) <= 1e-6 * want_p1 and abs(float(b["dense_rigid_residual_all"]) - want_resid) <= 1e-6 * want_resid
    raw_p1 = float(b["dense_p1_all"]) if "dense_p1_all" in b.files else None
    assert f"-> {got_p1 * 1000.0:.2f}" in extra[0] and (raw_p1 is None or f"p1 (mm) {raw_p1 * 1000.0:.2f} -> {got_p1 * 1000.0:.2f}" in extra[0])
    assert b["dense_rigid_flagged"].tolist() == [int(((ref["flags"] >> k) & 1).sum()) for k in range(3)]
    # one file per sequence key, each FK-consistent with the rigid poses of its sequence
    files = sorted(p.name for p in (tmp_path / "bvh").iterdir())
    assert files == sorted(K.sequence_file_name(tuple(k)) for k in sa["seq_keys"]) and len(files) == 6
    s = 1
    bvh = bvh_reader.parse((tmp_path / "bvh" / K.sequence_file_name(tuple(sa["seq_keys"][s]))).read_text())
    r0, r1 = int(seq_start[s]), int(seq_start[s + 1])
    assert bvh["frames"] == r1 - r0 and bvh["frame_time"] == 0.04
    world = ref["P"][r0:r1] * 100.0
    err = np.linalg.norm(bvh_reader.forward_kinematics(bvh) - world, axis=2).max()
    bar = _fk_bar(K.H36M_SKELETON, ref["rest"][s] * 100.0, np.radians(0.5e-6 + 2.0 ** -24 * 180.0), np.sqrt(3.0) * 2.0 ** -24 * np.abs(world).max() + 1e-8)
    print(f"results --dense-bvh: FK of sequence {s} against the definition's rigid poses * 100: {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    assert protocols.ROOT_JOINT == K.H36M_SKELETON.root
