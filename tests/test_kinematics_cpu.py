"""Joint rotations and BVH export without a GPU: the oracle of tests/kinematics_reference.py on exactly rigid
figures and on its Euler angles; ``bvh_text`` read back by tests/bvh_reader.py; the fifth public header include/r50_kinematics.h bound,
exported and guard-banded; every refusal of its ops before any launch; the skeleton's host checks; and the parsers."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import bvh_reader
from tests import kinematics_reference as KR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "r50_kinematics.h"
OPS = {"r50_op_rest_offsets", "r50_op_pose_rotations"}
PREDICT_KEYS = ['box', 'device', 'flip_tta', 'frame_batch', 'frame_skip', 'frames', 'fuse', 'head_precision', 'input_len', 'model_path', 'out',
                'precision', 'pred_len', 'render', 'render_fps', 'render_frames', 'resize_mode', 'seq_len', 'stride', 'synthetic_weights',
                'weights', 'weights_from', 'weights_seed', 'window_batch']
RESULTS_KEYS = ['aligned_video', 'auc_steps', 'batch_size', 'dense', 'dense_fuse', 'dense_out', 'detail_metrics', 'device', 'dtw', 'dtw_band',
                'features_root', 'geo_metrics', 'input_len', 'model_path', 'num_workers', 'out', 'pck_threshold_mm', 'precision', 'pred_len',
                'preprocessed_root', 'protocols', 'render', 'render_fps', 'render_n', 'render_sheet_every', 'save_n', 'seed', 'seq_len',
                'test_subjects', 'video_reader', 'video_size', 'weights_from']


def _h36m(x, seq_start, rest=None):
    return KR.pose_rotations(x, seq_start, KR.EDGES17, KR.FRAMES17, KR.rest_dirs17(), KR.SIGN_H36M, rest)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_oracle_reproduces_an_exactly_rigid_sequence(seed):
    """On fp64 positions (the fp32 cast alone leaves 2^-24 * 5 m per coordinate) the residual is rounding, at most 1e-9 of the figure's
    extent, and ``rest`` is the generating offset expressed in the parent's frame: for the child of a framed joint the T-pose offset itself
    (in the T-pose the pelvis and thorax frames lie on the world axes), for any other child the rest direction times the bone's length.
    The generator's conditioning holds on every frame, without noise and with 5 mm of it."""
    x, seq_start, offs = KR.articulated(seed, [50], dtype=np.float64)
    exact = _h36m(x, seq_start)
    KR.assert_conditioned(exact)
    extent = np.abs(offs[0]).sum()
    assert exact["resid"].max() <= 1e-9 * extent, exact["resid"].max()
    assert np.abs(exact["rigid"] - x).max() <= 1e-9 * extent
    dirs = KR.rest_dirs17()
    for p, c in KR.EDGES17:
        want = offs[0][c] if p in (0, 8) else dirs[c] * np.linalg.norm(offs[0][c])
        assert np.abs(exact["rest"][0, c] - want).max() <= 1e-12, (c, exact["rest"][0, c], want)
    r = exact["R"].reshape(-1, 3, 3)                                               # every global rotation is a rotation
    assert np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(r) - 1.0).max() < 1e-12
    for noise in (0.0, 0.005):
        x32, seq_start, _ = KR.articulated(seed, [50], noise=noise)
        ref = _h36m(x32, seq_start)
        KR.assert_conditioned(ref)
        print(f"seed {seed} noise {noise}: min 1 + d {ref['min_1pd']:.3f}, frame angles {ref['frame_angles'].min():.1f} .. "
              f"{ref['frame_angles'].max():.1f}, min reach {ref['min_reach']:.3f}, mean residual {ref['resid'].mean() * 1000:.3f} mm")


def test_euler_angles_and_quaternions_give_the_rotation_back():
    rng = np.random.default_rng(11)
    mats = [KR.rodrigues(rng.normal(0.0, 1.5, size=3)) for _ in range(200)]
    for deg in (90.0, -90.0):                                                      # the gimbal case, constructed: L21 = +-1
        mats += [KR.rot_zxy_deg([z, deg, y]) for z, y in ((20.0, 0.0), (-75.0, 40.0), (170.0, -130.0))]
    mats += [np.eye(3), np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0])]
    gimbal = 0
    for m in mats:
        e = KR.euler_zxy_deg(m)
        assert np.abs(KR.rot_zxy_deg(e) - m).max() <= 1e-12, (m, e)
        gimbal += abs(m[2, 1]) > 1.0 - 1e-12 and e[2] == 0.0
        q = KR.quat_of(m)
        assert q[0] >= 0.0 and abs(np.linalg.norm(q) - 1.0) < 1e-12 and np.abs(KR.quat_matrix(q) - m).max() <= 1e-12
    assert gimbal == 6
    assert KR.quat_of(np.eye(3)).tolist() == [1.0, 0.0, 0.0, 0.0] and KR.quat_of(np.diag([-1.0, -1.0, 1.0])).tolist() == [0.0, 0.0, 0.0, 1.0]
    assert KR.euler_zxy_deg(np.eye(3)).tolist() == [0.0, 0.0, 0.0] and not np.signbit(KR.euler_zxy_deg(np.eye(3))).any()


def _bvh_bar(sk, rest_scaled, angle_term_rad):
    """The distance FK of the file may be from the positions the file was written from, per joint at most: every chain from the root to a
    joint of depth D adds the root position's rounding, D offsets' roundings (each sqrt(3) * 0.5e-6 in file units: %.6f) and, per bone
    of length l whose direction has passed through k <= D rotations of three angles each, l * 3 k * angle_term (a rotation by an angle
    wrong by e moves a unit vector by at most e).  Taken at the deepest joint with the sum of all its chain's bone lengths."""
    depth, length = np.zeros(sk.joints, dtype=int), np.zeros(sk.joints)
    for p, c in sk.edges:
        depth[c], length[c] = depth[p] + 1, length[p] + np.linalg.norm(rest_scaled[c])
    d = int(depth.max())
    return (d + 1) * np.sqrt(3.0) * 0.5e-6 + float(length.max()) * 3 * d * angle_term_rad


def test_bvh_text_read_back_and_forward_kinematics():
    from implementation_phd_lab_vision_amd import kinematics as K
    sk = K.H36M_SKELETON
    x, seq_start, _ = KR.articulated(5, [12], noise=0.005)
    ref = _h36m(x, seq_start)
    scale, fps = 100.0, 25.0
    text = K.bvh_text(sk, ref["rest"][0], ref["P"][:, sk.root], ref["euler"], fps, scale)
    bvh = bvh_reader.parse(text)
    order = sk.hierarchy_order()
    assert bvh["names"] == [sk.names[k] for k in order] and sorted(bvh["names"]) == sorted(K.H36M_NAMES)
    assert order == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]           # H36M's edge list is already depth first
    assert bvh["channels"][0] == ["Xposition", "Yposition", "Zposition", "Zrotation", "Xrotation", "Yrotation"]
    assert all(c == ["Zrotation", "Xrotation", "Yrotation"] for c in bvh["channels"][1:])
    assert bvh["frames"] == 12 and bvh["frame_time"] == 0.04 and "Frames: 12\nFrame Time: 0.040000\n" in text
    assert sorted(bvh["end_sites"]) == [3, 6, 10, 13, 16] and all(v == [0.0, 0.0, 0.0] for v in bvh["end_sites"].values())
    assert [bvh["parent"][k] for k in range(17)] == [int(sk.parent[k]) for k in order]
    assert np.abs(bvh["offset"] - ref["rest"][0][order] * scale).max() <= 0.5e-6 + 1e-12
    # the bar: %.6f of offsets and positions, and of angles in degrees (0.5e-6 degrees each)
    bar = _bvh_bar(sk, ref["rest"][0] * scale, np.radians(0.5e-6))
    got = bvh_reader.forward_kinematics(bvh)
    err = np.abs(np.linalg.norm(got - ref["P"][:, order] * scale, axis=2)).max()
    print(f"bvh round trip: max distance {err:.3e} file units, bar {bar:.3e}")
    assert err <= bar < 1e-4
    # a skeleton whose edge list is not depth first: the file's order is, and every name still appears once
    sk2 = K.Skeleton(((0, 1), (0, 2), (1, 3), (2, 4)), ("a", "b", "c", "d", "e"), (), np.tile([0.0, 1.0, 0.0], (5, 1)))
    assert sk2.hierarchy_order() == [0, 1, 3, 2, 4]
    b2 = bvh_reader.parse(K.bvh_text(sk2, np.arange(15.0).reshape(5, 3), np.zeros((2, 3)), np.zeros((2, 5, 3)), 30.0, 1.0))
    assert b2["names"] == ["a", "b", "d", "c", "e"] and b2["parent"] == [-1, 0, 1, 0, 3] and b2["offset"][2].tolist() == [9.0, 10.0, 11.0]
    for bad in (dict(fps=0.0), dict(scale=-1.0), dict(fps=float("nan"))):
        with pytest.raises(ValueError):
            K.bvh_text(sk, ref["rest"][0], ref["P"][:, 0], ref["euler"], **bad)
    with pytest.raises(ValueError):
        K.bvh_text(sk, ref["rest"][0], ref["P"][:3, 0], ref["euler"])


def test_write_bvh_and_the_dump_entry_point(tmp_path):
    """``python -m ...kinematics --npz`` on a dump that already holds the rotations needs no GPU: the file is the one ``write_bvh`` writes."""
    from implementation_phd_lab_vision_amd import kinematics as K
    x, seq_start, _ = KR.articulated(6, [4])
    ref = _h36m(x, seq_start)
    npz = tmp_path / "clip_poses.npz"
    np.savez(npz, joints3d=x, rotations_euler_zxy_deg=ref["euler"].astype(np.float32), rest_offsets=ref["rest"][0],
             joints3d_rigid=ref["rigid"].astype(np.float32))
    out = K.main(["--npz", str(npz), "--out", str(tmp_path / "clip.bvh"), "--bvh-fps", "50", "--bvh-scale", "1"])
    want = K.bvh_text(K.H36M_SKELETON, ref["rest"][0], ref["rigid"].astype(np.float32)[:, 0].astype(np.float64) * K.H36M_SKELETON.sign,
                      ref["euler"].astype(np.float32), 50.0, 1.0)
    assert Path(out).read_text() == want and "Frame Time: 0.020000" in want
    assert K.write_bvh(str(tmp_path / "b.bvh"), K.H36M_SKELETON, ref["rest"][0], ref["P"][:, 0], ref["euler"]) == str(tmp_path / "b.bvh")
    np.savez(tmp_path / "j5.npz", joints3d=np.zeros((3, 5, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="5 joints need a kinematics.Skeleton"):
        K.main(["--npz", str(tmp_path / "j5.npz"), "--out", str(tmp_path / "j5.bvh")])
    assert K.sequence_file_name((9, "Walking 1", "cam_2")) == "S9_Walking_1_cam_2.bvh"


def test_the_h36m_skeleton_is_the_documented_one_and_the_host_checks_refuse():
    from implementation_phd_lab_vision_amd import kinematics as K
    from implementation_phd_lab_vision_amd.train import H36M_EDGES
    sk = K.H36M_SKELETON
    assert tuple(map(tuple, sk.edges.tolist())) == tuple(H36M_EDGES) == KR.EDGES17 and sk.root == 0 and sk.joints == 17
    assert tuple(map(tuple, sk.frames.tolist())) == KR.FRAMES17 and np.array_equal(sk.rest_dirs, KR.rest_dirs17())
    assert tuple(sk.sign.tolist()) == KR.SIGN_H36M
    assert sk.names == ("Hips", "RightUpLeg", "RightLeg", "RightFoot", "LeftUpLeg", "LeftLeg", "LeftFoot", "Spine", "Spine1", "Neck", "Head",
                        "LeftArm", "LeftForeArm", "LeftHand", "RightArm", "RightForeArm", "RightHand")
    ok = dict(edges=((0, 1), (1, 2)), names=("a", "b", "c"), frames=(), rest_dirs=np.tile([0.0, 1.0, 0.0], (3, 1)), sign=(1.0, 1.0, 1.0))
    K.Skeleton(**ok)
    for kw in (dict(edges=((1, 2), (0, 1))), dict(edges=((0, 1),)), dict(names=("a", "a", "c")), dict(names=("a", "b c", "d")),
               dict(frames=((0, 1, 1, 0, 2),)), dict(frames=((0, 0, 1, 0, 3),)), dict(frames=((0, 0, 1, 0, 2), (0, 0, 2, 0, 1))),
               dict(rest_dirs=np.tile([0.0, 1.1, 0.0], (3, 1))), dict(rest_dirs=np.zeros((2, 3))), dict(sign=(1.0, -1.0, 1.0)),
               dict(sign=(1.0, 2.0, 0.5)), dict(sign=(1.0, 1.0))):
        with pytest.raises(ValueError):
            K.Skeleton(**dict(ok, **kw))
    with pytest.raises(ValueError, match="need a kinematics.Skeleton"):
        K.skeleton_for(16)
    with pytest.raises(ValueError, match="the skeleton has 17 joints"):
        K.skeleton_for(16, sk)
    import torch
    with pytest.raises(ValueError, match="no CPU fallback"):                    # poses on the host: refused, not computed there
        K.pose_rotations(torch.zeros(4, 17, 3), (np.array([0, 4]), np.arange(4)))
    with pytest.raises(ValueError, match="no CPU fallback"):
        K.rest_offsets(torch.zeros(4, 17, 3), (np.array([0, 4]), np.arange(4)))
    with pytest.raises(ValueError, match="keep_poses"):
        K.evaluate_rigid({"group_names": ["walk"]})


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = re.findall(r"^\s*(?:int|int64_t|size_t)\s+(r50_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    assert protos, "no prototypes parsed from include/r50_kinematics.h"
    return [(name, len([a for a in args.split(",") if a.strip()])) for name, args in protos]


def test_every_prototype_of_the_kinematics_header_is_bound_exported_and_guard_banded(lib_built):
    from implementation_phd_lab_vision_amd import _lib
    from tests.rows import kinematics as T
    protos = _prototypes()
    names = [n for n, _ in protos]
    assert set(names) == OPS == set(_lib._SIGNATURES_KINEMATICS) and len(names) == len(set(names))
    assert set(re.findall(r"\b(r50_op_[a-z0-9_]+)\s*\(", HEADER.read_text())) == OPS, "a name in a comment is a prototype too"
    covered = set()
    for row in T.ROWS_KINEMATICS:
        covered.update(row.ops)
    assert covered == OPS and len({row.id for row in T.ROWS_KINEMATICS}) == len(T.ROWS_KINEMATICS)
    others = [(ROOT / "include" / h).read_text() for h in ("r50.h", "r50_hal.h", "r50_smooth.h", "r50_multiview.h")]
    for name, arity in protos:
        assert len(_lib._SIGNATURES_KINEMATICS[name][1]) == arity, name
        assert hasattr(lib_built, name), f"{name} declared in r50_kinematics.h but not exported by libr50hip.so"
        assert getattr(lib_built, name).argtypes == _lib._SIGNATURES_KINEMATICS[name][1]
        assert not any(name in table for table in (_lib._SIGNATURES, _lib._SIGNATURES_HAL, _lib._SIGNATURES_SMOOTH, _lib._SIGNATURES_MULTIVIEW))
        assert name not in _lib.EXPORTED_SYMBOLS and not any(name in text for text in others)
    assert "r50_kinematics.h" in (ROOT / "implementation_phd_lab_vision_amd" / "_lib.py").read_text().split("def _source_digest")[1].split("def ")[0]
    abi = (ROOT / "implementation_phd_lab_vision_amd" / "csrc" / "r50_abi.hip").read_text()
    assert '#include "kinematics_kernels.h"' in abi and "r50_kinematics.h" in abi


def test_every_refusal_returns_before_any_launch(lib_built):
    """No device is needed: each call is refused on its arguments, with the op's name in the message.  The pointers are made-up addresses
    that nothing dereferences."""
    import ctypes
    from implementation_phd_lab_vision_amd import kinematics as K
    x, tab, rest, quat, euler, rigid, resid, flags = (0x100000 * k for k in range(1, 9))
    edges, e, frames, nf, dirs, sign = K.H36M_SKELETON.c_args()
    ints = lambda v: (ctypes.c_int * len(v))(*v)                                    # noqa: E731
    dbl = lambda v: (ctypes.c_double * len(v))(*v)                                  # noqa: E731
    bad_order = ints([1, 2, 0, 1] + list(edges)[4:])
    twice = ints([0, 1, 0, 1] + list(edges)[4:])
    frame_out = ints([0, 1, 4, 0, 17, 8, 14, 11, 8, 9])
    frame_same = ints([0, 1, 1, 0, 7, 8, 14, 11, 8, 9])
    frame_twice = ints([0, 1, 4, 0, 7, 0, 14, 11, 8, 9])
    not_unit = dbl([v * (1.001 if k == 3 else 1.0) for k, v in enumerate(dirs)])
    nan_dir = dbl([float("nan") if k == 4 else v for k, v in enumerate(dirs)])
    n_bytes = 12 * 17 * 3 * 4
    ok = dict(x=x, tab=tab, F=12, S=2, J=17, edges=edges, E=e, frames=frames, NF=nf, dirs=dirs, sign=sign, rest=rest, quat=quat, euler=euler,
              rigid=rigid, resid=resid, flags=flags)
    common = (dict(x=None), dict(tab=None), dict(edges=None), dict(frames=None), dict(dirs=None), dict(sign=None), dict(rest=None),
              dict(F=0), dict(F=-1), dict(F=2 ** 31 // 192 + 1), dict(S=0), dict(S=13), dict(J=0), dict(J=65), dict(E=15), dict(E=17),
              dict(edges=bad_order), dict(edges=twice), dict(NF=-1), dict(NF=18), dict(frames=frame_out), dict(frames=frame_same),
              dict(frames=frame_twice), dict(dirs=not_unit), dict(dirs=nan_dir), dict(sign=dbl([1.0, -1.0, 1.0])), dict(sign=dbl([1.0, 0.5, 2.0])),
              dict(sign=dbl([-1.0, -1.0, -1.0])), dict(sign=dbl([float("nan"), 1.0, 1.0])))

    def refused(name, rc, why):
        assert rc == -1, (name, why, rc)                                                # R50_ERR_INVALID: refused, not a launch that failed
        assert name.encode() in lib_built.r50_last_error(None), (name, why)

    for kw in common + (dict(rest=x), dict(rest=x + n_bytes - 8), dict(rest=tab)):
        a = dict(ok, **kw)
        refused("r50_op_rest_offsets", lib_built.r50_op_rest_offsets(a["x"], a["tab"], a["F"], a["S"], a["J"], a["edges"], a["E"], a["frames"],
                                                                     a["NF"], a["dirs"], a["sign"], a["rest"], None), kw)
    for kw in common + (dict(quat=None), dict(euler=None), dict(rigid=None), dict(resid=None), dict(flags=None), dict(quat=quat + 4),
                        dict(rigid=x), dict(quat=x + n_bytes - 16), dict(euler=rest), dict(resid=tab), dict(flags=resid), dict(euler=quat + 16),
                        dict(rigid=euler - n_bytes + 4)):
        a = dict(ok, **kw)
        refused("r50_op_pose_rotations",
                lib_built.r50_op_pose_rotations(a["x"], a["tab"], a["F"], a["S"], a["J"], a["edges"], a["E"], a["frames"], a["NF"], a["dirs"],
                                                a["sign"], a["rest"], a["quat"], a["euler"], a["rigid"], a["resid"], a["flags"], None), kw)


def test_parser_namespaces_without_the_new_flags_are_what_they_were(capsys):
    from implementation_phd_lab_vision_amd import predict, results
    base_p = ["--frames", "a.npy", "--model_path", "m", "--out", "o"]
    base_r = ["--features_root", "f", "--preprocessed_root", "v", "--model_path", "m"]
    assert sorted(vars(predict.parse_args(base_p))) == PREDICT_KEYS
    assert sorted(vars(results.parse_args(base_r))) == RESULTS_KEYS
    assert sorted(vars(results.parse_args(base_r + ["--dense"]))) == RESULTS_KEYS
    a = predict.parse_args(base_p + ["--bvh"])
    assert a.bvh is True and sorted(vars(a)) == sorted(PREDICT_KEYS + ["bvh"])
    a = predict.parse_args(base_p + ["--bvh", "--bvh-fps", "50", "--bvh-scale", "1"])
    assert (a.bvh_fps, a.bvh_scale) == (50.0, 1.0)
    a = results.parse_args(base_r + ["--dense", "--dense-rigid"])
    assert a.dense_rigid is True and sorted(vars(a)) == sorted(RESULTS_KEYS + ["dense_rigid"])
    a = results.parse_args(base_r + ["--dense", "--dense-rigid", "--dense-bvh", "d", "--bvh-fps", "30"])
    assert a.dense_bvh == "d" and a.bvh_fps == 30.0 and not hasattr(a, "bvh_scale")
    for bad in (["--bvh-fps", "50"], ["--bvh-scale", "1"], ["--bvh", "--bvh-fps", "0"], ["--bvh", "--bvh-scale", "nan"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base_p + bad)
    for bad in (["--dense-rigid"], ["--dense", "--dense-bvh", "d"], ["--dense", "--dense-rigid", "--bvh-fps", "30"],
                ["--dense", "--dense-rigid", "--dense-bvh", "d", "--bvh-scale", "0"]):
        with pytest.raises(SystemExit):
            results.parse_args(base_r + bad)
    assert "--dense-rigid needs --dense" in capsys.readouterr().err


def test_the_product_never_imports_the_oracle():
    pkg = ROOT / "implementation_phd_lab_vision_amd"
    for path in [pkg / "kinematics.py", pkg / "predict.py", pkg / "results.py", ROOT / "scripts" / "bench_kinematics.py"]:
        text = path.read_text()
        assert "kinematics_reference" not in text and "bvh_reader" not in text and "from tests" not in text and "import tests" not in text, path
