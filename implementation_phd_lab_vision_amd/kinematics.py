"""Joint rotations on a rigid skeleton and BVH export for per-frame pose sequences (include/r50_kinematics.h).

``predict`` and ``results --dense`` end in joint positions; animation tools, game engines, retargeting and physics take joint rotations
on a rigid skeleton.  This module is the inverse-kinematics pass between the two, on the device where the poses already sit:

* ``Skeleton`` / ``H36M_SKELETON``: the edge list, the joint names, the joints whose orientation the positions determine in full
  (``frames``) and a rest direction for every other bone (``rest_dirs``), with the sign flips that take the poses to the BVH world
  (y up, the figure's left along +x, facing +z);
* ``rest_offsets`` (``r50_op_rest_offsets``): a rest pose per sequence, fp64;
* ``pose_rotations`` (``r50_op_pose_rotations``): per frame a local rotation per joint (quaternion and Z-X-Y Euler angles), the rigid
  reconstruction they imply, its mean distance from the input and the flags of the degenerate cases;
* ``bvh_text`` / ``write_bvh``: pure host code;
* ``evaluate_rigid``: what the rigid skeleton costs in accuracy, on a ``sequences.evaluate_dense(keep_poses=True)`` result.

fp32 in and out, fp64 in between, one rounding at the store, the same bits on every run.  No CPU fallback.

    python -m implementation_phd_lab_vision_amd.kinematics --npz NAME_poses.npz --out NAME.bvh [--bvh-fps 25 --bvh-scale 100]
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .smooth import DeviceTables, _check_poses, _stream, check_edges
from .train import H36M_EDGES

MAX_JOINTS = 64
FLAG_FRAME, FLAG_REACH, FLAG_ANTIPARALLEL = 1, 2, 4       # bits of ``flags``: a degenerate frame row, a child on the joint, an aim turned round
FLAG_NAMES = ("degenerate frame", "child on the joint", "antiparallel aim")
BVH_FPS, BVH_SCALE = 25.0, 100.0                           # 50 Hz over FRAME_SKIP = 2; metres to centimetres


class Skeleton:
    """``edges`` (J-1, 2) parent before child, checked as ``smooth.check_edges`` does, spanning all J = ``len(names)`` joints (the joint
    that is nobody's child is the root); ``frames`` rows ``(joint, a0, a1, b0, b1)``; ``rest_dirs`` (J, 3) unit vectors (the root's is
    not read); ``sign`` (3,) of +-1 with product +1, applied to the positions on load."""

    def __init__(self, edges, names: Sequence[str], frames, rest_dirs, sign=(1.0, 1.0, 1.0)):
        self.names = tuple(str(n) for n in names)
        j = len(self.names)
        if not 2 <= j <= MAX_JOINTS or len(set(self.names)) != j or any((not n) or any(c.isspace() for c in n) for n in self.names):
            raise ValueError(f"names must be 2 to {MAX_JOINTS} different words without blanks")
        self.edges = check_edges(edges, j)
        if self.edges.shape[0] != j - 1:
            raise ValueError(f"a skeleton of {j} joints needs {j - 1} edges (one root), got {self.edges.shape[0]}")
        self.joints = j
        self.root = int((set(range(j)) - set(self.edges[:, 1].tolist())).pop())
        fr = np.asarray(frames if len(frames) else np.zeros((0, 5)), dtype=np.int64)
        if fr.ndim != 2 or fr.shape[1] != 5 or fr.shape[0] > j:
            raise ValueError(f"frames must be (NF, 5) rows (joint, a0, a1, b0, b1), got {fr.shape}")
        if fr.size and (fr.min() < 0 or fr.max() >= j):
            raise ValueError(f"every frame index must lie in [0, {j})")
        if np.any(fr[:, 1] == fr[:, 2]) or np.any(fr[:, 3] == fr[:, 4]) or len(set(fr[:, 0].tolist())) != fr.shape[0]:
            raise ValueError("a frame row needs a0 != a1 and b0 != b1, and a joint is framed once only")
        self.frames = np.ascontiguousarray(fr, dtype=np.int32)
        d = np.ascontiguousarray(rest_dirs, dtype=np.float64)
        if d.shape != (j, 3):
            raise ValueError(f"rest_dirs must be ({j}, 3), got {d.shape}")
        others = np.arange(j) != self.root
        if not np.all(np.abs((d[others] ** 2).sum(axis=1) - 1.0) <= 1e-12):
            raise ValueError("rest_dirs must hold a unit vector for every joint but the root")
        self.rest_dirs = d
        s = np.ascontiguousarray(sign, dtype=np.float64)
        if s.shape != (3,) or not np.all(np.abs(s) == 1.0) or s.prod() != 1.0:
            raise ValueError(f"sign must be three values of +1 or -1 whose product is +1, got {sign!r}")
        self.sign = s
        self.parent = np.full(j, -1, dtype=np.int64)
        self.parent[self.edges[:, 1]] = self.edges[:, 0]
        self.children: List[List[int]] = [[int(c) for p, c in self.edges if p == k] for k in range(j)]

    def c_args(self):
        """(edges, E, frames, NF, rest_dirs, sign) as the ABI takes them: host arrays."""
        e, f = self.edges.reshape(-1), self.frames.reshape(-1)
        return ((ctypes.c_int * e.size)(*e.tolist()), int(self.edges.shape[0]), (ctypes.c_int * max(f.size, 1))(*f.tolist()),
                int(self.frames.shape[0]), (ctypes.c_double * (3 * self.joints))(*self.rest_dirs.reshape(-1).tolist()),
                (ctypes.c_double * 3)(*self.sign.tolist()))

    def hierarchy_order(self) -> List[int]:
        """The joints depth first from the root, the children of a joint in edge order: the order of a BVH file."""
        out, stack = [], [self.root]
        while stack:
            k = stack.pop()
            out.append(k)
            stack.extend(reversed(self.children[k]))
        return out


def _h36m_rest_dirs() -> np.ndarray:
    d = np.zeros((17, 3))
    d[[1, 14, 15, 16]] = (-1.0, 0.0, 0.0)
    d[[4, 11, 12, 13]] = (1.0, 0.0, 0.0)
    d[[2, 3, 5, 6]] = (0.0, -1.0, 0.0)
    d[[7, 8, 9, 10]] = (0.0, 1.0, 0.0)
    return d


H36M_NAMES = ("Hips", "RightUpLeg", "RightLeg", "RightFoot", "LeftUpLeg", "LeftLeg", "LeftFoot", "Spine", "Spine1", "Neck", "Head", "LeftArm",
              "LeftForeArm", "LeftHand", "RightArm", "RightForeArm", "RightHand")
# camera coordinates (y down, z away from the camera) -> y up, facing +z: a half turn about x
H36M_SKELETON = Skeleton(H36M_EDGES, H36M_NAMES, ((0, 1, 4, 0, 7), (8, 14, 11, 8, 9)), _h36m_rest_dirs(), (1.0, -1.0, -1.0))


def skeleton_for(joints: int, skeleton: Optional[Skeleton] = None) -> Skeleton:
    """``skeleton``, or ``H36M_SKELETON`` for 17 joints; any other count without a skeleton is refused."""
    if skeleton is None:
        if int(joints) != H36M_SKELETON.joints:
            raise ValueError(f"poses of {joints} joints need a kinematics.Skeleton of their own: only the {H36M_SKELETON.joints}-joint "
                             "Human3.6M skeleton is built in")
        skeleton = H36M_SKELETON
    if skeleton.joints != int(joints):
        raise ValueError(f"the skeleton has {skeleton.joints} joints, the poses {joints}")
    return skeleton


@dataclass
class Rotations:
    """What ``pose_rotations`` returns, on the device: ``quat`` (F, J, 4) (w, x, y, z) and ``euler`` (F, J, 3) degrees (Z, X, Y) of the
    local rotations, ``rigid`` (F, J, 3) the rigid reconstruction in the input's frame, ``resid`` (F,) its mean distance from the input,
    ``flags`` (F,) int32 (``FLAG_*``) and the ``rest`` (S, J, 3) fp64 offsets that were used."""
    quat: torch.Tensor
    euler: torch.Tensor
    rigid: torch.Tensor
    resid: torch.Tensor
    flags: torch.Tensor
    rest: torch.Tensor


def rest_offsets(x: torch.Tensor, tables, skeleton: Optional[Skeleton] = None) -> torch.Tensor:
    """One ``r50_op_rest_offsets`` launch: ``rest (S, J, 3)`` fp64 on the device, the rest pose of every sequence in the world frame."""
    tables = DeviceTables.of(tables, x.device)
    f, j = _check_poses(x, tables, "rest_offsets")
    sk = skeleton_for(j, skeleton)
    rest = torch.empty((tables.sequences, j, 3), dtype=torch.float64, device=x.device)
    rc = _lib.load_library().r50_op_rest_offsets(x.data_ptr(), tables.seq_start.data_ptr(), f, tables.sequences, j, *sk.c_args(), rest.data_ptr(),
                                                 _stream(x))
    _lib.check(rc, None, "r50_op_rest_offsets")
    return rest


def pose_rotations(x: torch.Tensor, tables, skeleton: Optional[Skeleton] = None, rest: Optional[torch.Tensor] = None) -> Rotations:
    """``r50_op_pose_rotations`` on x (F, J, 3) fp32 with the rest offsets ``rest`` (by default those of x: ``rest_offsets`` first)."""
    tables = DeviceTables.of(tables, x.device)
    f, j = _check_poses(x, tables, "pose_rotations")
    sk = skeleton_for(j, skeleton)
    if rest is None:
        rest = rest_offsets(x, tables, sk)
    if rest.dtype != torch.float64 or tuple(rest.shape) != (tables.sequences, j, 3) or rest.device != x.device or not rest.is_contiguous():
        raise ValueError(f"rest must be a contiguous ({tables.sequences}, {j}, 3) fp64 tensor on {x.device}")
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=x.device)          # noqa: E731
    out = Rotations(new((f, j, 4)), new((f, j, 3)), new((f, j, 3)), new((f,)), new((f,), torch.int32), rest)
    rc = _lib.load_library().r50_op_pose_rotations(x.data_ptr(), tables.row_seq.data_ptr(), f, tables.sequences, j, *sk.c_args(), rest.data_ptr(),
                                                   out.quat.data_ptr(), out.euler.data_ptr(), out.rigid.data_ptr(), out.resid.data_ptr(),
                                                   out.flags.data_ptr(), _stream(x))
    _lib.check(rc, None, "r50_op_pose_rotations")
    return out


# ---- BVH: pure host code ------------------------------------------------------------------------------------------------------------------
def bvh_text(skeleton: Skeleton, rest, root_xyz, euler_deg, fps: float = BVH_FPS, scale: float = BVH_SCALE) -> str:
    """A BVH file as text.  ``rest`` (J, 3) the offsets of one sequence and ``root_xyz`` (N, 3) the root's positions, both in the world
    frame; ``euler_deg`` (N, J, 3) degrees (Z, X, Y) per joint in joint order.  HIERARCHY: ``OFFSET`` = rest * scale as %.6f, the root
    with six channels (position, then Z, X, Y rotation), every other joint with the three rotations, a leaf as a JOINT with an End Site
    of offset 0 (so that all J names appear).  MOTION: one line per frame, the root's position * scale, then the angles in hierarchy
    order."""
    rest, root_xyz, euler_deg = np.asarray(rest, dtype=np.float64), np.asarray(root_xyz, dtype=np.float64), np.asarray(euler_deg, dtype=np.float64)
    j = skeleton.joints
    n = int(euler_deg.shape[0]) if euler_deg.ndim == 3 else -1
    if rest.shape != (j, 3) or euler_deg.shape != (n, j, 3) or root_xyz.shape != (n, 3) or n < 1:
        raise ValueError(f"rest ({j}, 3), root_xyz (N, 3) and euler_deg (N, {j}, 3) expected, got {rest.shape}, {root_xyz.shape}, {euler_deg.shape}")
    fps, scale = float(fps), float(scale)
    if not (math.isfinite(fps) and fps > 0.0 and math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"fps and scale must be positive and finite, got {fps}, {scale}")
    if not (np.isfinite(rest).all() and np.isfinite(root_xyz).all() and np.isfinite(euler_deg).all()):
        raise ValueError("rest, root_xyz and euler_deg must be finite")
    lines = ["HIERARCHY"]

    def node(k: int, depth: int) -> None:
        pad = "  " * depth
        lines.append(f"{pad}{'ROOT' if k == skeleton.root else 'JOINT'} {skeleton.names[k]}")
        lines.append(pad + "{")
        o = rest[k] * scale
        lines.append(f"{pad}  OFFSET {o[0]:.6f} {o[1]:.6f} {o[2]:.6f}")
        if k == skeleton.root:
            lines.append(f"{pad}  CHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation")
        else:
            lines.append(f"{pad}  CHANNELS 3 Zrotation Xrotation Yrotation")
        for c in skeleton.children[k]:
            node(c, depth + 1)
        if not skeleton.children[k]:
            lines.extend([f"{pad}  End Site", pad + "  {", f"{pad}    OFFSET {0.0:.6f} {0.0:.6f} {0.0:.6f}", pad + "  }"])
        lines.append(pad + "}")

    node(skeleton.root, 0)
    order = skeleton.hierarchy_order()
    lines += ["MOTION", f"Frames: {n}", f"Frame Time: {1.0 / fps:.6f}"]
    body = np.concatenate([root_xyz * scale, euler_deg[:, order].reshape(n, -1)], axis=1)
    lines += [" ".join(f"{v:.6f}" for v in row) for row in body]
    return "\n".join(lines) + "\n"


def write_bvh(path: str, skeleton: Skeleton, rest, root_xyz, euler_deg, fps: float = BVH_FPS, scale: float = BVH_SCALE) -> str:
    text = bvh_text(skeleton, rest, root_xyz, euler_deg, fps, scale)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def video_rotations(joints3d: np.ndarray, device, skeleton: Optional[Skeleton] = None) -> Dict[str, np.ndarray]:
    """The poses of one video (N, J, 3) as one sequence of one segment through both ops; host arrays under the keys ``predict --bvh``
    adds to its ``.npz``.  The skeleton is checked before anything is uploaded."""
    x = np.ascontiguousarray(joints3d, dtype=np.float32)
    if x.ndim != 3 or x.shape[2] != 3 or x.shape[0] < 1:
        raise ValueError(f"poses (N, J, 3) expected, got {x.shape}")
    sk = skeleton_for(x.shape[1], skeleton)
    n = int(x.shape[0])
    device = torch.device(device)
    with torch.cuda.device(device):
        xd = torch.from_numpy(x).to(device)
        rot = pose_rotations(xd, (np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32)), sk)
        return {"rotations_quat": rot.quat.cpu().numpy(), "rotations_euler_zxy_deg": rot.euler.cpu().numpy(),
                "rest_offsets": rot.rest[0].cpu().numpy(), "joints3d_rigid": rot.rigid.cpu().numpy(), "rigid_residual": rot.resid.cpu().numpy(),
                "rigid_flags": rot.flags.cpu().numpy()}


def write_video_bvh(path: str, res: Dict[str, np.ndarray], skeleton: Optional[Skeleton] = None, fps: float = BVH_FPS,
                    scale: float = BVH_SCALE) -> str:
    """The BVH file of a ``video_rotations`` result (or of the ``.npz`` that holds one)."""
    rigid = np.asarray(res["joints3d_rigid"], dtype=np.float64)
    sk = skeleton_for(rigid.shape[1], skeleton)
    return write_bvh(path, sk, res["rest_offsets"], rigid[:, sk.root] * sk.sign, res["rotations_euler_zxy_deg"], fps, scale)


# ---- what a rigid skeleton costs: the dense pass ------------------------------------------------------------------------------------------
@torch.no_grad()
def evaluate_rigid(dense: Dict[str, object], skeleton: Optional[Skeleton] = None, device="cuda", chunk_rows: int = 1 << 20,
                   keep: bool = False) -> Dict[str, object]:
    """``dense`` is the result of ``sequences.evaluate_dense(keep_poses=True)``; its ``pred_post`` where a post-process ran, else its
    ``pred``, goes through both ops in runs of whole sequences of at most ``chunk_rows`` rows (a longer sequence is a run of its own),
    and the rigid poses are scored against ``gt`` by the metrics and protocols launches of ``evaluate_dense`` (the residual rides in the
    spread slot); the sums are read once.  Returns (metres; fp64), for M in ``p1``, ``p2``, ``mpjve``, ``accel``::

        rigid_M (G,), rigid_M_all, rigid_M_mean      beside M (or post_M) of ``dense``
        rigid_residual (G,), rigid_residual_all       the mean of ``resid``
        rigid_flagged (3,) int64                      frames with flag bit 0, 1, 2 set
        with keep: rigid (F, J, 3), euler (F, J, 3), rest (S, J, 3), resid (F,), flags (F,)
    """
    from . import protocols, sequences
    missing = [k for k in ("seq_keys", "seq_start", "frame_idx", "pred", "gt", "group_names", "count") if k not in dense]
    if missing:
        raise ValueError(f"the dense result lacks {missing}: run evaluate_dense with keep_poses=True")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("evaluate_rigid runs on a GPU: there is no CPU fallback")
    single = np.ascontiguousarray(dense["pred_post"] if "pred_post" in dense else dense["pred"], dtype=np.float32)
    f, joints = int(single.shape[0]), int(single.shape[1])
    sk = skeleton_for(joints, skeleton)
    seq_keys, seq_start, frame_idx = dense["seq_keys"], np.asarray(dense["seq_start"]).astype(np.int64), np.asarray(dense["frame_idx"])
    group_names = list(dense["group_names"])
    gpos = {a: g for g, a in enumerate(group_names)}
    seq_group = np.array([gpos[protocols.action_name(k[1])] for k in seq_keys], dtype=np.int32)
    n_groups, n_seq = len(group_names), len(seq_keys)
    runs, s0 = [], 0
    for s in range(1, n_seq + 1):                                                   # whole sequences, at most chunk_rows rows a run
        if s == n_seq or seq_start[s + 1] - seq_start[s0] > int(chunk_rows):
            runs.append((s0, s))
            s0 = s
    with torch.cuda.device(device):
        pred = torch.from_numpy(single).to(device)
        gt = torch.from_numpy(np.ascontiguousarray(dense["gt"], dtype=np.float32)).to(device)
        rigid, euler = torch.empty_like(pred), torch.empty_like(pred)
        resid = torch.empty(f, dtype=torch.float32, device=device)
        flags = torch.empty(f, dtype=torch.int32, device=device)
        rest = torch.empty((n_seq, joints, 3), dtype=torch.float64, device=device)
        for a, b in runs:
            r0, r1 = int(seq_start[a]), int(seq_start[b])
            tables = ((seq_start[a:b + 1] - r0).astype(np.int32), frame_idx[r0:r1].astype(np.int32))
            rot = pose_rotations(pred[r0:r1], tables, sk)
            rigid[r0:r1], euler[r0:r1], resid[r0:r1], flags[r0:r1], rest[a:b] = rot.rigid, rot.euler, rot.resid, rot.flags, rot.rest
        seq = np.repeat(np.arange(n_seq, dtype=np.int32), np.diff(seq_start))
        group = torch.from_numpy(seq_group[seq]).to(device)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(np.asarray(dense["count"]), dtype=np.int64)]).astype(np.int32)).to(device)
        part = sequences.sequence_metrics(rigid, gt, resid, offsets, torch.from_numpy(seq).to(device),
                                          torch.from_numpy(np.ascontiguousarray(frame_idx, dtype=np.int32)).to(device), group, n_groups)
        acc_p2 = torch.zeros(3 * n_groups, dtype=torch.float64, device=device)
        protocols._launch(rigid.view(f, 1, joints, 3), gt.view(f, 1, joints, 3), 0, group, n_groups, acc_p2, protocols.ROOT_JOINT)
        bits = torch.stack([((flags >> k) & 1).sum() for k in range(3)]).to(torch.float64)
        host = torch.cat([acc_p2, part.reshape(-1), bits]).cpu().numpy()
        kept = {"rigid": rigid.cpu().numpy(), "euler": euler.cpu().numpy(), "rest": rest.cpu().numpy(), "resid": resid.cpu().numpy(),
                "flags": flags.cpu().numpy()} if keep else {}
    p2, part, bits = np.split(host, [3 * n_groups, host.size - 3])
    vals = sequences.metric_values(sequences.sum_blocks(part.reshape(-1, n_groups, sequences.METRIC_SLOTS)),
                                   p2[:2 * n_groups].reshape(n_groups, 2)[:, 1])
    out: Dict[str, object] = dict(kept)
    for m in ("p1", "p2", "mpjve", "accel"):
        for suffix in ("", "_all", "_mean"):
            out["rigid_" + m + suffix] = vals[m + suffix]
    out["rigid_residual"], out["rigid_residual_all"] = vals["spread"], vals["spread_all"]
    out["rigid_flagged"] = bits.round().astype(np.int64)
    return out


def rigid_lines(dense: Dict[str, object], res: Dict[str, object]) -> List[str]:
    """The ``Dense | rigid`` lines: raw -> rigid over all frames and per action (mm), the residual and the flagged frames."""
    single = "post_" if "pred_post" in dense else ""

    def pair(m: str, key: str, i=None) -> str:
        a, b = dense[single + m + key], res["rigid_" + m + key]
        a, b = (a, b) if i is None else (a[i], b[i])
        return f"{a * 1000.0:.2f} -> {b * 1000.0:.2f}"

    def row(key: str, i=None) -> str:
        d = res["rigid_residual" + key]
        d = d if i is None else d[i]
        return (f"p1 (mm) {pair('p1', key, i)} | p2 (mm) {pair('p2', key, i)} | vel (mm/frame) {pair('mpjve', key, i)} | accel (mm/frame^2) "
                f"{pair('accel', key, i)} | residual (mm) {d * 1000.0:.2f}")

    lines = ["Dense | rigid skeleton (joint rotations, section Y) | flagged frames " +
             ", ".join(f"{name} {int(n)}" for name, n in zip(FLAG_NAMES, res["rigid_flagged"])) + f" | raw -> rigid, all: {row('_all')}"]
    for i, name in enumerate(dense["group_names"]):
        lines.append(f"Dense | rigid   {name} | {row('', i)}")
    return lines


def rigid_npz(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``dense_rigid_*`` keys of the result ``.npz``: ``dense_rigid_M`` (G,) and ``dense_rigid_M_all`` () fp32 for M in p1, p2, mpjve,
    accel, residual; ``dense_rigid_flagged`` (3,) int64."""
    out = {"dense_rigid_flagged": np.asarray(res["rigid_flagged"], dtype=np.int64)}
    for m in ("p1", "p2", "mpjve", "accel", "residual"):
        out["dense_rigid_" + m] = np.asarray(res["rigid_" + m], dtype=np.float32)
        out["dense_rigid_" + m + "_all"] = np.asarray(res["rigid_" + m + "_all"], dtype=np.float32)
    return out


def sequence_file_name(key) -> str:
    """``S9_Walking_1_cam.bvh`` of a sequence key (subject, action, camera)."""
    word = "_".join(str(v) for v in key)
    return "S" + "".join(c if c.isalnum() or c in "-_." else "_" for c in word) + ".bvh"


def write_dense_bvh(outdir: str, dense: Dict[str, object], res: Dict[str, object], skeleton: Optional[Skeleton] = None, fps: float = BVH_FPS,
                    scale: float = BVH_SCALE) -> List[str]:
    """One BVH file per sequence key of an ``evaluate_rigid(keep=True)`` result."""
    import os
    sk = skeleton_for(res["rigid"].shape[1], skeleton)
    os.makedirs(outdir, exist_ok=True)
    seq_start, written = np.asarray(dense["seq_start"]), []
    for s, key in enumerate(dense["seq_keys"]):
        r0, r1 = int(seq_start[s]), int(seq_start[s + 1])
        root = res["rigid"][r0:r1, sk.root].astype(np.float64) * sk.sign
        written.append(write_bvh(os.path.join(outdir, sequence_file_name(key)), sk, res["rest"][s], root, res["euler"][r0:r1], fps, scale))
    return written


def add_bvh_flags(parser) -> None:
    """``--bvh-fps`` and ``--bvh-scale``; absent from the namespace unless given."""
    import argparse
    parser.add_argument("--bvh-fps", type=float, default=argparse.SUPPRESS, help=f"frames per second of the BVH files (default {BVH_FPS})")
    parser.add_argument("--bvh-scale", type=float, default=argparse.SUPPRESS,
                        help=f"BVH units per unit of the poses (default {BVH_SCALE}: metres to centimetres)")


def bvh_options(args, error) -> Tuple[float, float]:
    fps, scale = float(getattr(args, "bvh_fps", BVH_FPS)), float(getattr(args, "bvh_scale", BVH_SCALE))
    if not (math.isfinite(fps) and fps > 0.0 and math.isfinite(scale) and scale > 0.0):
        error(f"--bvh-fps and --bvh-scale must be positive and finite, got {fps}, {scale}")
    return fps, scale


def main(argv: Optional[List[str]] = None) -> str:
    """A ``NAME_poses.npz`` written earlier by ``predict`` to a BVH file: its ``joints3d`` go through both ops again (on the GPU), unless
    the file already holds the rotations (``predict --bvh``)."""
    import argparse
    p = argparse.ArgumentParser("Joint rotations and a BVH file from a poses dump")
    p.add_argument("--npz", type=str, required=True, help="NAME_poses.npz of predict (joints3d (N, 17, 3))")
    p.add_argument("--out", type=str, required=True, metavar="FILE.bvh")
    p.add_argument("--device", type=str, default="cuda")
    add_bvh_flags(p)
    args = p.parse_args(argv)
    fps, scale = bvh_options(args, p.error)
    z = np.load(args.npz, allow_pickle=False)
    if "rotations_euler_zxy_deg" in z.files:
        res = {k: z[k] for k in ("rotations_euler_zxy_deg", "rest_offsets", "joints3d_rigid")}
    else:
        if "joints3d" not in z.files:
            raise ValueError(f"{args.npz}: no `joints3d` array in the file (it holds {sorted(z.files)})")
        skeleton_for(z["joints3d"].shape[1])
        device = torch.device(args.device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.R50Error("the rotations are computed on an MI355X only; there is no CPU fallback")
        res = video_rotations(z["joints3d"], device)
        print(f"{args.npz}: mean rigid residual {float(res['rigid_residual'].mean()):.6f}, flagged frames "
              f"{int(np.count_nonzero(res['rigid_flags']))} of {res['rigid_flags'].size}")
    out = write_video_bvh(args.out, res, None, fps, scale)
    print(f"BVH written to: {out}")
    return out


if __name__ == "__main__":
    main()
