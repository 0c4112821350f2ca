"""2D-guided refinement of stitched per-frame pose sequences (include/r50_refine.h).

``results --dense`` and ``predict`` end in one 3D pose per video frame that the head lifted from image features; 2D detections of the same
frames are at hand in both (``joints2d`` and the camera).  This module fits the lifted sequence to them under a temporal and a skeletal
prior, on the device where the stitched poses already sit, between the stitch and the post-process:

* ``rays_from_pixels`` turns pixels and a camera into normalised image coordinates, which do not depend on a crop;
* ``fit_sweeps`` / ``fit_energy`` are the two ops (``r50_op_pose_fit_sweeps``, ``r50_op_pose_fit_energy``);
* ``RefineSettings`` bundles the weights; ``refine_sequences`` runs energy, sweeps, energy without a host round trip;
* ``dense_rays`` / ``evaluate_refine`` / ``refine_lines`` / ``refine_npz`` / ``refine_export`` are the ``results --dense --dense-refine`` pass.

fp32 in and out, fp64 in between, one rounding at the store, the same bits on every run.  No CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .smooth import DeviceTables, _check_poses, _edge_array, _stream, bone_stats, check_edges
from .train import H36M_EDGES

ENERGY_SLOTS = 6            # r50_op_pose_fit_energy: [e2d, e3d, eacc, ebone, sum of conf over the included (t, j), skipped (t, j)]
MAX_ITERS = 1000
MAX_OMEGA = 0.75


def _intrinsics(cam) -> Tuple[np.ndarray, np.ndarray]:
    """``(f (..., 2), c (..., 2))`` fp64 of a camera given as K (..., 3, 3) or as a pair ``(f, c)``."""
    if isinstance(cam, (tuple, list)) and len(cam) == 2:
        f, c = (np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1) for v in cam)
        if f.size != 2 or c.size != 2:
            raise ValueError(f"the camera's f and c must hold two values each, got {f.size} and {c.size}")
    else:
        k = np.asarray(cam.detach().cpu().numpy() if isinstance(cam, torch.Tensor) else cam, dtype=np.float64)
        if k.ndim < 2 or k.shape[-2:] != (3, 3):
            raise ValueError(f"the camera must be K (..., 3, 3) or a pair (f, c), got an array of shape {k.shape}")
        if np.any(k[..., 0, 1] != 0.0) or np.any(k[..., 1, 0] != 0.0):
            raise ValueError("K has skew (K[0][1] or K[1][0] is not 0): normalised coordinates would need its inverse")
        if np.any(k[..., 2, :] != np.array([0.0, 0.0, 1.0])):
            raise ValueError("the last row of K must be [0, 0, 1]")
        f, c = np.stack([k[..., 0, 0], k[..., 1, 1]], axis=-1), np.stack([k[..., 0, 2], k[..., 1, 2]], axis=-1)
    if not (np.isfinite(f).all() and np.isfinite(c).all() and np.all(f > 0.0)):
        raise ValueError("the camera needs finite focal lengths > 0 and a finite principal point")
    return f, c


def rays_from_pixels(joints2d, cam) -> np.ndarray:
    """``((u - cx) / fx, (v - cy) / fy)`` in fp64, rounded once to fp32: joints2d (..., J, 2) pixels; ``cam`` a K (3, 3), a K per leading
    index (B, 3, 3) for joints2d (B, ..., J, 2), or a pair ``(f, c)``.  A K with skew or a last row other than [0, 0, 1] is refused."""
    uv = np.asarray(joints2d.detach().cpu().numpy() if isinstance(joints2d, torch.Tensor) else joints2d, dtype=np.float64)
    if uv.ndim < 2 or uv.shape[-1] != 2:
        raise ValueError(f"joints2d (..., J, 2) expected, got {uv.shape}")
    f, c = _intrinsics(cam)
    if f.ndim > 1:
        if f.ndim != 2 or uv.ndim < 3 or f.shape[0] != uv.shape[0]:
            raise ValueError(f"{f.shape[:-1]} cameras do not go with joints2d of shape {uv.shape}")
        shape = (f.shape[0],) + (1,) * (uv.ndim - 2) + (2,)
        f, c = f.reshape(shape), c.reshape(shape)
    return np.ascontiguousarray(((uv - c) / f).astype(np.float32))


@dataclass
class RefineSettings:
    """The weights of the fit (include/r50_refine.h), checked when the object is made: ``iters`` sweeps of step ``omega`` on
    ``lambda_2d`` reprojection + ``lambda_3d`` distance to the prediction + ``lambda_acc`` second differences + ``lambda_bone`` bone
    lengths over ``edges``.  A bone term whose lengths come from a biased prediction makes the result worse, so its default weight is 0."""
    iters: int = 50
    lambda_2d: float = 1.0
    lambda_3d: float = 1.0
    lambda_acc: float = 1.0
    lambda_bone: float = 0.0
    omega: float = 0.6
    z_min: float = 0.1
    edges: Sequence[Sequence[int]] = H36M_EDGES

    def __post_init__(self):
        if int(self.iters) != self.iters or not 0 <= int(self.iters) <= MAX_ITERS:
            raise ValueError(f"iters must be an integer in [0, {MAX_ITERS}], got {self.iters!r}")
        self.iters = int(self.iters)
        for name in ("lambda_2d", "lambda_3d", "lambda_acc", "lambda_bone", "omega", "z_min"):
            setattr(self, name, float(getattr(self, name)))
        if not (math.isfinite(self.lambda_3d) and self.lambda_3d > 0.0):
            raise ValueError(f"lambda_3d must be finite and > 0 (it keeps every 3x3 system positive definite), got {self.lambda_3d}")
        for name in ("lambda_2d", "lambda_acc", "lambda_bone"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        if not 0.0 < self.omega <= MAX_OMEGA:
            raise ValueError(f"omega must lie in (0, {MAX_OMEGA}]: a larger step does not descend, got {self.omega}")
        if not (math.isfinite(self.z_min) and self.z_min > 0.0):
            raise ValueError(f"z_min must be finite and > 0, got {self.z_min}")
        if self.lambda_bone != 0.0:             # the order and uniqueness of the list; the joint count is checked against the poses later
            e = np.asarray(self.edges)
            check_edges(e, int(e.max()) + 1 if e.size and e.ndim == 2 else 0)

    def describe(self) -> str:
        s = (f"2D fit iters={self.iters} omega={self.omega:g} lambda 2d={self.lambda_2d:g} 3d={self.lambda_3d:g} acc={self.lambda_acc:g} "
             f"bone={self.lambda_bone:g} z_min={self.z_min:g}")
        return s + (f" over {len(self.edges)} edges (per-sequence mean length)" if self.lambda_bone != 0.0 else "")


def _check_side(x: torch.Tensor, rays: torch.Tensor, conf: Optional[torch.Tensor], what: str) -> None:
    f, j = int(x.shape[0]), int(x.shape[1])
    if rays.dtype != torch.float32 or tuple(rays.shape) != (f, j, 2) or rays.device != x.device or not rays.is_contiguous():
        raise ValueError(f"{what}: rays must be a contiguous ({f}, {j}, 2) fp32 tensor on {x.device}, got {tuple(rays.shape)} {rays.dtype}")
    if conf is not None and (conf.dtype != torch.float32 or tuple(conf.shape) != (f, j) or conf.device != x.device or not conf.is_contiguous()):
        raise ValueError(f"{what}: conf must be a contiguous ({f}, {j}) fp32 tensor on {x.device}, got {tuple(conf.shape)} {conf.dtype}")


def _edge_args(edges, joints: int, bone_len: Optional[torch.Tensor], sequences: int, device, what: str):
    """``(edge array or None, E, bone_len pointer)`` of an optional bone term."""
    if bone_len is None:
        return None, 0, None
    e = check_edges(edges, joints)
    if (bone_len.dtype != torch.float64 or tuple(bone_len.shape) != (sequences, e.shape[0]) or bone_len.device != device
            or not bone_len.is_contiguous()):
        raise ValueError(f"{what}: bone_len must be a contiguous ({sequences}, {e.shape[0]}) fp64 tensor on {device}")
    return _edge_array(e), int(e.shape[0]), bone_len.data_ptr()


def fit_energy(x: torch.Tensor, x0: torch.Tensor, rays: torch.Tensor, conf: Optional[torch.Tensor], tables: DeviceTables, z_min: float = 0.1,
               edges=None, bone_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``r50_op_pose_fit_energy`` launch: ``energy (S, 6)`` fp64 on the device, per sequence the unweighted terms of the poses ``x``
    [e2d, e3d, eacc, ebone, the sum of conf over the joints e2d includes, the joints skipped for a depth under ``z_min``]; ``ebone`` is 0
    without ``bone_len`` (S, E)."""
    f, j = _check_poses(x, tables, "fit_energy")
    _check_poses(x0, tables, "fit_energy")
    if tuple(x0.shape) != tuple(x.shape):
        raise ValueError(f"fit_energy: x {tuple(x.shape)} and x0 {tuple(x0.shape)} differ")
    _check_side(x, rays, conf, "fit_energy")
    ed, n_edges, lens = _edge_args(edges, j, bone_len, tables.sequences, x.device, "fit_energy")
    energy = torch.empty((tables.sequences, ENERGY_SLOTS), dtype=torch.float64, device=x.device)
    rc = _lib.load_library().r50_op_pose_fit_energy(x.data_ptr(), x0.data_ptr(), rays.data_ptr(), conf.data_ptr() if conf is not None else None,
                                                    tables.seq_start.data_ptr(), tables.row_seg.data_ptr(), f, tables.sequences, j, ed, n_edges,
                                                    lens, float(z_min), energy.data_ptr(), _stream(x))
    _lib.check(rc, None, "r50_op_pose_fit_energy")
    return energy


def fit_sweeps(x0: torch.Tensor, rays: torch.Tensor, conf: Optional[torch.Tensor], tables: DeviceTables, settings: RefineSettings,
               bone_len: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``settings.iters`` launches of ``r50_op_pose_fit_sweeps``' kernel: the refined poses (F, J, 3) fp32.  ``bone_len`` (S, E) fp64 is
    needed where ``settings.lambda_bone != 0``; ``workspace``: 2 F J 3 doubles on the device (allocated here if absent)."""
    f, j = _check_poses(x0, tables, "fit_sweeps")
    _check_side(x0, rays, conf, "fit_sweeps")
    if settings.lambda_bone != 0.0 and bone_len is None:
        raise ValueError("fit_sweeps: lambda_bone != 0 needs bone_len")
    ed, n_edges, lens = _edge_args(settings.edges, j, bone_len if settings.lambda_bone != 0.0 else None, tables.sequences, x0.device,
                                   "fit_sweeps")
    if workspace is None:
        workspace = torch.empty(2 * f * j * 3, dtype=torch.float64, device=x0.device)
    if workspace.dtype != torch.float64 or workspace.numel() < 2 * f * j * 3 or workspace.device != x0.device or not workspace.is_contiguous():
        raise ValueError(f"fit_sweeps: workspace must be a contiguous fp64 tensor of at least {2 * f * j * 3} elements on {x0.device}")
    out = torch.empty_like(x0)
    s = settings
    rc = _lib.load_library().r50_op_pose_fit_sweeps(x0.data_ptr(), rays.data_ptr(), conf.data_ptr() if conf is not None else None,
                                                    tables.seg_start.data_ptr(), tables.row_seg.data_ptr(), tables.row_seq.data_ptr(), f,
                                                    tables.segments, tables.sequences, j, ed, n_edges, lens, s.lambda_2d, s.lambda_3d,
                                                    s.lambda_acc, s.lambda_bone, s.omega, s.z_min, s.iters, workspace.data_ptr(),
                                                    out.data_ptr(), _stream(x0))
    _lib.check(rc, None, "r50_op_pose_fit_sweeps")
    return out


def refine_sequences(x0: torch.Tensor, rays: torch.Tensor, conf: Optional[torch.Tensor], tables, settings: RefineSettings,
                     bone_len: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Dict[str, object]]:
    """``x0`` (F, J, 3) fp32 on a GPU fitted to ``rays`` (F, J, 2) [weighted by ``conf`` (F, J)]; ``tables`` a ``SequenceTable``, a pair
    ``(seq_start, idx)`` or ``DeviceTables``.  Returns ``(refined, info)``; ``x0`` is not modified.  ``info``: ``tables``,
    ``energy_before`` and ``energy_after`` ((S, 6) fp64 on the device, from the energy op: nothing here waits for the GPU) and
    ``bone_len``.  With ``lambda_bone != 0`` and no ``bone_len`` the lengths are the mean column of ``smooth.bone_stats(x0)``."""
    tables = DeviceTables.of(tables, x0.device)
    _check_poses(x0, tables, "refine_sequences")
    if settings.lambda_bone != 0.0 and bone_len is None:
        bone_len = bone_stats(x0, tables, settings.edges)[:, :, 0].contiguous()
    lens = bone_len if settings.lambda_bone != 0.0 else None
    before = fit_energy(x0, x0, rays, conf, tables, settings.z_min, settings.edges, lens)
    refined = fit_sweeps(x0, rays, conf, tables, settings, lens)
    after = fit_energy(refined, x0, rays, conf, tables, settings.z_min, settings.edges, lens)
    return refined, {"tables": tables, "energy_before": before, "energy_after": after, "bone_len": lens}


# ---- command-line flags, shared by ``results`` and ``predict`` ---------------------------------------------------------------------------
FLAG_DEFAULTS = dict(refine_iters=50, refine_lambda_2d=1.0, refine_lambda_3d=1.0, refine_lambda_acc=1.0, refine_lambda_bone=0.0,
                     refine_omega=0.6, refine_z_min=0.1)


def add_parameter_flags(parser) -> None:
    """The fit's parameter flags; absent from the namespace unless given."""
    import argparse
    s = argparse.SUPPRESS
    parser.add_argument("--refine-iters", type=int, default=s, help="2D fit: sweeps, 0 .. 1000 (default 50)")
    parser.add_argument("--refine-lambda-2d", type=float, default=s, help="2D fit: weight of the reprojection residual (default 1)")
    parser.add_argument("--refine-lambda-3d", type=float, default=s, help="2D fit: weight of the distance to the prediction, > 0 (default 1)")
    parser.add_argument("--refine-lambda-acc", type=float, default=s, help="2D fit: weight of the second differences along time (default 1)")
    parser.add_argument("--refine-lambda-bone", type=float, default=s,
                        help="2D fit: weight of the bone lengths against their per-sequence mean (default 0)")
    parser.add_argument("--refine-omega", type=float, default=s, help="2D fit: step of a sweep, in (0, 0.75] (default 0.6)")
    parser.add_argument("--refine-z-min", type=float, default=s, help="2D fit: the smallest depth a joint is projected at, metres (default 0.1)")


def settings_from_args(args, enabled: bool, owner: str, error) -> Optional[RefineSettings]:
    """The ``RefineSettings`` of a parsed command line, or None when the fit is not asked for; ``error`` (the parser's) is called if a
    parameter flag is given without ``owner`` (the flag that turns the fit on), or a parameter is refused."""
    if not enabled:
        for k in FLAG_DEFAULTS:
            if hasattr(args, k):
                error(f"--{k.replace('_', '-')} needs {owner}")
        return None
    v = {k: getattr(args, k, d) for k, d in FLAG_DEFAULTS.items()}
    try:
        return RefineSettings(iters=v["refine_iters"], lambda_2d=v["refine_lambda_2d"], lambda_3d=v["refine_lambda_3d"],
                              lambda_acc=v["refine_lambda_acc"], lambda_bone=v["refine_lambda_bone"], omega=v["refine_omega"],
                              z_min=v["refine_z_min"])
    except ValueError as exc:
        error(str(exc))


# ---- the dense pass ------------------------------------------------------------------------------------------------------------------------
def _first_contributors(store, dense: Dict[str, object]):
    """Per stitched frame of ``dense`` the clip and window position it is first shown by, from the table rebuilt as ``evaluate_dense``
    builds it."""
    from .sequences import SequenceTable
    t = int(store.feats.shape[1])
    table = SequenceTable.from_clips(store.item_clips(), t)
    if table.frames != int(np.asarray(dense["pred"]).shape[0]) or not np.array_equal(table.seq_start, np.asarray(dense["seq_start"])) or \
            not np.array_equal(table.idx, np.asarray(dense["frame_idx"])):
        raise ValueError("the dense result was not computed from this store: the stitched frames differ")
    first = table.src[table.offsets[:-1]].astype(np.int64)
    return table, first // t, first % t


def _dense_rays_focal(store, dense: Dict[str, object], batch: int = 4096) -> Tuple[np.ndarray, np.ndarray]:
    table, item, pos = _first_contributors(store, dense)
    rays, focal = [], []
    for s in range(0, table.frames, batch):
        it = item[s:s + batch]
        got = store.get_batch(it.tolist())
        uv = got[2].detach().cpu().numpy()[np.arange(it.size), pos[s:s + batch]]                # (n, J, 2)
        k = got[3].detach().to(torch.float64).cpu().numpy()
        rays.append(rays_from_pixels(uv, k))
        focal.append(np.stack([k[:, 0, 0], k[:, 1, 1]], axis=-1))
    return np.concatenate(rays), np.concatenate(focal)


def dense_rays(store, dense: Dict[str, object]) -> np.ndarray:
    """(F, J, 2) fp32: per stitched frame of ``dense`` the rays of its first contributing clip in the ``SequenceTable`` order (the
    earliest clip start), from that clip's ``joints2d`` and ``K``.  Rays do not depend on the crop, so the clips of a frame agree."""
    return _dense_rays_focal(store, dense)[0]


@torch.no_grad()
def evaluate_refine(dense: Dict[str, object], store, device="cuda", settings: Optional[RefineSettings] = None, noise_px: float = 0.0,
                    seed: int = 0, keep: bool = False, chunk_rows: int = 1 << 20) -> Dict[str, object]:
    """``dense`` is the result of ``sequences.evaluate_dense(keep_poses=True)`` on ``store``; its ``pred`` is fitted to the store's 2D
    joints in runs of whole sequences of at most ``chunk_rows`` rows and the result scored against ``gt`` by the metrics and protocols
    launches of ``evaluate_dense``; the sums are read once.  The store's 2D joints are GROUND TRUTH, so without noise the gain is an
    upper bound; ``noise_px`` adds seeded Gaussian noise of that many pixels of the contributing clip's 224 crop (divided by that clip's
    focal length).  Returns (metres; fp64), for M in ``p1``, ``p2``, ``mpjve``, ``accel``::

        refine_M (G,), refine_M_all, refine_M_mean           beside M of ``dense``
        refine_residual_raw / refine_residual (G,), *_all    sqrt(e2d / sum conf) before and after the fit
        refine_skipped (2,) int64                             (t, j) behind z_min before and after
        refine_energy_before / refine_energy_after (S, 6), refine (the settings), refine_noise_px, refine_seed
        with keep: pred_refined (F, J, 3)
    """
    from . import protocols, sequences
    settings = settings or RefineSettings()
    missing = [k for k in ("seq_keys", "seq_start", "frame_idx", "pred", "gt", "group_names", "count") if k not in dense]
    if missing:
        raise ValueError(f"the dense result lacks {missing}: run evaluate_dense with keep_poses=True")
    noise_px = float(noise_px)
    if not (math.isfinite(noise_px) and noise_px >= 0.0):
        raise ValueError(f"noise_px must be finite and >= 0, got {noise_px}")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("evaluate_refine runs on a GPU: there is no CPU fallback")
    rays_host, focal = _dense_rays_focal(store, dense)
    if noise_px > 0.0:
        rng = np.random.default_rng(int(seed))
        rays_host = (rays_host.astype(np.float64) + noise_px * rng.standard_normal(rays_host.shape) / focal[:, None, :]).astype(np.float32)
    single = np.ascontiguousarray(dense["pred"], dtype=np.float32)
    f, joints = int(single.shape[0]), int(single.shape[1])
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
        rays = torch.from_numpy(np.ascontiguousarray(rays_host)).to(device)
        refined = torch.empty_like(pred)
        energies = []
        for a, b in runs:
            r0, r1 = int(seq_start[a]), int(seq_start[b])
            tables = ((seq_start[a:b + 1] - r0).astype(np.int32), frame_idx[r0:r1].astype(np.int32))
            refined[r0:r1], info = refine_sequences(pred[r0:r1], rays[r0:r1], None, tables, settings)
            energies.append(torch.stack([info["energy_before"], info["energy_after"]], dim=1).reshape(-1))
        seq = np.repeat(np.arange(n_seq, dtype=np.int32), np.diff(seq_start))
        group = torch.from_numpy(seq_group[seq]).to(device)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(np.asarray(dense["count"]), dtype=np.int64)]).astype(np.int32)).to(device)
        part = sequences.sequence_metrics(refined, gt, torch.zeros(f, dtype=torch.float32, device=device), offsets,
                                          torch.from_numpy(seq).to(device),
                                          torch.from_numpy(np.ascontiguousarray(frame_idx, dtype=np.int32)).to(device), group, n_groups)
        acc_p2 = torch.zeros(3 * n_groups, dtype=torch.float64, device=device)
        protocols._launch(refined.view(f, 1, joints, 3), gt.view(f, 1, joints, 3), 0, group, n_groups, acc_p2, protocols.ROOT_JOINT)
        host = torch.cat([acc_p2, part.reshape(-1)] + energies).cpu().numpy()
        kept = {"pred_refined": refined.cpu().numpy()} if keep else {}
    p2, part, energy = np.split(host, [3 * n_groups, host.size - n_seq * 2 * ENERGY_SLOTS])
    vals = sequences.metric_values(sequences.sum_blocks(part.reshape(-1, n_groups, sequences.METRIC_SLOTS)),
                                   p2[:2 * n_groups].reshape(n_groups, 2)[:, 1])
    out: Dict[str, object] = dict(kept)
    for m in ("p1", "p2", "mpjve", "accel"):
        for suffix in ("", "_all", "_mean"):
            out["refine_" + m + suffix] = vals[m + suffix]
    energy = energy.reshape(n_seq, 2, ENERGY_SLOTS)
    out["refine_energy_before"], out["refine_energy_after"] = energy[:, 0].copy(), energy[:, 1].copy()
    for k, name in enumerate(("refine_residual_raw", "refine_residual")):
        e2d = np.bincount(seq_group, weights=energy[:, k, 0], minlength=n_groups)
        cs = np.bincount(seq_group, weights=energy[:, k, 4], minlength=n_groups)
        out[name] = np.where(cs > 0, np.sqrt(e2d / np.where(cs > 0, cs, 1.0)), np.nan)
        out[name + "_all"] = float(np.sqrt(e2d.sum() / cs.sum())) if cs.sum() > 0 else float("nan")
    out["refine_skipped"] = energy[:, :, 5].sum(axis=0).round().astype(np.int64)
    out["refine"], out["refine_noise_px"], out["refine_seed"] = settings.describe(), noise_px, int(seed)
    return out


def _noise_note(res: Dict[str, object]) -> str:
    if res["refine_noise_px"] > 0.0:
        return f"ground-truth 2D + {res['refine_noise_px']:g} px noise (224 crop, seed {res['refine_seed']})"
    return "ground-truth 2D without noise: an upper bound"


def refine_lines(dense: Dict[str, object], res: Dict[str, object]) -> List[str]:
    """The ``Dense | refine`` lines: raw -> refined over all frames and per action (mm), the reprojection residual, the joints skipped
    behind z_min and which 2D observations were used."""
    def pair(m: str, key: str, i=None) -> str:
        a, b = dense[m + key], res["refine_" + m + key]
        a, b = (a, b) if i is None else (a[i], b[i])
        return f"{a * 1000.0:.2f} -> {b * 1000.0:.2f}"

    def row(key: str, i=None) -> str:
        a, b = res["refine_residual_raw" + key], res["refine_residual" + key]
        a, b = (a, b) if i is None else (a[i], b[i])
        return (f"p1 (mm) {pair('p1', key, i)} | p2 (mm) {pair('p2', key, i)} | vel (mm/frame) {pair('mpjve', key, i)} | accel (mm/frame^2) "
                f"{pair('accel', key, i)} | reprojection (mm) {a * 1000.0:.2f} -> {b * 1000.0:.2f}")

    skipped = res["refine_skipped"]
    lines = [f"Dense | refine {res['refine']} (section Z) | {_noise_note(res)} | joints skipped behind z_min {int(skipped[0])} -> "
             f"{int(skipped[1])} | raw -> refined, all: {row('_all')}"]
    for i, name in enumerate(dense["group_names"]):
        lines.append(f"Dense | refine   {name} | {row('', i)}")
    return lines


def refine_npz(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The ``dense_refine_*`` keys of the result ``.npz``: ``dense_refine_M`` (G,) and ``dense_refine_M_all`` () fp32 for M in p1, p2, mpjve,
    accel, residual_raw, residual; ``dense_refine_skipped`` (2,) int64; ``dense_refine_energy_before`` / ``_after`` (S, 6) fp64;
    ``dense_refine`` (the settings) and ``dense_refine_noise`` [px, seed] fp64."""
    out = {"dense_refine": np.array(str(res["refine"])), "dense_refine_skipped": np.asarray(res["refine_skipped"], dtype=np.int64),
           "dense_refine_noise": np.array([res["refine_noise_px"], res["refine_seed"]], dtype=np.float64),
           "dense_refine_energy_before": np.asarray(res["refine_energy_before"], dtype=np.float64),
           "dense_refine_energy_after": np.asarray(res["refine_energy_after"], dtype=np.float64)}
    for m in ("p1", "p2", "mpjve", "accel", "residual_raw", "residual"):
        out["dense_refine_" + m] = np.asarray(res["refine_" + m], dtype=np.float32)
        out["dense_refine_" + m + "_all"] = np.asarray(res["refine_" + m + "_all"], dtype=np.float32)
    return out


def refine_export(res: Dict[str, object]) -> Dict[str, np.ndarray]:
    """What ``--dense-out`` gains: ``pred_refined`` (F, J, 3) fp32 of an ``evaluate_refine(keep=True)`` result, and what made it."""
    return {"pred_refined": res["pred_refined"], "refine": np.array(str(res["refine"]))}


# ---- one video (``predict --refine-2d``) ---------------------------------------------------------------------------------------------------
def video_rays(joints2d, cam: dict, joints: int) -> np.ndarray:
    """(n, J, 2) fp32 rays of the kept frames' 2D joints in whole-frame pixels under the camera's ``f`` and ``c``."""
    uv = np.asarray(joints2d)
    if uv.ndim != 3 or uv.shape[1:] != (int(joints), 2):
        raise ValueError(f"joints2d must be (N, {joints}, 2), got {uv.shape}")
    return rays_from_pixels(uv, (cam["f"], cam["c"]))


def refine_video(joints3d: torch.Tensor, rays: np.ndarray, conf, settings: RefineSettings) -> Tuple[torch.Tensor, Dict[str, object]]:
    """The poses of one video (n, J, 3) on the device as one sequence of one segment through ``refine_sequences``."""
    n, j = int(joints3d.shape[0]), int(joints3d.shape[1])
    dev = joints3d.device
    conf_t = None
    if conf is not None:
        conf = np.ascontiguousarray(conf, dtype=np.float32)
        if conf.shape != (n, j) or not np.all(conf >= 0.0):
            raise ValueError(f"conf2d must be ({n}, {j}) values >= 0, got {conf.shape}")
        conf_t = torch.from_numpy(conf).to(dev)
    if tuple(rays.shape) != (n, j, 2):
        raise ValueError(f"the rays cover {tuple(rays.shape)}, the poses ({n}, {j}, 3)")
    return refine_sequences(joints3d.contiguous(), torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).to(dev), conf_t,
                            (np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32)), settings)
