"""Test-subject results of a trained lifting head on one MI355X: ``python -m implementation_phd_lab_vision_amd.results``, the
counterpart of ``python src/results.py`` (src/results.py:137-239).

It scores a checkpoint on the test subject (S9) with ``train.evaluate`` over the reference's shuffled test loader
(``shuffle=True, drop_last=True``, :162-170), prints the reference's metrics line, and dumps ONE batch to an ``.npz`` for the
visualisation scripts: the clips' video, ground-truth and predicted 3D joints, 2D joints, intrinsics, meta and the test metrics.
With ``--pred-len P`` (default 0: off) it also forecasts: ``forecast.evaluate_rollout`` over the test set
prints MPJPE per horizon, and the ``.npz`` gains ``predicted_future3djoints`` (the dumped clips' P future poses after
``--input-len`` observed frames), ``future_mpjpe`` (P,) and ``rollout_lens`` [I, P].  With ``--protocols`` (default off) it also scores
the H3.6M protocols per action: ``protocols.evaluate_protocols`` over every test clip once, in store order
(not the loader's ``drop_last`` batches), prints root-relative MPJPE (P1) and PA-MPJPE (P2) for all clips, the action mean and each
action (and per horizon with ``--pred-len``), and the ``.npz`` gains the ``protocol_*`` keys.  With ``--detail-metrics`` (default off)
it also reports, over the same pass structure, P1 / P2 per joint, PCK at ``--pck-threshold-mm`` and AUC over
``--auc-steps`` thresholds (both root-relative and after the similarity fit), and the velocity and acceleration errors in mm per frame
and mm per frame^2, for all clips, the action mean and each action (and per horizon with ``--pred-len``); the ``.npz`` gains the
``detail_*`` keys.  With ``--render DIR`` (default off) the first ``--render-n`` dumped clips are also
drawn on the device (``render.render_panels``: frame + GT 2D joints | frame + projected GT and prediction | 3D view) and written as
``DIR/clip_<i>_S<subject>_<action>.png`` (an APNG at ``--render-fps``) and ``DIR/clip_<i>_sheet.png`` (every ``--render-sheet-every``-th
frame); the frames are the clip's person crop -- ``meta["box"]`` through ``frames.crop_and_resize_video_uint8``, what ``joints2d`` and
``K`` refer to -- and the ``.npz`` gains ``video_crop`` (n, T, 224, 224, 3).  With ``--dense`` (default off)
the overlapping clips are stitched into one pose per video frame (``sequences.evaluate_dense``, ``--dense-fuse mean | context | last``)
and every video frame is scored once: the ``Dense |`` lines print P1, P2, the velocity and acceleration errors and the spread of the
contributors for all frames, the action mean and each action, and the clip-wise P1 / P2 by window position; the ``.npz`` gains the
``dense_*`` keys and ``--dense-out FILE.npz`` receives the stitched sequences themselves.  With ``--dtw`` (default off; needs
``--pred-len``) the forecasts are also scored after dynamic time warping (``dtw.evaluate_dtw``,
``--dtw-band N``): the ``DTW metrics`` lines print the warped P1 / P2 beside the unwarped ones for all clips and each action, and the
warped error and the lag in frames per horizon; the ``.npz`` gains the ``dtw_*`` keys.  With ``--baselines`` (default off; needs
``--pred-len``) trivial forecasts are scored on the same clips (``baselines.evaluate_baselines``): the last
pose held, the last step continued, and the future of the nearest training clip in movie-strip space (``--nn-subjects``, ``--nn-k``);
the ``Baselines`` lines print each predictor's MPJPE / P1 / P2 per horizon beside the model's and the model's skill against it; the
``.npz`` gains the ``baseline_*`` and ``nn_*`` keys.  With ``--hallucinate`` (default off; needs a checkpoint of ``train_hal``;
INTEGRATION.md section V) the head is also scored from single frames (``hallucinate.evaluate_hallucinator``): the ``Hallucinator`` lines
print the reconstruction of every frame from that frame alone beside the one with temporal context and, with ``--pred-len``, the
forecast from the last observed frame alone beside the rollout's, per horizon and per action; the ``.npz`` gains the ``hal_*`` keys.
With ``--dense-smooth gauss | savgol | one_euro`` and / or ``--dense-fix-bones`` (default off; need ``--dense``; INTEGRATION.md section
W) the stitched sequences are also filtered along time and rebuilt with constant bone lengths on the device (``smooth.PostProcess``):
the ``Dense | post`` lines set the processed poses' errors and bone-length deviation beside the raw ones, the ``.npz`` gains the
``dense_post_*`` keys and ``--dense-out`` gains ``pred_post``.  With ``--multiview`` (default off; needs ``--dense``)
the cameras of every take are brought into one frame of reference and fused into one pose per frame (``multiview.evaluate_multiview``,
``--multiview-fit gt | pred``, ``--multiview-fuse mean | median | others``): ``Dense | multiview`` lines, ``dense_mv_*`` keys, and
``--dense-out`` gains ``pred_mv``, ``frame_disagreement``, ``views`` and ``mv_pair_*``.  With ``--dense-rigid`` (default off; needs
``--dense``) every stitched sequence is also fitted with joint rotations on a rigid skeleton
(``kinematics.evaluate_rigid``): ``Dense | rigid`` lines set the rigid reconstruction's errors beside the poses', the ``.npz`` gains the
``dense_rigid_*`` keys, and ``--dense-bvh DIR`` writes one BVH file per sequence.  With ``--dense-holdout K`` (default off; needs
``--dense``; INTEGRATION.md section AB) only every K-th row of a stitched sequence is kept and the rows in between are interpolated
(``resample.evaluate_holdout``): ``Dense | holdout`` lines, ``dense_holdout_*`` keys, ``pred_holdout`` in ``--dense-out``.  With
``--bootstrap R`` (default off; INTEGRATION.md section AC) the P1 / P2 numbers get percentile intervals and standard errors from R
replicates of a stratified cluster bootstrap (``bootstrap.evaluate_bootstrap``: whole sequences, takes or clips resampled inside each
action), and with ``--compare MODEL_PATH`` a paired comparison of the two checkpoints: ``Bootstrap | ...`` lines, ``bootstrap_*`` keys.
Every report's printed lines and ``.npz`` keys
(``*_lines``, ``*_arrays`` / ``*_npz``) are defined in the module that computes it; ``main`` only calls them in order.

Two differences from running the reference's script as it stands:

* the head's dimensions come from the checkpoint (``infer_head_dims``): the reference builds ``PHD(joints_num=17)`` with its
  default dims (latent 2048, 3 blocks, :175), so its strict ``load_state_dict`` fails on the ``PHD(1024, 17, 2)`` checkpoints
  its own src/train.py writes (:370).  Here both load.
* frame selection.  Shard metas carry no ``frame_skip``, so the reference's ``frames[::meta.get("frame_skip", 1)][start:end]``
  (:101-105) slices the full-rate video with clip indices that count every ``frame_skip``-th frame: the video it dumps covers
  another, shorter span than the clip's joints.  That stays the default, kept on purpose and documented (INTEGRATION.md,
  section H); ``--aligned-video`` takes the clip's own frames, ``[::index.pt frame_skip][start:end]``.

Video decode stays on the host (``--video-reader``, torchvision's ``read_video`` by default, as the reference).  The frames a
clip names are uploaded once and ``_pad_or_trim_video`` + ``_resize_video_hw`` (:65-93) are one ``r50_op_resize_frames_u8``
launch per clip into the batch buffer.  No CPU fallback.
"""
from __future__ import annotations

import argparse
import glob
import importlib
import os
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

SEQ_LEN = 40                              # src/config.py
INPUT_LEN = 15                            # src/config.py: the rollout's observed frames (--input-len)
TEST_SUBJECTS = [9]                       # hard-coded at src/results.py:159
BASELINE_NAMES = ("const_pose", "const_vel", "nn")   # baselines.BASELINES (--baselines)


def build_parser() -> argparse.ArgumentParser:
    """The reference's flags and defaults (src/results.py:138-150), then this project's extras."""
    p = argparse.ArgumentParser("Test Subject 9 + dump ONE BATCH to NPZ")
    p.add_argument("--features_root", type=str, required=True)
    p.add_argument("--preprocessed_root", type=str, required=True)
    p.add_argument("--seq-len", type=int, default=SEQ_LEN)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--num-workers", type=int, default=4, help="accepted, no effect: the feature store is resident in HBM")
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--weights-from", choices=WEIGHT_SOURCES, default="auto",
                   help="which weights of --model_path to evaluate: auto = the EMA weights when the checkpoint has them, else the raw ones")
    p.add_argument("--out", type=str, default="outputs/batch_result_S9.npz")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--save-n", type=int, default=16, help="How many samples from the batch to save")
    p.add_argument("--video-size", type=int, default=224,
                   help="Resize saved videos to video_size x video_size before stacking (use 0 to disable).")
    p.add_argument("--seed", type=int, default=0, help="torch.manual_seed before the test loader draws its two orders")
    p.add_argument("--precision", choices=("fp16", "bf16"), default="fp16", help="16-bit type of the head's GEMMs")
    p.add_argument("--test-subjects", type=int, nargs="+", default=list(TEST_SUBJECTS))
    p.add_argument("--aligned-video", action="store_true",
                   help="dump the clip's own frames, [::index.pt frame_skip][start:end] (default: the reference's "
                        "[::meta.get('frame_skip', 1)][start:end])")
    p.add_argument("--video-reader", type=str, default=None,
                   help="module:function, a callable path -> (N,H,W,3) uint8 (default: torchvision.io.read_video(path, pts_unit='sec')[0])")
    p.add_argument("--input-len", type=int, default=INPUT_LEN, help="observed frames of the rollout (src/config.py INPUT_LEN)")
    p.add_argument("--pred-len", type=int, default=0,
                   help="frames to forecast with f_AR and score per horizon (INTEGRATION.md section J); 0 = off")
    p.add_argument("--protocols", action="store_true",
                   help="also score root-relative MPJPE (P1) and PA-MPJPE (P2) per action over every test clip, and per horizon "
                        "with --pred-len (INTEGRATION.md section L)")
    p.add_argument("--geo-metrics", action="store_true",
                   help="also report the test-subject 2D reprojection loss and pixel error, velocity and bone-length losses and the number of "
                        "predicted joints at or behind the camera plane, over the same batches (INTEGRATION.md section N)")
    p.add_argument("--detail-metrics", action="store_true",
                   help="also report P1 / P2 per joint, PCK / AUC and the velocity / acceleration errors per action over every test clip, "
                        "and per horizon with --pred-len (INTEGRATION.md section O)")
    p.add_argument("--pck-threshold-mm", type=float, default=150.0, help="PCK threshold and the end of the AUC range, in mm (--detail-metrics)")
    p.add_argument("--auc-steps", type=int, default=31, help="thresholds of the AUC, 0 .. --pck-threshold-mm evenly (--detail-metrics)")
    p.add_argument("--render", type=str, default=None, metavar="DIR",
                   help="also draw the first --render-n dumped clips on the device (pose overlays + 3D view) and write an APNG and a "
                        "contact sheet per clip under DIR (INTEGRATION.md section P); default off")
    p.add_argument("--render-n", type=int, default=4, help="clips to render (--render)")
    p.add_argument("--render-fps", type=float, default=10.0, help="frame rate of the APNGs (--render)")
    p.add_argument("--render-sheet-every", type=int, default=5, help="the contact sheet holds every this-many-th frame (--render)")
    p.add_argument("--dense", action="store_true",
                   help="also stitch the overlapping clips into one pose per video frame and score every video frame once, per action "
                        "(INTEGRATION.md section Q)")
    p.add_argument("--dense-fuse", choices=("mean", "context", "last"), default="context",
                   help="how a frame's predictions are fused (--dense): the plain mean, weights growing with the past a window position "
                        "has seen up to f_movie's receptive field, or the prediction that has seen the most past")
    p.add_argument("--dense-out", type=str, default=None, metavar="FILE.npz",
                   help="also write the stitched sequences (seq_keys, seq_start, frame_idx, pred, gt, spread, count) there (--dense)")
    p.add_argument("--dtw", action="store_true",
                   help="also score the forecast after dynamic time warping: warped P1 / P2 beside the unwarped ones per action, and the "
                        "warped error and the lag in frames per horizon (needs --pred-len; INTEGRATION.md section T)")
    p.add_argument("--dtw-band", type=int, default=-1, metavar="N",
                   help="only warp within |i - j| <= N frames (--dtw); negative = no band (default)")
    p.add_argument("--baselines", nargs="*", choices=BASELINE_NAMES, default=argparse.SUPPRESS, metavar="NAME",
                   help="also score trivial forecasts on the same clips (needs --pred-len; INTEGRATION.md section U): const_pose, const_vel "
                        "and nn (the future of the nearest training clip in movie-strip space); a bare flag means all three")
    p.add_argument("--baseline-anchor", choices=("pred", "gt"), default=argparse.SUPPRESS,
                   help="the pose the baselines start from (--baselines): the head's own reconstruction of the last observed frames "
                        "(pred, default) or the ground truth (gt)")
    p.add_argument("--nn-k", type=int, default=argparse.SUPPRESS, metavar="K", help="neighbours averaged by the nn baseline, 1..8 (default 1)")
    p.add_argument("--nn-subjects", type=int, nargs="+", default=argparse.SUPPRESS,
                   help="subjects whose clips the nn baseline searches (default: train.TRAIN_SUBJECTS); must not overlap --test-subjects")
    p.add_argument("--nn-features-root", type=str, default=argparse.SUPPRESS, metavar="DIR",
                   help="feature cache of the nn baseline's database (default: --features_root)")
    p.add_argument("--nn-max-clips", type=int, default=argparse.SUPPRESS, metavar="N", help="use only the first N database clips (nn baseline)")
    p.add_argument("--hallucinate", action="store_true", default=argparse.SUPPRESS,
                   help="also score the hallucinator f_hal on the same clips (INTEGRATION.md section V): every frame's pose from that frame "
                        "alone beside the one with temporal context and, with --pred-len, the forecast from the last observed frame "
                        "alone beside the rollout's; needs a checkpoint written by train_hal")
    p.add_argument("--dense-smooth", choices=("gauss", "savgol", "one_euro"), default=argparse.SUPPRESS,
                   help="also filter every stitched sequence along time on the device and score the result beside the raw poses "
                        "(--dense; INTEGRATION.md section W): a Gaussian, a Savitzky-Golay filter, or the causal One-Euro filter")
    p.add_argument("--dense-fix-bones", action="store_true", default=argparse.SUPPRESS,
                   help="also give every bone its sequence's mean length, after the filter (--dense; INTEGRATION.md section W)")
    from .smooth import add_parameter_flags
    add_parameter_flags(p)
    from .multiview import add_flags as add_multiview_flags
    add_multiview_flags(p)
    p.add_argument("--dense-rigid", action="store_true", default=argparse.SUPPRESS,
                   help="also fit joint rotations on a rigid skeleton to every stitched sequence and score the rigid reconstruction "
                        "beside the poses it was fitted to (--dense; INTEGRATION.md section Y)")
    p.add_argument("--dense-bvh", type=str, default=argparse.SUPPRESS, metavar="DIR",
                   help="write one BVH file per sequence into DIR (--dense-rigid)")
    from .kinematics import add_bvh_flags
    add_bvh_flags(p)
    p.add_argument("--dense-refine", action="store_true", default=argparse.SUPPRESS,
                   help="also fit every stitched sequence to the cache's 2D joints under a temporal prior and score the result beside the "
                        "raw poses (--dense; INTEGRATION.md section Z); the cache's 2D joints are ground truth: an upper bound")
    p.add_argument("--dense-refine-noise-px", type=float, default=argparse.SUPPRESS, metavar="PX",
                   help="add seeded Gaussian noise of PX pixels of the 224 crop to the 2D joints (--dense-refine; default 0)")
    p.add_argument("--dense-refine-seed", type=int, default=argparse.SUPPRESS, metavar="N", help="seed of that noise (default 0)")
    from .refine import add_parameter_flags as add_refine_flags
    add_refine_flags(p)
    p.add_argument("--dense-holdout", type=int, default=argparse.SUPPRESS, metavar="K",
                   help="also keep only every K-th row of every stitched sequence (K >= 2) and every segment's last row, rebuild the rows in "
                        "between by interpolation and score them beside the full-rate poses (--dense; INTEGRATION.md section AB): what a "
                        "backbone that sees every K-th frame would cost")
    p.add_argument("--dense-holdout-kind", choices=("cubic", "linear"), default=argparse.SUPPRESS,
                   help="how --dense-holdout interpolates (default cubic)")
    p.add_argument("--bootstrap", type=int, default=argparse.SUPPRESS, metavar="R",
                   help="also give P1 / P2 (per action, and per horizon with --pred-len) a percentile interval and a standard error from R "
                        "replicates of a stratified cluster bootstrap: whole units resampled with replacement inside each action "
                        "(INTEGRATION.md section AC)")
    p.add_argument("--bootstrap-unit", choices=("sequence", "take", "clip"), default=argparse.SUPPRESS,
                   help="what --bootstrap resamples: a sequence (subject, action with trial, camera; default), a take (all cameras of one "
                        "motion) or single clips (overlapping clips are dependent: this understates the uncertainty)")
    p.add_argument("--bootstrap-seed", type=int, default=argparse.SUPPRESS, metavar="N", help="seed of the replicates, 0 .. 2^64 - 1 (default 0)")
    p.add_argument("--bootstrap-level", type=float, default=argparse.SUPPRESS, metavar="L", help="coverage of the intervals (default 0.95)")
    p.add_argument("--compare", type=str, default=argparse.SUPPRESS, metavar="MODEL_PATH",
                   help="a second checkpoint (--bootstrap): both models are scored on the same resampled units, and the lines give "
                        "A, B, B - A with its interval and the share of replicates in which B is better")
    p.add_argument("--compare-weights-from", choices=WEIGHT_SOURCES, default=argparse.SUPPRESS,
                   help="which weights of --compare to evaluate (default auto, as --weights-from)")
    return p


def dense_post(args: argparse.Namespace, error=None):
    """The ``smooth.PostProcess`` of parsed arguments, or None without ``--dense-smooth`` / ``--dense-fix-bones``."""
    from .smooth import post_from_args

    def raise_(msg):
        raise ValueError(msg)
    return post_from_args(args, getattr(args, "dense_smooth", None), getattr(args, "dense_fix_bones", False), error or raise_)


def dense_refine(args: argparse.Namespace, error=None):
    """The ``refine.RefineSettings`` of parsed arguments, or None without ``--dense-refine``."""
    from .refine import settings_from_args

    def raise_(msg):
        raise ValueError(msg)
    return settings_from_args(args, hasattr(args, "dense_refine"), "--dense-refine", error or raise_)


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    """``build_parser().parse_args`` plus the rollout flags' checks: --pred-len >= 0 and, when it is on, 1 <= --input-len and
    --input-len + --pred-len <= --seq-len."""
    p = build_parser()
    args = p.parse_args(argv)
    if args.pred_len < 0:
        p.error(f"--pred-len must be >= 0 (0 = no rollout), got {args.pred_len}")
    if args.pred_len > 0:
        if args.input_len < 1:
            p.error(f"--input-len must be >= 1, got {args.input_len}")
        if args.input_len + args.pred_len > args.seq_len:
            p.error(f"--input-len + --pred-len = {args.input_len + args.pred_len} exceeds --seq-len {args.seq_len}")
    if args.detail_metrics:
        if not 2 <= args.auc_steps <= 1024:
            p.error(f"--auc-steps must lie in [2, 1024], got {args.auc_steps}")
        if not (np.isfinite(args.pck_threshold_mm) and args.pck_threshold_mm > 0):
            p.error(f"--pck-threshold-mm must be finite and > 0, got {args.pck_threshold_mm}")
    if args.render is not None:
        if args.render_n < 1:
            p.error(f"--render-n must be >= 1, got {args.render_n}")
        if not args.render_fps > 0:
            p.error(f"--render-fps must be > 0, got {args.render_fps}")
        if args.render_sheet_every < 1:
            p.error(f"--render-sheet-every must be >= 1, got {args.render_sheet_every}")
    if args.dense_out is not None and not args.dense:
        p.error("--dense-out needs --dense")
    for flag in ("dense_smooth", "dense_fix_bones"):
        if hasattr(args, flag) and not args.dense:
            p.error(f"--{flag.replace('_', '-')} needs --dense")
    dense_post(args, p.error)                # a parameter flag without its filter, or a refused parameter
    from .multiview import OPTION_FLAGS as MULTIVIEW_FLAGS
    if hasattr(args, "multiview") and not args.dense:
        p.error("--multiview needs --dense")
    for flag in MULTIVIEW_FLAGS:
        if hasattr(args, flag) and not hasattr(args, "multiview"):
            p.error(f"--{flag.replace('_', '-')} needs --multiview")
    if not getattr(args, "multiview_gt_tol_mm", 1.0) > 0:
        p.error(f"--multiview-gt-tol-mm must be > 0, got {args.multiview_gt_tol_mm}")
    if hasattr(args, "dense_rigid") and not args.dense:
        p.error("--dense-rigid needs --dense")
    if hasattr(args, "dense_bvh") and not hasattr(args, "dense_rigid"):
        p.error("--dense-bvh needs --dense-rigid")
    for flag in ("bvh_fps", "bvh_scale"):
        if hasattr(args, flag) and not hasattr(args, "dense_bvh"):
            p.error(f"--{flag.replace('_', '-')} needs --dense-bvh")
    from .kinematics import bvh_options
    bvh_options(args, p.error)
    if hasattr(args, "dense_refine") and not args.dense:
        p.error("--dense-refine needs --dense")
    for flag in ("dense_refine_noise_px", "dense_refine_seed"):
        if hasattr(args, flag) and not hasattr(args, "dense_refine"):
            p.error(f"--{flag.replace('_', '-')} needs --dense-refine")
    if not (np.isfinite(getattr(args, "dense_refine_noise_px", 0.0)) and getattr(args, "dense_refine_noise_px", 0.0) >= 0.0):
        p.error(f"--dense-refine-noise-px must be finite and >= 0, got {args.dense_refine_noise_px}")
    dense_refine(args, p.error)              # a parameter flag without --dense-refine, or a refused parameter
    if hasattr(args, "dense_holdout") and not args.dense:
        p.error("--dense-holdout needs --dense")
    if hasattr(args, "dense_holdout_kind") and not hasattr(args, "dense_holdout"):
        p.error("--dense-holdout-kind needs --dense-holdout")
    if getattr(args, "dense_holdout", 2) < 2:
        p.error(f"--dense-holdout keeps every K-th row with K >= 2, got {args.dense_holdout}")
    for flag in ("bootstrap_unit", "bootstrap_seed", "bootstrap_level", "compare"):
        if hasattr(args, flag) and not hasattr(args, "bootstrap"):
            p.error(f"--{flag.replace('_', '-')} needs --bootstrap")
    if hasattr(args, "compare_weights_from") and not hasattr(args, "compare"):
        p.error("--compare-weights-from needs --compare")
    if getattr(args, "bootstrap", 1) < 1:
        p.error(f"--bootstrap takes the number of replicates R >= 1, got {args.bootstrap}")
    if not 0 <= getattr(args, "bootstrap_seed", 0) < 1 << 64:
        p.error(f"--bootstrap-seed must lie in [0, 2^64), got {args.bootstrap_seed}")
    if not 0.0 < getattr(args, "bootstrap_level", 0.95) < 1.0:
        p.error(f"--bootstrap-level must lie in (0, 1), got {args.bootstrap_level}")
    if args.dtw and args.pred_len <= 0:
        p.error("--dtw needs --pred-len > 0: it scores the forecast")
    if args.dtw and args.pred_len > 64:
        p.error(f"--dtw warps at most 64 predicted frames, got --pred-len {args.pred_len}")
    if hasattr(args, "baselines"):
        if args.pred_len <= 0:
            p.error("--baselines needs --pred-len > 0: it scores forecasts")
        which = baseline_options(args)[0]
        if "const_vel" in which and args.input_len < 2:
            p.error("--baselines const_vel needs --input-len >= 2: it continues the last observed step")
        if not 1 <= getattr(args, "nn_k", 1) <= 8:
            p.error(f"--nn-k must lie in [1, 8], got {args.nn_k}")
        if getattr(args, "nn_max_clips", 1) < 1:
            p.error(f"--nn-max-clips must be >= 1, got {args.nn_max_clips}")
        if "nn" in which:
            from .train import TRAIN_SUBJECTS
            both = sorted(set(getattr(args, "nn_subjects", TRAIN_SUBJECTS)) & set(args.test_subjects))
            if both:
                p.error(f"--nn-subjects overlaps --test-subjects in {both}: a query would retrieve itself")
    else:
        for flag in ("baseline_anchor", "nn_k", "nn_subjects", "nn_features_root", "nn_max_clips"):
            if hasattr(args, flag):
                p.error(f"--{flag.replace('_', '-')} needs --baselines")
    return args


def baseline_options(args: argparse.Namespace) -> Tuple[Tuple[str, ...], str, int]:
    """(which, anchor, nn_k) of parsed arguments that carry ``--baselines``: a bare flag means all three, in BASELINE_NAMES order and
    without repeats."""
    given = set(args.baselines) if args.baselines else set(BASELINE_NAMES)
    return tuple(n for n in BASELINE_NAMES if n in given), getattr(args, "baseline_anchor", "pred"), int(getattr(args, "nn_k", 1))


# ---- host pieces ------------------------------------------------------------------------------------------------------------
def find_video_path(preprocessed_root: str, meta: dict) -> str:
    """``_find_video_path`` (src/results.py:31-42): the first of the sorted ``*.mp4`` under ``S{subject}/{action}/cam_{cam}``."""
    cam = str(meta["cam"])
    if not cam.startswith("cam_"):
        cam = f"cam_{cam}"
    cam_dir = os.path.join(preprocessed_root, f"S{int(meta['subject'])}", str(meta["action"]), cam)
    mp4s = sorted(glob.glob(os.path.join(cam_dir, "*.mp4")))
    if not mp4s:
        raise FileNotFoundError(f"No mp4 found under {cam_dir}")
    return mp4s[0]


def frame_index_map(n_frames: int, start: int, end: int, frame_skip: int, seq_len: int) -> List[int]:
    """Indices into the decoded video of the ``seq_len`` frames the reference dumps: ``frames[::frame_skip][start:end]``
    (src/results.py:103-105), then ``_pad_or_trim_video`` (:65-79: trim, or repeat the last frame).  RuntimeError when the
    selection is empty, as the reference raises (:107-110)."""
    sel = list(range(n_frames))[::frame_skip][start:end]
    if not sel:
        raise RuntimeError(f"Loaded 0 frames with start={start}, end={end}, frame_skip={frame_skip} from a video of {n_frames} frames")
    return sel[:seq_len] + [sel[-1]] * max(seq_len - len(sel), 0)


def infer_head_dims(state: Dict[str, torch.Tensor]) -> Tuple[int, int, int]:
    """(latent_dim, joints_num, number_blocks) of a reference-layout state dict: ``input_proj.weight`` is (latent_dim, 2048),
    ``f_3D.y0`` holds joints_num * 3 values, ``f_movie.blocks.<i>.*`` counts the blocks."""
    latent_dim = int(state["input_proj.weight"].shape[0])
    joints_num = int(state["f_3D.y0"].numel()) // 3
    blocks = {int(k.split(".")[2]) for k in state if k.startswith("f_movie.blocks.")}
    return latent_dim, joints_num, (max(blocks) + 1 if blocks else 0)


WEIGHT_SOURCES = ("auto", "model", "ema")


def load_head_state(path: str, which: str = "auto") -> Dict[str, torch.Tensor]:
    """The state dict of a checkpoint: ``ckpt["model"]`` of a training checkpoint (``train.save_checkpoint``, src/train.py:61-76),
    or the file itself when it is a plain state dict (src/results.py:181-182).  ``weights_only=True``.
    ``which``: a run with ``--ema-decay`` also saves its averaged weights, ``ckpt["ema"]["model"]``.
    "auto" returns them when the file has them (they are what selected ``best.pt``) and the raw weights otherwise; "model" the raw
    weights whatever else is there; "ema" the averaged ones, ``ValueError`` when the file has none."""
    if which not in WEIGHT_SOURCES:
        raise ValueError(f"which: expected one of {WEIGHT_SOURCES}, got {which!r}")
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    has_ema = isinstance(ckpt, dict) and isinstance(ckpt.get("ema"), dict) and "model" in ckpt["ema"]
    if which == "ema" and not has_ema:
        raise ValueError(f"{path}: no EMA weights in this file (it was not written by a run with --ema-decay)")
    if has_ema and which != "model":
        return ckpt["ema"]["model"]
    return ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt else ckpt


def build_head(state: Dict[str, torch.Tensor], device, precision: str = "fp16"):
    """A ``model.PHDFor3DJoints`` with the checkpoint's own dimensions, loaded strictly, on ``device``, in eval mode.  A state with
    the hallucinator's keys (``f_hal.*``) gives a head with f_hal."""
    from .model import PHDFor3DJoints, has_hallucinator
    latent_dim, joints_num, number_blocks = infer_head_dims(state)
    head = PHDFor3DJoints(latent_dim, joints_num, number_blocks, precision=precision, hallucinator=has_hallucinator(state))
    head.load_state_dict(state, strict=True)
    return head.to(device).eval()


def loader_batch_order(n: int, batch_size: int, seed: int) -> Tuple[List[List[int]], List[int]]:
    """The reference's test loader over ``n`` items (``DataLoader(test_set, batch_size, shuffle=True, drop_last=True)``,
    src/results.py:162-170), drawn by torch's own DataLoader after ``torch.manual_seed(seed)``: the batches of one full pass
    (the evaluation, :190) and the first batch of a second iterator (the dump, :197).  Each iterator draws a base seed and then
    its sampler's seed from the global generator, as the reference's loader does; worker processes do not change that."""
    from torch.utils.data import DataLoader
    torch.manual_seed(seed)
    loader = DataLoader(range(n), batch_size=batch_size, shuffle=True, drop_last=True)
    eval_batches = [b.tolist() for b in loader]
    return eval_batches, next(iter(loader)).tolist()


def resolve_video_reader(spec: Optional[str]) -> Callable:
    """``--video-reader``: ``module:function``, or None for ``torchvision.io.read_video(path, pts_unit="sec")[0]`` (:101).
    Raises SystemExit with a message when it cannot be imported."""
    if spec is None:
        try:
            tv_io = importlib.import_module("torchvision.io")
        except ImportError as e:
            raise SystemExit(f"results: the default video reader needs torchvision ({e}); install it or pass "
                             "--video-reader module:function") from None
        return lambda path: tv_io.read_video(path, pts_unit="sec")[0]
    mod, sep, fn = spec.partition(":")
    if not sep or not mod or not fn:
        raise SystemExit(f"results: --video-reader must be module:function, got {spec!r}")
    try:
        reader = getattr(importlib.import_module(mod), fn)
    except (ImportError, AttributeError) as e:
        raise SystemExit(f"results: cannot load --video-reader {spec!r}: {e}") from None
    if not callable(reader):
        raise SystemExit(f"results: --video-reader {spec!r} is not callable")
    return reader


CROP_SIZE = 224                           # the person crop the shards' joints2d and K refer to (src/dataset.py:107-140)


def crop_clip(frames_sel: torch.Tensor, box, b: int) -> Optional[torch.Tensor]:
    """(T, 224, 224, 3) uint8 on the device: the clip's person crop, ``frames_sel`` (T,H,W,3) on the device through
    ``frames.crop_and_resize_video_uint8`` with ``meta["box"]`` = [top, left, hh, ww].  None, with one printed notice, when the clip
    has no usable box: ``None`` (features written with ``--augment``: each variant drew its own crop) or one that does not lie inside
    the decoded frame."""
    from .frames import crop_and_resize_video_uint8
    if box is None:
        print(f"render: clip {b} has no crop box (features written with --augment): plain background")
        return None
    top, left, hh, ww = (int(v) for v in (box.tolist() if isinstance(box, torch.Tensor) else box))
    h, w = int(frames_sel.shape[1]), int(frames_sel.shape[2])
    if top < 0 or left < 0 or hh < 1 or ww < 1 or top + hh > h or left + ww > w:
        print(f"render: clip {b}: the crop box {[top, left, hh, ww]} does not lie inside its {h}x{w} frames: plain background")
        return None
    return crop_and_resize_video_uint8(frames_sel, [top, left, hh, ww], CROP_SIZE).permute(0, 2, 3, 1).contiguous()


def dump_videos(metas: Sequence[dict], preprocessed_root: str, reader: Callable, seq_len: int, video_size: int,
                frame_skip_of: Callable[[dict], int], device, crops: Optional[list] = None, crop_n: int = 0) -> np.ndarray:
    """(B, seq_len, H, W, 3) uint8: per clip, decode on the host, select (``frame_index_map``), then one
    ``r50_op_resize_frames_u8`` launch into the batch buffer; ``video_size == 0`` keeps the decoded size (host pad / trim only).
    ``crops`` (a list, with ``crop_n`` > 0): receives, for each of the first ``crop_n`` clips, ``crop_clip`` of the same decoded and
    selected frames (``--render``: the video is decoded once)."""
    from .frames import resize_frames_uint8
    host_clips, buf = [], None
    if video_size > 0:
        buf = torch.empty((len(metas), seq_len, video_size, video_size, 3), dtype=torch.uint8, device=device)
    for b, meta in enumerate(metas):
        if not isinstance(meta, dict):
            raise RuntimeError(f"Expected meta[{b}] to be dict, got {type(meta)}")
        path = find_video_path(preprocessed_root, meta)
        frames = torch.as_tensor(reader(path))
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise RuntimeError(f"video reader returned {tuple(frames.shape)} {frames.dtype} for {path}; expected (N,H,W,3) uint8")
        sel = frame_index_map(frames.shape[0], int(meta["start"]), int(meta["end"]), frame_skip_of(meta), seq_len)
        want_crop = crops is not None and b < crop_n
        if buf is None and not want_crop:
            host_clips.append(frames[sel].numpy())
            continue
        used = sorted(set(sel))                                   # upload only the frames the map names, once each
        pos = {f: i for i, f in enumerate(used)}
        clip = frames[used].contiguous().to(device)
        if want_crop:
            crops.append(crop_clip(clip[[pos[f] for f in sel]], meta.get("box"), b))
        if buf is None:
            host_clips.append(frames[sel].numpy())
            continue
        resize_frames_uint8(clip, [pos[f] for f in sel], video_size, out=buf[b])
    if buf is not None:
        return buf.cpu().numpy()
    if len({c.shape for c in host_clips}) > 1:
        raise RuntimeError(f"--video-size 0 keeps each video's own frame size, and this batch mixes "
                           f"{sorted({c.shape[1:3] for c in host_clips})}: pass --video-size > 0")
    return np.stack(host_clips, axis=0)


def main(argv: Optional[List[str]] = None) -> str:
    """``python src/results.py`` on one MI355X.  Returns the path of the written ``.npz``."""
    from .feature_store import DeviceFeatureStore
    from .protocols import action_groups
    from .train import evaluate

    args = parse_args(argv)
    reader = resolve_video_reader(args.video_reader)             # before the evaluation pass: fail early
    device = torch.device(args.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.R50Error("the results pass runs on an MI355X only; there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t0 = time.time()
    test_set = DeviceFeatureStore(args.features_root, subjects=args.test_subjects, test_set=True, device=device)
    if len(test_set) < args.batch_size:
        raise SystemExit(f"results: the test set has {len(test_set)} clips, fewer than one batch of {args.batch_size} "
                         "(the loader drops the last incomplete batch); lower --batch-size")
    index_skip = int(torch.load(os.path.join(args.features_root, "index.pt"), map_location="cpu", weights_only=True).get("frame_skip", 1))
    state = load_head_state(args.model_path, args.weights_from)
    if hasattr(args, "hallucinate"):
        from .hallucinate import require_hallucinator
        require_hallucinator(state)
    head = build_head(state, device, args.precision)
    print(f"Head: latent_dim={head.latent_dim} joints={head.joints_num} blocks={head.number_blocks} ({args.precision}) | "
          f"test clips: {len(test_set)}")

    eval_batches, dump_idx = loader_batch_order(len(test_set), args.batch_size, args.seed)
    avg_loss, avg_mpjpe, avg_l3d, avg_l2d = evaluate(head, test_set, args.batch_size, test_set=True, batches=eval_batches)
    print(f"Test metrics | loss: {avg_loss:.6f} | mpjpe (m): {avg_mpjpe:.6f} "
          f"| mpjpe (mm): {avg_mpjpe * 1000.0:.2f} | l3d: {avg_l3d:.6f} | l2d: {avg_l2d:.6f}")
    rollout = None
    if args.pred_len > 0:
        from .forecast import evaluate_rollout
        rollout = evaluate_rollout(head, test_set, args.input_len, args.pred_len)
        mm = rollout["mpjpe"]
        at = " | ".join(f"@{k}: {mm[k - 1] * 1000.0:.2f}" for k in sorted({h for h in (1, 5, 10, args.pred_len) if h <= args.pred_len}))
        print(f"Rollout metrics | input {args.input_len} | pred {args.pred_len} | clips {rollout['clips']} | mpjpe (mm) {at} "
              f"| mean: {rollout['mpjpe_mean'] * 1000.0:.2f}")
    if args.protocols or args.detail_metrics or args.dtw or hasattr(args, "baselines") or hasattr(args, "hallucinate"):
        names, ids = action_groups(test_set.item_actions())      # the per-action reports' groups, shared by all of them
    protocols = None
    if args.protocols:                       # every test clip once, in store order (not the loader's drop_last batches)
        from .protocols import evaluate_protocols, protocol_arrays, protocol_lines
        protocols = evaluate_protocols(head, test_set, ids, names, args.input_len if args.pred_len > 0 else 0, args.pred_len)
        for line in protocol_lines(protocols, args.input_len, args.pred_len):
            print(line)

    geo = None
    if args.geo_metrics:                     # the loader's batches again, the terms by r50_op_geo_pose_loss_grad with dy = NULL
        from .train import GEO_EXTRA_KEYS, GeoWeights, evaluate_geo
        geo = evaluate_geo(head, test_set, args.batch_size, GeoWeights(), batches=eval_batches)
        print("Geo metrics | " + " | ".join(f"{key}: {geo[key]:.6f}" for key in GEO_EXTRA_KEYS))

    detail = None
    if args.detail_metrics:                  # the protocols' pass: every test clip once, in store order
        from .detail_metrics import detail_lines, detail_npz, evaluate_detail
        detail = evaluate_detail(head, test_set, ids, names, args.input_len if args.pred_len > 0 else 0, args.pred_len,
                                 n_thr=args.auc_steps, thr_max=args.pck_threshold_mm / 1000.0)
        for line in detail_lines(detail, args.input_len, args.pred_len):
            print(line)

    dense, multi, rigid, fitted, holdout = None, None, None, None, None
    if args.dense:                           # every video frame once: the clips of a sequence fused per frame
        from .sequences import dense_export, dense_lines, dense_npz, dense_post_lines, evaluate_dense
        from . import multiview as mv
        post, mv_options = dense_post(args), mv.options_from_args(args)
        want_rigid = hasattr(args, "dense_rigid")
        fit = dense_refine(args)
        if want_rigid:
            from . import kinematics
            kinematics.skeleton_for(int(head.joints_num))        # refused before the pass if there is no skeleton for the head's joints
        dense = evaluate_dense(head, test_set, fuse=args.dense_fuse,
                               keep_poses=args.dense_out is not None or mv_options is not None or want_rigid or fit is not None
                               or hasattr(args, "dense_holdout"),
                               **({} if post is None else {"post": post}))
        for line in dense_lines(dense) + (dense_post_lines(dense) if post is not None else []):
            print(line)
        if mv_options is not None:           # the cameras of every take fused, scored beside the single views (section X)
            multi = mv.evaluate_multiview(dense, device, **mv_options)
            for line in mv.multiview_lines(dense, multi):
                print(line)
        if want_rigid:                       # joint rotations on a rigid skeleton, the reconstruction scored beside the poses (section Y)
            rigid = kinematics.evaluate_rigid(dense, None, device, keep=hasattr(args, "dense_bvh"))
            for line in kinematics.rigid_lines(dense, rigid):
                print(line)
            if hasattr(args, "dense_bvh"):
                files = kinematics.write_dense_bvh(args.dense_bvh, dense, rigid, None, *kinematics.bvh_options(args, None))
                print(f"Dense | rigid   {len(files)} BVH files written to: {args.dense_bvh}")
        if fit is not None:                  # the stitched poses fitted to the cache's 2D joints, scored beside the raw ones (section Z)
            from . import refine
            fitted = refine.evaluate_refine(dense, test_set, device, fit, getattr(args, "dense_refine_noise_px", 0.0),
                                            getattr(args, "dense_refine_seed", 0), keep=args.dense_out is not None)
            for line in refine.refine_lines(dense, fitted):
                print(line)
        if hasattr(args, "dense_holdout"):   # every K-th row kept, the rows in between interpolated and scored (section AB)
            from . import resample
            holdout = resample.evaluate_holdout(dense, args.dense_holdout, getattr(args, "dense_holdout_kind", "cubic"), device,
                                                keep=args.dense_out is not None)
            for line in resample.holdout_lines(dense, holdout):
                print(line)

    dtw = None
    if args.dtw:                             # the protocols' pass over the forecasts: every test clip once, in store order
        from .dtw import dtw_arrays, dtw_lines, evaluate_dtw
        dtw = evaluate_dtw(head, test_set, ids, names, args.input_len, args.pred_len, band=args.dtw_band)
        for line in dtw_lines(dtw, args.input_len, args.pred_len):
            print(line)

    base, base_db = None, None
    if hasattr(args, "baselines"):           # the protocols' pass again: the trivial forecasts beside the model's, every test clip once
        from .baselines import StripDatabase, baseline_arrays, baseline_lines, evaluate_baselines
        which, anchor, nn_k = baseline_options(args)
        if "nn" in which:
            from .train import TRAIN_SUBJECTS
            nn_subjects = list(getattr(args, "nn_subjects", TRAIN_SUBJECTS))
            both = sorted(set(nn_subjects) & set(args.test_subjects))
            if both:
                raise SystemExit(f"results: the nn baseline's subjects overlap --test-subjects in {both}: a query would retrieve itself")
            train_set = DeviceFeatureStore(getattr(args, "nn_features_root", args.features_root), subjects=nn_subjects,
                                           max_clips=getattr(args, "nn_max_clips", None), device=device)
            if int(train_set.feats.shape[1]) < args.input_len + args.pred_len:
                raise SystemExit(f"results: the nn baseline's clips have {int(train_set.feats.shape[1])} frames, fewer than --input-len + "
                                 f"--pred-len = {args.input_len + args.pred_len}")
            if len(train_set) < nn_k:
                raise SystemExit(f"results: the nn baseline's database has {len(train_set)} clips, fewer than --nn-k {nn_k}")
            base_db = StripDatabase.build(head, train_set, args.input_len)
            print(f"Baselines | nn database: {len(base_db)} clips of subjects {nn_subjects}")
        base = evaluate_baselines(head, test_set, base_db, ids, names, args.input_len, args.pred_len, which, nn_k=nn_k, anchor=anchor)
        for line in baseline_lines(base, args.input_len, args.pred_len):
            print(line)

    hal = None
    if hasattr(args, "hallucinate"):         # the protocols' pass once more: from single frames beside with temporal context
        from .hallucinate import evaluate_hallucinator, hallucinate_lines
        hal = evaluate_hallucinator(head, test_set, ids, names, args.input_len if args.pred_len > 0 else 0, args.pred_len)
        for line in hallucinate_lines(hal):
            print(line)

    boot = None
    if hasattr(args, "bootstrap"):           # intervals on P1 / P2 from whole resampled units; two checkpoints on the same units (section AC)
        from . import bootstrap as bs
        other = None
        if hasattr(args, "compare"):
            other = build_head(load_head_state(args.compare, getattr(args, "compare_weights_from", "auto")), device, args.precision)
            if int(other.joints_num) != int(head.joints_num):
                raise SystemExit(f"results: --compare has {int(other.joints_num)} joints, --model_path {int(head.joints_num)}")
        boot = bs.evaluate_bootstrap(head, test_set, None, args.bootstrap, getattr(args, "bootstrap_unit", "sequence"),
                                     getattr(args, "bootstrap_seed", 0), getattr(args, "bootstrap_level", 0.95),
                                     args.input_len if args.pred_len > 0 else 0, args.pred_len, compare=other)
        for line in bs.bootstrap_lines(boot):
            print(line)

    feats, joints3d, joints2d, k, metas = test_set.get_batch(dump_idx)
    n_save = min(feats.shape[0], args.save_n)
    pred = head.joints(feats)[:n_save].cpu().numpy()
    if args.aligned_video:
        frame_skip_of = lambda meta: index_skip                   # noqa: E731
    else:
        frame_skip_of = lambda meta: int(meta.get("frame_skip", 1))   # noqa: E731  (the reference's behaviour, kept on purpose)
    n_render = min(n_save, args.render_n) if args.render is not None else 0
    crops: List[Optional[torch.Tensor]] = []
    videos = dump_videos(metas[:n_save], args.preprocessed_root, reader, args.seq_len, args.video_size, frame_skip_of, device,
                         crops=crops if n_render else None, crop_n=n_render)
    joints3d_np = joints3d[:n_save].cpu().numpy()

    out_path = args.out
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    extra = {}
    if rollout is not None:                  # the dumped clips' forecast: observe input_len frames, predict pred_len
        extra = {"predicted_future3djoints": head.rollout(feats[:n_save], args.input_len, args.pred_len)[1].cpu().numpy(),
                 "future_mpjpe": np.array(rollout["mpjpe"], dtype=np.float32),
                 "rollout_lens": np.array([args.input_len, args.pred_len], dtype=np.int64)}
    if protocols is not None:
        extra.update(protocol_arrays(protocols))
    if geo is not None:
        extra["geo_metrics"] = np.array([geo[key] for key in GEO_EXTRA_KEYS], dtype=np.float64)
        extra["geo_metric_names"] = np.array(GEO_EXTRA_KEYS)
    if detail is not None:
        extra.update(detail_npz(detail))
    if dense is not None:
        extra.update(dense_npz(dense))
        if multi is not None:
            extra.update(mv.multiview_npz(multi))
        if rigid is not None:
            extra.update(kinematics.rigid_npz(rigid))
        if fitted is not None:
            extra.update(refine.refine_npz(fitted))
        if holdout is not None:
            extra.update(resample.holdout_npz(holdout))
        if args.dense_out is not None:
            os.makedirs(os.path.dirname(args.dense_out) or ".", exist_ok=True)
            np.savez_compressed(args.dense_out, **dense_export(dense), **({} if multi is None else mv.multiview_export(multi)),
                                **({} if fitted is None else refine.refine_export(fitted)),
                                **({} if holdout is None else resample.holdout_export(holdout)))
            print(f"Dense | stitched sequences saved to: {args.dense_out}")
    if dtw is not None:
        extra.update(dtw_arrays(dtw))
    if base is not None:
        extra.update(baseline_arrays(base))
        if base_db is not None:              # the dumped clips' retrieval: which training clips, how far, and the future they give
            from .baselines import forecast_batch
            fb = forecast_batch(head, base_db, feats[:n_save], joints3d[:n_save].to(torch.float32).contiguous(), args.input_len,
                                args.pred_len, ("nn",), baseline_options(args)[2], baseline_options(args)[1])
            extra.update(nn_index=fb["nn_index"].cpu().numpy(), nn_dist2=fb["nn_dist2"].cpu().numpy(),
                         nn_future3djoints=fb["nn"].cpu().numpy())
    if hal is not None:
        from .hallucinate import hallucinate_arrays
        extra.update(hallucinate_arrays(hal))
    if boot is not None:
        extra.update(bs.bootstrap_npz(boot))
    if n_render:                             # the person crops, drawn over; a clip without a usable box gets the plain background
        from . import render
        plain = torch.tensor(render._rgb_tuple(render.PANEL_BG_RGB), dtype=torch.uint8, device=device)
        video_crop = torch.stack([c if c is not None else plain.expand(args.seq_len, CROP_SIZE, CROP_SIZE, 3) for c in crops])
        future = torch.from_numpy(extra["predicted_future3djoints"][:n_render]).to(device) if rollout is not None else None
        written = render.render_clips(args.render, video_crop, joints2d[:n_render], k[:n_render].to(torch.float32), joints3d[:n_render],
                                      torch.from_numpy(pred[:n_render]).to(device), future, args.input_len if rollout is not None else 0,
                                      list(metas[:n_render]), args.render_fps, args.render_sheet_every)
        extra["video_crop"] = video_crop.cpu().numpy()
        print(f"Rendered {n_render} clips ({len(written)} files) to: {args.render}")
    np.savez_compressed(out_path, video=videos, joints3d=joints3d_np, predicted3djoints=pred,
                        joints2d=joints2d[:n_save].cpu().numpy(), K=k[:n_save].to(torch.float32).cpu().numpy(),
                        meta=np.array(list(metas[:n_save]), dtype=object),
                        test_metrics=np.array([avg_loss, avg_mpjpe, avg_l3d, avg_l2d], dtype=np.float32), **extra)
    print(f"[OK] Saved batch to: {out_path}")
    print(f"video shape: {videos.shape} | joints3d: {joints3d_np.shape} | pred: {pred.shape}")
    print(f"Results time: {time.time() - t0:.2f}s")
    return out_path


if __name__ == "__main__":
    main()
