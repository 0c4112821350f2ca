"""Host-side mirror of the reference's phase-1 training step for the lifting head on one MI355X.

The reference (src/train.py:114-176,370-393)::

    model = PHD(latent_dim=1024, joints_num=17, number_blocks=2); f_AR frozen (:375-376)
    optim = torch.optim.AdamW(trainable, lr=args.lr, weight_decay=1e-2); scaler = torch.amp.GradScaler('cuda')
    with torch.autocast(dtype=torch.float16):
        _phi, _phi_hat, joints_pred, _ = model.forward(feats, predict_future=False)
        loss = l3d = (joints_pred - joints3d).pow(2).mean()
    scaler.scale(loss).backward(); scaler.step(optim); scaler.update()

``TrainableHead`` keeps the model surface of ``model.PHDFor3DJoints`` (constructor, ``load_state_dict`` / ``state_dict`` with the
reference's keys) and adds ``train_step(feats, joints3d, optim, scaler)``; its flat buffers, the backward's launch helpers and the tail
of a step are ``trainable.FlatTrainableHead``'s, shared with phase 2 (train_ar.py) and the joint stage (train_joint.py), as the epoch
loop below (``open_run`` / ``fit``) is.  Arithmetic on the device, through the C ABI:

* forward as in model.py plus the two ``nn.Dropout(0.5)`` sites (src/model.py:44,52 and :98), applied with byte masks;
* backward: every dX = dY W and dW = dY^T X is an igemm MFMA launch (``r50_op_conv2d(_f16)``) on operands made K-contiguous by
  ``r50_op_transpose16``; GroupNorm + ReLU + causal-row backward, ReLU / dropout backward, bias column sums, the MSE gradient are
  the kernels of include/r50.h "Lifting head, backward + optimizer".  16-bit activations and gradients, fp32 accumulation in the
  GEMMs, fp32 master weights and fp32 flat gradient buffer (the shared regressor weights accumulate their three uses in fp32);
* ``AdamW`` / ``GradScaler``: one flat fp32 parameter / moment / gradient buffer, one ``r50_op_adamw`` launch per step, skipped on
  the device when ``r50_op_check_finite`` raised the flag; the scale follows torch.amp.GradScaler's rule (x0.5 on overflow, x2
  after 2000 clean steps).
* optional (``AdamW.max_grad_norm`` / ``AdamW.ema``, ``--clip-grad-norm`` / ``--ema-decay``): clipping by
  the global gradient norm, ``r50_op_grad_norm`` in the finite check's place, and EMA weights kept by ``r50_op_adamw_clip_ema`` in the
  optimizer's launch; with both off the step's launches are the ones above.
* f_AR is frozen and its output does not enter the loss (:158-161), so the training step does not run it.
* multi-GPU: one process per GPU, ``all_reduce_gradients`` averages the flat gradient buffer with ONE RCCL all-reduce per step
  (35.8 M parameters x 4 B = 67.6 MB at train.py's configuration; 16.9 M trainable) instead of nn.DataParallel's scatter /
  replicate / gather (:381-383).

The driver (src/train.py:219-465; ``python -m implementation_phd_lab_vision_amd.train``): ``evaluate`` (the validation pass, metrics
by ``r50_op_pose_metrics``), ``samplers.MixedShardBatchSampler`` over ``DeviceFeatureStore``, ``CosineLR`` (torch's
CosineAnnealingLR in the reference's order), ``save_checkpoint`` / ``load_checkpoint`` in the reference's format
(``AdamW.state_dict`` in torch.optim.AdamW's layout), early stopping and the reference's CLI.

The geometric losses the reference defines and leaves switched off (2D reprojection through ``K``, velocity, bone length;
INTEGRATION.md section N) are optional arguments of the step and of the evaluation: ``GeoWeights``, ``H36M_EDGES``,
``forward_backward / train_step / evaluate / train_epoch(..., geo=...)``, one HIP op (``r50_op_geo_pose_loss_grad``) for the loss and
its gradient.  ``main`` never passes them; ``python -m implementation_phd_lab_vision_amd.train_geo`` does, through ``run``.

PyTorch is used for device memory, the stream, the dropout masks' random bits, the LR schedule and torch.distributed.  No CPU fallback.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import math
import os
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .model import _REG_HIDDEN, _REG_ITERS, PHDFor3DJoints, expected_keys
from .trainable import (DROPOUT_P, FlatItem, FlatTrainableHead, WeightEMA, _Arena, all_reduce_gradients, block_items,  # noqa: F401
                        input_proj_items, regressor_items, sync_overflow_flag)

# ---- geometric losses ---------------------------------------------------------------------------------
# The 16-edge tree of the 17-joint H3.6M layout (src/train.py:29-35): hip -> right leg, left leg, spine -> head, left arm, right arm.
H36M_EDGES: Tuple[Tuple[int, int], ...] = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10),
                                           (8, 11), (11, 12), (12, 13), (8, 14), (14, 15), (15, 16))
GEO_EPS = 1e-6         # project_with_K_torch's clamp (src/train.py:84)
GEO_KEYS = ("loss", "l3d", "mpjpe", "l2d", "reproj_px", "l_vel", "l_bone", "n_clamped")       # r50_op_geo_pose_loss_grad's out8
GEO_EXTRA_KEYS = GEO_KEYS[3:]                                                                 # what the geometric terms add


@dataclass(frozen=True)
class GeoWeights:
    """Weights of the 2D reprojection, velocity and bone-length terms added to l3d (section N).  The defaults are the reference's:
    ``--lambda-2d`` 1e-6 (src/train.py:291), ``lambda_vel`` / ``lambda_bone`` 1 (the signature of its ``train()``, :114)."""
    lambda_2d: float = 1e-6
    lambda_vel: float = 1.0
    lambda_bone: float = 1.0

    def __post_init__(self):
        for name in ("lambda_2d", "lambda_vel", "lambda_bone"):
            v = float(getattr(self, name))
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
            object.__setattr__(self, name, v)

    def as_tuple(self) -> Tuple[float, float, float]:
        return (self.lambda_2d, self.lambda_vel, self.lambda_bone)


def expand_intrinsics(K: torch.Tensor, b: int) -> torch.Tensor:
    """K as the op reads it: (B,3,3) fp32 contiguous, one matrix per clip as the shards store it.  A (3,3) is expanded; a per-frame
    (B,T,3,3) is refused (out of scope, section N)."""
    if K.dim() == 4:
        raise ValueError("K: per-frame intrinsics (B,T,3,3) are not supported; pass one (3,3) per clip, (B,3,3)")
    if K.dim() == 2 and tuple(K.shape) == (3, 3):
        K = K.unsqueeze(0).expand(b, 3, 3)
    if tuple(K.shape) != (b, 3, 3):
        raise ValueError(f"K: expected (3,3) or (B,3,3) with B = {b}, got {tuple(K.shape)}")
    return K.to(torch.float32).contiguous()


def _edge_array(edges: Sequence[Tuple[int, int]]):
    flat = [int(v) for e in edges for v in e]
    return (ctypes.c_int * max(len(flat), 1))(*flat)


def geo_pose_loss_grad(y: torch.Tensor, gt3d: torch.Tensor, gt2d: torch.Tensor, K: torch.Tensor, b: int, t: int, joints: int,
                       geo: GeoWeights, out8: torch.Tensor, dy: Optional[torch.Tensor] = None, s0: int = 0, term_scale: float = 1.0,
                       loss_scale: float = 1.0, stream: Optional[int] = None, edges: Sequence[Tuple[int, int]] = H36M_EDGES) -> None:
    """One ``r50_op_geo_pose_loss_grad`` call on the current device: ``y`` (B*T, J*3) fp32 (or any contiguous view of that size),
    ``gt3d`` (B,T,J,3), ``gt2d`` (B,T,J,2), ``K`` (B,3,3), all fp32 contiguous; ``out8`` 8 fp32 (``GEO_KEYS``); ``dy`` like ``y`` or
    None (losses only).  The scratch for the per-clip partial sums is allocated here, outside the op."""
    for name, ten, n in (("y", y, b * t * joints * 3), ("gt3d", gt3d, b * t * joints * 3), ("gt2d", gt2d, b * t * joints * 2),
                         ("K", K, b * 9), ("out8", out8, 8)) + ((("dy", dy, b * t * joints * 3),) if dy is not None else ()):
        if ten.dtype != torch.float32 or not ten.is_contiguous() or ten.numel() != n or not ten.is_cuda:
            raise ValueError(f"{name}: expected {n} contiguous fp32 elements on the device")
    part = torch.empty(8 * b, dtype=torch.float64, device=y.device)
    if stream is None:
        stream = torch.cuda.current_stream(y.device).cuda_stream
    lam = geo.as_tuple()
    _lib.check(_lib.load_library().r50_op_geo_pose_loss_grad(y.data_ptr(), gt3d.data_ptr(), gt2d.data_ptr(), K.data_ptr(), b, t, s0, joints,
                                                              _edge_array(edges), len(edges), lam[0], lam[1], lam[2], GEO_EPS, term_scale,
                                                              loss_scale, dy.data_ptr() if dy is not None else None, part.data_ptr(),
                                                              out8.data_ptr(), stream), None, "r50_op_geo_pose_loss_grad")


class GradScaler:
    """torch.amp.GradScaler('cuda') defaults (src/train.py:392): init 65536, x2 after 2000 clean steps, x0.5 on inf/nan."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000, enabled: bool = True):
        self.enabled = enabled
        self._scale = float(init_scale) if enabled else 1.0
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval
        self._growth_tracker = 0

    def get_scale(self) -> float:
        return self._scale

    def update(self, found_inf: bool) -> None:
        if not self.enabled:
            return
        if found_inf:
            self._scale *= self.backoff_factor
            self._growth_tracker = 0
        else:
            self._growth_tracker += 1
            if self._growth_tracker == self.growth_interval:
                self._scale *= self.growth_factor
                self._growth_tracker = 0


class AdamW:
    """torch.optim.AdamW(trainable, lr, weight_decay=1e-2) (src/train.py:389) over the head's flat fp32 buffers."""

    def __init__(self, head: "TrainableHead", lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2):
        self.head, self.lr, self.betas, self.eps, self.weight_decay = head, lr, betas, eps, weight_decay
        self.initial_lr = lr                 # what CosineAnnealingLR records in the param group (saved in checkpoints)
        self.step_count = 0
        self.exp_avg = torch.zeros_like(head.flat_master)
        self.exp_avg_sq = torch.zeros_like(head.flat_master)
        self.max_grad_norm: Optional[float] = None      # section S: clip the global gradient norm to this (``_finish_step`` reads it)
        self.ema: Optional[WeightEMA] = None            # section S: averaged weights, updated inside the optimizer's launch

    def step(self, found_inf_flag: Optional[torch.Tensor]) -> None:
        """One update from ``head.flat_grad`` (already unscaled).  The step counter advances only when the update is applied.
        With ``max_grad_norm`` and / or ``ema`` set the launch is ``r50_op_adamw_clip_ema``: the gradient is read times the coefficient
        ``r50_op_grad_norm`` left in the head's clip buffer (``flat_grad`` itself is NOT changed: ``named_gradients()`` stays the
        unclipped gradient), and the EMA buffer moves by ``ema.weight()`` towards the new parameters."""
        h = self.head
        self.step_count += 1
        if self.max_grad_norm is not None or self.ema is not None:
            ema = self.ema
            rc = _lib.load_library().r50_op_adamw_clip_ema(
                h.flat_master.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), h.flat_grad.data_ptr(), h.flat_w16.data_ptr(),
                h.flat_master.numel(), self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.step_count,
                found_inf_flag.data_ptr() if found_inf_flag is not None else None,
                h._clip2.data_ptr() if self.max_grad_norm is not None else None, ema.flat.data_ptr() if ema is not None else None,
                ema.weight() if ema is not None else 0.0, h._et, h._stream())
            _lib.check(rc, None, "r50_op_adamw_clip_ema")
            if ema is not None:
                ema.updates += 1
            return
        rc = _lib.load_library().r50_op_adamw(h.flat_master.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                              h.flat_grad.data_ptr(), h.flat_w16.data_ptr(), h.flat_master.numel(), self.lr,
                                              self.betas[0], self.betas[1], self.eps, self.weight_decay, self.step_count,
                                              found_inf_flag.data_ptr() if found_inf_flag is not None else None, h._et, h._stream())
        _lib.check(rc, None, "r50_op_adamw")

    def _param_group(self, n: int) -> dict:
        """torch.optim.AdamW's param group for these hyperparameters, with the flags of the installed torch (taken from a
        throwaway instance rather than restated), ``initial_lr`` as CosineAnnealingLR sets it, parameter ids 0..n-1."""
        probe = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=self.lr, betas=self.betas, eps=self.eps,
                                  weight_decay=self.weight_decay)
        group = probe.state_dict()["param_groups"][0]
        group["initial_lr"] = self.initial_lr
        group["params"] = list(range(n))
        return group

    def state_dict(self) -> dict:
        """What ``torch.optim.AdamW(trainable, lr, weight_decay=1e-2).state_dict()`` of the reference holds (src/train.py:70,389):
        parameter ``i`` is ``trainable_names()[i]`` in the reference's layout, ``state[i] = {step: fp32 scalar tensor, exp_avg,
        exp_avg_sq}`` (CPU, fp32; empty before the first applied step, as torch's lazy state)."""
        names = self.head.trainable_parameter_names()
        state = {}
        if self.step_count > 0:
            m, v = self.head.flat_to_reference(self.exp_avg), self.head.flat_to_reference(self.exp_avg_sq)
            state = {i: {"step": torch.tensor(float(self.step_count), dtype=torch.float32), "exp_avg": m[n], "exp_avg_sq": v[n]}
                     for i, n in enumerate(names)}
        return {"state": state, "param_groups": [self._param_group(len(names))]}

    def load_state_dict(self, state_dict: dict) -> None:
        """Inverse of ``state_dict``; accepts what torch.optim.AdamW over the reference's trainable parameters saved.  Takes the
        group's hyperparameters (lr, initial_lr, betas, eps, weight_decay) as torch does, the moments and the step, then refreshes
        the head's 16-bit weights and their transposes from its fp32 master."""
        names = self.head.trainable_parameter_names()
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(names):
            raise ValueError(f"expected one param group of {len(names)} parameters (the head's trainable set)")
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("amsgrad / maximize AdamW states are not supported")
        ids = g["params"]
        state = state_dict["state"]
        if not state:
            step, m, v = 0, torch.zeros_like(self.exp_avg), torch.zeros_like(self.exp_avg_sq)
        else:
            steps = {float(state[i]["step"]) for i in ids}
            if len(steps) != 1:
                raise ValueError(f"the trainable parameters step together; found steps {sorted(steps)}")
            step = int(steps.pop())
            m = self.head.flat_from_reference({n: state[i]["exp_avg"] for n, i in zip(names, ids)})
            v = self.head.flat_from_reference({n: state[i]["exp_avg_sq"] for n, i in zip(names, ids)})
        self.lr, self.eps, self.weight_decay = float(g["lr"]), float(g["eps"]), float(g["weight_decay"])
        self.betas = (float(g["betas"][0]), float(g["betas"][1]))
        self.initial_lr = float(g.get("initial_lr", self.lr))
        self.exp_avg, self.exp_avg_sq, self.step_count = m, v, step
        self.head.refresh_weights16()


def trainable_names(number_blocks: int) -> List[str]:
    """``[n for n, p in model.named_parameters() if p.requires_grad]`` of the reference's ``PHDFor3DJoints`` with f_AR frozen
    (src/train.py:375-388): the module registers f_movie, f_AR, f_3D and then input_proj (src/model.py:142-146), a ResidualBlock
    gn1, conv1, gn2, conv2 (:39-44).  ``f_3D.y0`` is a buffer.  This is the numbering of the optimizer's state."""
    names: List[str] = []
    for i in range(number_blocks):
        for m in ("gn1", "conv1.conv", "gn2", "conv2.conv"):
            names += [f"f_movie.blocks.{i}.{m}.weight", f"f_movie.blocks.{i}.{m}.bias"]
    for j in (0, 3, 5):
        names += [f"f_3D.mlp.{j}.weight", f"f_3D.mlp.{j}.bias"]
    return names + ["input_proj.weight", "input_proj.bias"]


def phase1_items(number_blocks: int) -> List[FlatItem]:
    """Phase 1's flat buffer, in order: input_proj, f_movie's blocks (each gn1, gn2, conv1, conv2), the regressor."""
    items = input_proj_items()
    for i in range(number_blocks):
        items += block_items(f"f_movie.blocks.{i}", ("gn1", "gn2", "conv1", "conv2"))
    return items + regressor_items()


class TrainableHead(FlatTrainableHead):
    """``PHDFor3DJoints`` with the phase-1 trainable parameters (input_proj, f_movie, f_3D) in flat fp32 / 16-bit buffers.
    ``last_losses``: ``GEO_KEYS`` of the last train_step that was given ``geo``."""

    _no_transpose = frozenset({"input_proj.w"})

    def __init__(self, latent_dim: int = 2048, joints_num: int = 17, number_blocks: int = 3, precision: str = "fp16",
                 hallucinator: bool = False):
        super().__init__(latent_dim, joints_num, number_blocks, precision, hallucinator)
        self._use_graphs = False
        self._graphs: Dict[tuple, tuple] = {}
        self._geo_out8: Optional[torch.Tensor] = None

    def enable_graphs(self, on: bool = True) -> "TrainableHead":
        """Replay forward + loss + backward (~250 short launches) as one captured HIP graph per (B, T, loss scale, mode): the step
        is launch-bound otherwise.  The optimizer part stays outside (its bias corrections are per-step host scalars)."""
        self._use_graphs = bool(on)
        return self

    def _flat_items(self) -> List[FlatItem]:
        return phase1_items(self.number_blocks)

    def trainable_parameter_names(self) -> List[str]:
        """The names of the optimizer's parameters, in its numbering: ``trainable_names(number_blocks)``."""
        return trainable_names(self.number_blocks)

    def _dropout_sites(self) -> List[Tuple[str, int]]:
        """One per f_movie block (src/model.py:52) and one per regressor iteration (:98)."""
        return [(f"f_movie.blocks.{i}", self.latent_dim) for i in range(self.number_blocks)] + \
            [(f"f_3D.{i}", _REG_HIDDEN) for i in range(_REG_ITERS)]

    # ---- one training step ------------------------------------------------------------------------
    def _check_geo(self, b: int, t: int, joints2d: Optional[torch.Tensor], K: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The 2D targets and intrinsics of a step with geometric terms, as the op reads them."""
        if joints2d is None or K is None:
            raise ValueError("geo: the geometric terms need joints2d (B,T,J,2) and K (B,3,3)")
        if self.joints_num != 17:
            raise ValueError("geo: the bone term is defined on the 17-joint H3.6M skeleton (H36M_EDGES)")
        if tuple(joints2d.shape) != (b, t, self.joints_num, 2) or joints2d.device != self._device or K.device != self._device:
            raise ValueError("joints2d: expected (B,T,J,2), K (B,3,3), on the head's device")
        return joints2d.to(torch.float32).contiguous(), expand_intrinsics(K, b)

    def forward_backward(self, feats: torch.Tensor, joints3d: torch.Tensor, loss_scale: float = 1.0,
                         masks: Optional[Dict[str, torch.Tensor]] = None, joints2d: Optional[torch.Tensor] = None,
                         K: Optional[torch.Tensor] = None, geo: Optional[GeoWeights] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Forward (train mode when ``masks`` is given or ``self.training``; else dropout is identity), l3d loss (src/train.py:161),
        backward into ``flat_grad`` (UNSCALED: the 16-bit backward runs on loss_scale * loss, the fp32 buffer receives grad / loss_scale).
        ``self._found`` is raised when a 16-bit gradient overflowed (fp16 saturates at 65504 here instead of producing inf).
        Returns (joints_pred (B,T,J,3) fp32, loss2 = [l3d, mpjpe] fp32 device tensor).
        ``geo``: the loss is l3d + lambda_2d l2d + lambda_vel l_vel + lambda_bone l_bone (section N) on ``joints2d`` (B,T,J,2) and
        ``K`` (B,3,3) or (3,3): ``r50_op_geo_pose_loss_grad`` takes the place of ``r50_op_mse_loss_grad``, nothing else changes;
        loss2 = [the composite loss, mpjpe] and ``self._geo_out8`` holds the op's eight numbers on the device."""
        b, t = self._check_batch(feats, joints3d)
        if geo is not None:
            gt2d, kmat = self._check_geo(b, t, joints2d, K)
        if masks is None and self.training:
            masks = self.make_dropout_masks(b, t)
        keep_scale = 1.0 / (1.0 - DROPOUT_P)
        lib = _lib.load_library()
        rows, d, o = b * t, self.latent_dim, self.out_dim
        inv = 1.0 / loss_scale
        self._arena.reset()
        self._found.zero_()
        with torch.cuda.device(self._device):
            # ---------------- forward, keeping what the backward needs ----------------
            f = feats.to(torch.float32).contiguous()
            x0 = torch.empty((rows, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), rows, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None, "r50_op_cast_rows")
            x = self._gemm(x0, "input_proj", relu=False)
            phi, saved = self._blocks_forward_saved("f_movie", self.number_blocks, x, b, t, masks, keep_scale)
            y = self._dev["y0"].view(1, o).expand(rows, o).contiguous()
            reg = []
            for i in range(_REG_ITERS):
                inp = torch.empty((rows, self._dp), dtype=self._dtype, device=self._device)
                _lib.check(lib.r50_op_concat_pad(phi.data_ptr(), d, y.data_ptr(), o, rows, inp.data_ptr(), self._dp, self._et, self._stream()),
                           None, "r50_op_concat_pad")
                h1 = self._gemm(inp, "mlp0", relu=True)
                if masks is not None:
                    self._mask_scale(h1, masks[f"f_3D.{i}"], keep_scale)
                h2 = self._gemm(h1, "mlp3", relu=True)
                dy = self._gemm(h2, "mlp5", relu=False)
                _lib.check(lib.r50_op_add_rows(y.data_ptr(), o, dy.data_ptr(), self._op, rows, self._et, self._stream()), None, "r50_op_add_rows")
                reg.append((inp, h1, h2))
            # ---------------- loss and its gradient ----------------
            gt = joints3d.to(torch.float32).contiguous()
            dyacc = torch.empty((rows, o), dtype=torch.float32, device=self._device)
            if geo is None:
                loss2 = torch.empty(2, dtype=torch.float32, device=self._device)
                _lib.check(lib.r50_op_mse_loss_grad(y.data_ptr(), gt.data_ptr(), rows * o, loss_scale, dyacc.data_ptr(), loss2.data_ptr(),
                                                    self._stream()), None, "r50_op_mse_loss_grad")
            else:
                out8 = torch.empty(8, dtype=torch.float32, device=self._device)
                geo_pose_loss_grad(y, gt, gt2d, kmat, b, t, self.joints_num, geo, out8, dy=dyacc, loss_scale=loss_scale,
                                   stream=self._stream())
                loss2 = torch.stack((out8[0], out8[2]))
                self._geo_out8 = out8
            # ---------------- backward: regressor, last iteration first ----------------
            dphi, _g5 = self._regressor_backward(reg, dyacc, rows, inv, keep_scale if masks is not None else 1.0, weights=True)
            dx = torch.empty((rows, d), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(dphi.data_ptr(), rows, d, dx.data_ptr(), d, self._et, self._stream()), None, "r50_op_cast_rows")
            # ---------------- backward: f_movie blocks, last first ----------------
            for i in reversed(range(self.number_blocks)):
                dx = self._block_backward(f"f_movie.blocks.{i}", saved[i], dx, b, t, inv, keep_scale)
            self._wgrad("input_proj.w", dx, x0, inv, False, bias="input_proj.b")
            self._check_arena()                                               # every 16-bit gradient the GEMMs wrote this step
        return y.view(b, t, self.joints_num, 3), loss2

    def _forward_backward_graphed(self, feats: torch.Tensor, joints3d: torch.Tensor, loss_scale: float,
                                  joints2d: Optional[torch.Tensor] = None, K: Optional[torch.Tensor] = None,
                                  geo: Optional[GeoWeights] = None):
        b, t, _ = feats.shape
        key = (b, t, float(loss_scale), self.training) + (geo.as_tuple() if geo is not None else ())
        if geo is not None:
            joints2d, K = self._check_geo(b, t, joints2d, K)
        if key not in self._graphs:
            if len(self._graphs) >= 8:                      # loss scales come and go; keep the cache bounded
                self._graphs.pop(next(iter(self._graphs)))
            s_feats = torch.empty((b, t, 2048), dtype=torch.float32, device=self._device)
            s_gt = torch.empty((b, t, self.joints_num, 3), dtype=torch.float32, device=self._device)
            s_feats.copy_(feats); s_gt.copy_(joints3d)
            s_2d = s_k = None
            if geo is not None:                             # the 2D targets and intrinsics get static buffers of their own
                s_2d, s_k = joints2d.clone(), K.clone()
            eager_arena, self._arena = self._arena, _Arena(self._device, self._dtype)
            try:
                side = torch.cuda.Stream(self._device)
                side.wait_stream(torch.cuda.current_stream(self._device))
                with torch.cuda.stream(side):              # warm-up off the default stream: sizes the arena, loads every kernel
                    for _ in range(2):
                        self.forward_backward(s_feats, s_gt, loss_scale, None, s_2d, s_k, geo)
                torch.cuda.current_stream(self._device).wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    pred, loss2 = self.forward_backward(s_feats, s_gt, loss_scale, None, s_2d, s_k, geo)
                self._graphs[key] = (graph, s_feats, s_gt, pred, loss2, self._arena, s_2d, s_k, self._geo_out8 if geo is not None else None)
            finally:
                self._arena = eager_arena
        graph, s_feats, s_gt, pred, loss2, _, s_2d, s_k, out8 = self._graphs[key]
        s_feats.copy_(feats); s_gt.copy_(joints3d)
        if geo is not None:
            s_2d.copy_(joints2d); s_k.copy_(K)
            self._geo_out8 = out8
        graph.replay()
        return pred, loss2

    def train_step(self, feats: torch.Tensor, joints3d: torch.Tensor, optim: AdamW, scaler: Optional[GradScaler] = None,
                   masks: Optional[Dict[str, torch.Tensor]] = None, group=None, joints2d: Optional[torch.Tensor] = None,
                   K: Optional[torch.Tensor] = None, geo: Optional[GeoWeights] = None) -> Tuple[float, float, bool]:
        """src/train.py:137-176 for one batch: forward + l3d, scaled backward, inf check, AdamW, scale update.
        Returns (loss, mpjpe, skipped).  With ``geo`` (and ``joints2d``, ``K``) the loss is section N's composite and
        ``self.last_losses`` holds the op's eight numbers under ``GEO_KEYS``; they cost a second 32-byte host read after ``loss2``'s
        (the stream is already drained by the overflow flag's read)."""
        scale = scaler.get_scale() if scaler is not None else 1.0
        if self._use_graphs and masks is None:
            _, loss2 = self._forward_backward_graphed(feats, joints3d, scale, joints2d, K, geo)
        else:
            _, loss2 = self.forward_backward(feats, joints3d, scale, masks, joints2d, K, geo)
        found = self._finish_step(optim, scaler, group)
        l = loss2.cpu()
        if geo is not None:
            self.last_losses = dict(zip(GEO_KEYS, self._geo_out8.tolist()))
        return float(l[0]), float(l[1]), found


def mpjpe_m(pred: torch.Tensor, gt: torch.Tensor) -> float:
    """src/train.py:42-45 (reported by train_step from the device; this is the host form for evaluation code)."""
    return float(torch.norm(pred - gt, dim=-1).mean().item())


def train(model: TrainableHead, loader, optim: AdamW, scaler: Optional[GradScaler], device, log_every: int = 500):
    """The epoch loop of the reference's ``train()`` (src/train.py:114-215): same batch tuple, same returned (mean loss, mean mpjpe)."""
    model.train()
    running_loss = running_mpjpe = 0.0
    n_batches = 0
    for it, batch in enumerate(loader):
        feats, joints3d = batch[0].to(device, non_blocking=True), batch[1].to(device, non_blocking=True)
        loss, mpjpe, _ = model.train_step(feats, joints3d, optim, scaler)
        running_loss += loss
        running_mpjpe += mpjpe
        n_batches += 1
        if log_every > 0 and (it + 1) % log_every == 0:
            print(f"[3D]  iter {it + 1:05d} | loss {running_loss / n_batches:.6f} | mpjpe {running_mpjpe / n_batches:.3f}")
    return running_loss / max(n_batches, 1), running_mpjpe / max(n_batches, 1)


# ---- the phase-1 driver: src/train.py:219-465 (evaluate, checkpoints, LR schedule, early stopping, CLI) -----------------------
H36M_ROOT = "/home/s26ldeso/Human3.6M_preprocessed_resnet_features"    # the reference's defaults (src/config.py)
SEQ_LEN, BATCH_SIZE, LR, EPOCHS, JOINTS_NUM = 40, 32, 1e-4, 50, 17
TRAIN_SUBJECTS, VAL_SUBJECTS = [1, 6, 7, 8], [5]                          # hard-coded at src/train.py:312,318


def default_state_dict(latent_dim: int = 1024, joints_num: int = JOINTS_NUM, number_blocks: int = 2,
                       seed: int = 0) -> Dict[str, torch.Tensor]:
    """Initial weights with the distribution of torch's default initialisation of the reference module: nn.Linear / nn.Conv1d
    weight and bias U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (kaiming_uniform with a = sqrt(5)), GroupNorm weight 1 / bias 0, y0 zero.
    Drawn from ``torch.Generator().manual_seed(seed)``; the reference draws from the unseeded global generator."""
    gen = torch.Generator().manual_seed(seed)
    keys = expected_keys(latent_dim, joints_num, number_blocks)
    sd: Dict[str, torch.Tensor] = {}
    for k, shape in keys.items():
        if k == "f_3D.y0" or (".gn" in k and k.endswith(".bias")):
            sd[k] = torch.zeros(shape)
        elif ".gn" in k:
            sd[k] = torch.ones(shape)
        else:
            w = keys[k[: -len("bias")] + "weight"] if k.endswith(".bias") else shape
            bound = (w[1] * (w[2] if len(w) == 3 else 1)) ** -0.5
            sd[k] = torch.empty(shape).uniform_(-bound, bound, generator=gen)
    return sd


def dropout_generator(seed: int, epoch: int, it: int, device) -> torch.Generator:
    """The generator of one step's dropout masks: seeded from (seed, epoch, iteration) alone, so an epoch draws the same masks
    whether the run was resumed or not."""
    key = int.from_bytes(hashlib.sha256(f"{seed}/{epoch}/{it}".encode()).digest()[:8], "little") & ((1 << 63) - 1)
    return torch.Generator(device=device).manual_seed(key)


class CosineLR:
    """The reference's per-epoch learning rate: a real ``torch.optim.lr_scheduler.CosineAnnealingLR(optim, T_max=epochs)``
    (src/train.py:395) on a proxy ``torch.optim.AdamW`` holding the hyperparameters, driven in the reference's order: built
    fresh, THEN the checkpoint's param group loaded into the optimizer (:400-405, ``load_group``), ``step()`` after each epoch's
    evaluation (:425).  So a resumed run restarts the scheduler's counter at 0 from the loaded LR and applies the recursive
    cosine factor from there: its LRs are not those of an uninterrupted run.  That is the reference's behaviour, kept on purpose."""

    def __init__(self, lr: float, epochs: int):
        self.proxy = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=lr, weight_decay=1e-2)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.proxy, T_max=epochs)

    @property
    def lr(self) -> float:
        return float(self.proxy.param_groups[0]["lr"])

    @property
    def initial_lr(self) -> float:
        return float(self.proxy.param_groups[0]["initial_lr"])

    def load_group(self, optim_state: dict) -> None:
        """What ``optim.load_state_dict(ckpt["optim"])`` does to the param group: the saved hyperparameters replace the current ones."""
        self.proxy.param_groups[0].update({k: v for k, v in optim_state["param_groups"][0].items() if k != "params"})

    def step(self) -> None:
        self.proxy.step()             # no gradients, so nothing changes; it tells the scheduler the optimizer stepped first
        self.scheduler.step()


@torch.no_grad()
def evaluate_geo(head: PHDFor3DJoints, store, batch_size: int, geo: GeoWeights, batches=None) -> Dict[str, float]:
    """``evaluate``'s pass with section N's terms: per batch the head in eval mode through ``joints()`` and one
    ``r50_op_geo_pose_loss_grad`` call with ``dy = NULL``; the eight numbers are summed on the device and read once.  Returns the mean
    over batches of each of ``GEO_KEYS`` (``n_clamped``: the TOTAL over the pass, it is a count)."""
    if batches is None:
        batches = (list(range(s, min(s + batch_size, len(store)))) for s in range(0, len(store), batch_size))
    was_training = head.training
    head.train(False)
    dev = head._device
    try:
        with torch.cuda.device(dev):
            acc = torch.zeros(8, dtype=torch.float64, device=dev)
            out8 = torch.empty(8, dtype=torch.float32, device=dev)
            n = 0
            for idx in batches:
                batch = store.get_batch(idx)
                pred = head.joints(batch[0])
                b, t = pred.shape[0], pred.shape[1]
                gt = batch[1].to(device=dev, dtype=torch.float32).contiguous()
                gt2d = batch[2].to(device=dev, dtype=torch.float32).contiguous()
                geo_pose_loss_grad(pred.contiguous(), gt, gt2d, expand_intrinsics(batch[3].to(dev), b), b, t, head.joints_num, geo, out8,
                                   stream=head._stream())
                acc += out8.double()
                n += 1
            sums = acc.tolist()
    finally:
        head.train(was_training)
    out = {k: v / max(n, 1) for k, v in zip(GEO_KEYS, sums)}
    out["n_clamped"] = sums[7]
    return out


@torch.no_grad()
def evaluate(head: PHDFor3DJoints, store, batch_size: int, test_set: bool = False, batches=None,
             geo: Optional[GeoWeights] = None) -> Tuple[float, float, float, float]:
    """src/train.py:219-280: (loss, mpjpe, l3d, 0.0), each the mean over batches of the per-batch mean.  The items of ``store``
    in order, ``batch_size`` at a time, the last batch kept even if short (the reference's val loader: shuffle=False,
    drop_last=False).  The head runs in eval mode through ``joints()`` (no f_AR); one ``r50_op_pose_metrics`` launch per batch
    adds into a device accumulator, read once at the end.  The head's mode is restored; its weights are not touched.
    ``test_set``: the store yields the meta list as a fifth field (ignored here), as the reference's flag says.
    ``batches``: an iterable of index lists to evaluate instead, in its order (e.g. the reference's shuffled test loader,
    src/results.py:162-170); ``batch_size`` is then unused.
    ``geo``: the pass is ``evaluate_geo``'s: (composite loss, mpjpe, l3d, l2d).  The reference's four-value return has no room for
    the other terms, so they are left on the head as a plain attribute, ``head.last_eval_geo`` (a dict over ``GEO_KEYS``, replaced by
    every such pass); call ``evaluate_geo`` directly to get the dict as a return value."""
    del test_set                      # only changes the batch tuple's length in the reference; get_batch's first two fields serve
    if geo is not None:
        g = evaluate_geo(head, store, batch_size, geo, batches)
        head.last_eval_geo = g
        return g["loss"], g["mpjpe"], g["l3d"], g["l2d"]
    if batches is None:
        batches = (list(range(s, min(s + batch_size, len(store)))) for s in range(0, len(store), batch_size))
    was_training = head.training
    head.train(False)
    lib = _lib.load_library()
    dev = head._device
    try:
        with torch.cuda.device(dev):
            acc = torch.zeros(3, dtype=torch.float64, device=dev)
            for idx in batches:
                batch = store.get_batch(idx)
                pred = head.joints(batch[0])
                gt = batch[1].to(device=dev, dtype=torch.float32).contiguous()
                rows = pred.shape[0] * pred.shape[1]
                _lib.check(lib.r50_op_pose_metrics(pred.data_ptr(), gt.data_ptr(), rows, head.joints_num, acc.data_ptr(),
                                                   head._stream()), None, "r50_op_pose_metrics")
            l3d, mpjpe, n = acc.tolist()
    finally:
        head.train(was_training)
    n = max(n, 1.0)
    return l3d / n, mpjpe / n, l3d / n, 0.0


def train_epoch(head: TrainableHead, store, sampler, optim: AdamW, scaler: Optional[GradScaler], seed: int, epoch: int,
                log_every: int = 500, geo: Optional[GeoWeights] = None):
    """One training epoch of the driver (src/train.py:114-215): the batches of ``sampler`` (its epoch already set) drawn from
    ``store``, one ``train_step`` each with the masks of ``dropout_generator(seed, epoch, it)``.
    Returns (mean loss, mean mpjpe, applied steps, skipped steps); with ``geo`` the steps run section N's composite loss on the
    batch's joints2d and K and a fifth value follows: the means of ``GEO_KEYS`` over the batches (``n_clamped``: the total).  The
    length of the result therefore depends on ``geo`` (4 without, 5 with): callers that pass ``geo`` unpack five."""
    head.train()
    running_loss = running_mpjpe = 0.0
    n_batches = skipped = 0
    geo_sums = {k: 0.0 for k in GEO_KEYS}
    for it, idx in enumerate(sampler):
        batch = store.get_batch(idx)
        feats, joints3d = batch[:2]
        masks = head.make_dropout_masks(feats.shape[0], feats.shape[1], generator=dropout_generator(seed, epoch, it, head._device))
        if geo is None:
            loss, mpjpe, found = head.train_step(feats, joints3d, optim, scaler, masks=masks)
        else:
            loss, mpjpe, found = head.train_step(feats, joints3d, optim, scaler, masks=masks, joints2d=batch[2], K=batch[3], geo=geo)
            for k in geo_sums:
                geo_sums[k] += head.last_losses[k]
        running_loss += loss
        running_mpjpe += mpjpe
        n_batches += 1
        skipped += int(found)
        if log_every > 0 and (it + 1) % log_every == 0:
            print(f"[3D]  iter {it + 1:05d}/{len(sampler):05d} | loss {running_loss / n_batches:.6f} | mpjpe {running_mpjpe / n_batches:.3f}")
    out = (running_loss / max(n_batches, 1), running_mpjpe / max(n_batches, 1), n_batches - skipped, skipped)
    if geo is None:
        return out
    means = {k: v / max(n_batches, 1) for k, v in geo_sums.items()}
    means["n_clamped"] = geo_sums["n_clamped"]
    return out + (means,)


def save_checkpoint(path: str, head: TrainableHead, optim: AdamW, epoch: int, best_val: float, args) -> None:
    """src/train.py:61-76: {"epoch", "best_val", "model" (the reference's state-dict keys), "optim" (torch.optim.AdamW's
    layout), "args"}.  Tensors, numbers, strings and lists only: it loads with ``torch.load(weights_only=True)``.
    With ``optim.ema`` set (section S) one more key, "ema": ``WeightEMA.state_dict()``; "model" stays the raw weights."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ckpt = {"epoch": epoch, "best_val": best_val, "model": head.state_dict(), "optim": optim.state_dict(),
            "args": dict(vars(args)) if isinstance(args, argparse.Namespace) else dict(args)}
    if optim.ema is not None:
        ckpt["ema"] = optim.ema.state_dict()
    torch.save(ckpt, path)


def load_checkpoint(path: str, head: TrainableHead, optim: AdamW) -> dict:
    """Load a checkpoint of ``save_checkpoint`` (or of the reference) into ``head`` and ``optim``; returns the whole dict.  With
    ``optim.ema`` set, the file's "ema" is loaded into it; a file without one (a run that had no EMA) starts the average from the
    loaded raw weights."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    head.load_state_dict(ckpt["model"], strict=True)
    optim.load_state_dict(ckpt["optim"])
    if optim.ema is not None:
        if "ema" in ckpt:
            optim.ema.load_state_dict(ckpt["ema"])
        else:
            optim.ema.flat.copy_(head.flat_master)
            optim.ema.updates = 0
    return ckpt


def build_parser() -> argparse.ArgumentParser:
    """The reference's flags and defaults (src/train.py:283-299, src/config.py), then this project's extras."""
    p = argparse.ArgumentParser("Phase-1 training: freeze ResNet, train f_movie + f_3D (3D joints + 2D reprojection)")
    p.add_argument("--train", type=str, default=H36M_ROOT)
    p.add_argument("--val", type=str, default=H36M_ROOT)
    p.add_argument("--seq-len", type=int, default=SEQ_LEN, help="accepted, no effect (as in the reference)")
    p.add_argument("--batch-size", type=int, default=BATCH_SIZE)
    p.add_argument("--lr", type=float, default=LR)
    p.add_argument("--epochs", type=int, default=EPOCHS)
    p.add_argument("--num-workers", type=int, default=2, help="accepted, no effect: batches come from HBM")
    p.add_argument("--lambda-2d", type=float, default=1e-6, help="2D reprojection loss weight (accepted, no effect here, as in the reference; "
                                                                   "python -m implementation_phd_lab_vision_amd.train_geo applies it)")
    p.add_argument("--outdir", type=str, default="./runs/phase1")
    p.add_argument("--resume", type=str, default=None)
    p.add_argument("--log-every", type=int, default=500)
    p.add_argument("--early-stop-patience", type=int, default=10,
                   help="Stop if val MPJPE doesn't improve for this many epochs (0 disables).")
    p.add_argument("--early-stop-min-delta", type=float, default=0.0, help="Minimum MPJPE improvement to reset patience.")
    p.add_argument("--precision", choices=("fp16", "bf16"), default="fp16", help="16-bit type of the head's GEMMs")
    p.add_argument("--seed", type=int, default=0, help="seeds the initial weights and the dropout masks")
    p.add_argument("--train-subjects", type=int, nargs="+", default=list(TRAIN_SUBJECTS))
    p.add_argument("--val-subjects", type=int, nargs="+", default=list(VAL_SUBJECTS))
    # Gradient clipping and EMA weights.  No defaults: a run without these flags has the namespace -- and
    # the "args" its checkpoints record -- it had before they existed.  Read them with clip_ema_options().
    p.add_argument("--clip-grad-norm", type=float, default=argparse.SUPPRESS, metavar="FLOAT",
                   help="clip the global L2 norm of the gradient to this (torch.nn.utils.clip_grad_norm_), > 0 (default: no clipping)")
    p.add_argument("--ema-decay", type=float, default=argparse.SUPPRESS, metavar="FLOAT",
                   help="keep an exponential moving average of the weights with this decay, in (0, 1); validation, best.pt and early "
                        "stopping then follow the averaged weights (default: no EMA)")
    p.add_argument("--ema-no-warmup", action="store_true", default=argparse.SUPPRESS,
                   help="with --ema-decay: use the decay from the first update on instead of min(decay, (1 + u) / (10 + u))")
    return p


def clip_ema_options(args: argparse.Namespace) -> Tuple[Optional[float], Optional[float], bool]:
    """(--clip-grad-norm or None, --ema-decay or None, EMA warm-up on) of any stage's parsed arguments."""
    return getattr(args, "clip_grad_norm", None), getattr(args, "ema_decay", None), not getattr(args, "ema_no_warmup", False)


def validate_clip_ema(p: argparse.ArgumentParser, args: argparse.Namespace) -> argparse.Namespace:
    """Section S's rules on parsed arguments (``p.error`` on a breach); every stage's driver calls it."""
    clip, decay, _ = clip_ema_options(args)
    if clip is not None and not (clip > 0 and clip != float("inf")):          # also refuses nan
        p.error("--clip-grad-norm must be finite and > 0")
    if decay is not None and not 0.0 < decay < 1.0:
        p.error("--ema-decay must lie in (0, 1)")
    if hasattr(args, "ema_no_warmup") and decay is None:
        p.error("--ema-no-warmup applies together with --ema-decay only")
    return args


def main(argv: Optional[List[str]] = None) -> float:
    """``python src/train.py`` (src/train.py:283-465) on one MI355X.  Per epoch, in the reference's order: train, evaluate,
    scheduler step, ``last.pt``, ``best.pt`` when val MPJPE improved by more than ``--early-stop-min-delta``, patience counter.
    ``--resume`` loads model and optimizer (a missing file is ignored; GradScaler state is not saved), as the reference does.
    Also prints one JSON line per epoch.  Returns the best val MPJPE."""
    p = build_parser()
    return run(validate_clip_ema(p, p.parse_args(argv)))


def geo_json(prefix: str, values: Dict[str, float]) -> Dict[str, float]:
    """The geometric numbers of one pass for the per-epoch JSON line: ``{prefix}_{l2d, reproj_px, l_vel, l_bone, n_clamped}``."""
    return {f"{prefix}_{k}": values[k] for k in GEO_EXTRA_KEYS}


def validate_with_ema(run: "Run", validate):
    """The validation of one epoch.  ``validate()`` runs the stage's validation pass on the head's current weights and returns
    (score, JSON fields, the ``Val:`` line).  Without EMA that is the result.  With it (section S) the pass runs twice, once on the
    raw weights and once inside ``head.swapped_weights(ema.flat)``: the averaged weights' score and fields are returned (they select
    ``best.pt`` and drive early stopping), the raw weights' numbers follow under the same keys with a ``_raw`` suffix, and both lines
    are kept."""
    if run.optim.ema is None:
        score, fields, line = validate()
        return score, fields, (line,)
    _, raw_fields, raw_line = validate()
    with run.head.swapped_weights(run.optim.ema.flat):
        score, fields, line = validate()
    fields = dict(fields)
    fields.update({f"{k}_raw": v for k, v in raw_fields.items()})
    return score, fields, (line.replace("Val:  ", "Val:   [EMA]", 1), raw_line.replace("Val:  ", "Val:   [raw]", 1))


def clip_fields(run: "Run") -> Dict[str, float]:
    """The epoch's gradient-norm numbers for its JSON line (empty without ``--clip-grad-norm``); resets the device counters."""
    if run.optim.max_grad_norm is None:
        return {}
    st = run.head.clip_stats(reset=True)
    return {k: st[k] for k in ("grad_norm_mean", "grad_norm_max", "clipped_frac")}


@dataclass
class Run:
    """What ``open_run`` set up and ``fit`` drives."""
    device: torch.device
    train_set: object
    val_set: object
    sampler: object
    head: FlatTrainableHead
    optim: AdamW
    scaler: GradScaler
    schedule: CosineLR
    start_epoch: int
    best_val: float


def open_run(args: argparse.Namespace, make_head) -> Run:
    """The set-up every stage's driver shares: the device, ``--outdir``, the train and validation stores in HBM, the sampler,
    ``make_head(device)`` (the stage's head, loaded and on the device), AdamW / GradScaler / CosineLR, and ``--resume`` (model and
    optimizer; a missing file is ignored; GradScaler state is not saved), as the reference does.  ``--clip-grad-norm`` and
    ``--ema-decay`` (section S) become ``optim.max_grad_norm`` and ``optim.ema``; ``--resume`` then restores the EMA too."""
    from .feature_store import DeviceFeatureStore
    from .samplers import MixedShardBatchSampler

    if not torch.cuda.is_available():
        raise _lib.R50Error("the training driver runs on an MI355X only; there is no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.outdir, exist_ok=True)
    train_set = DeviceFeatureStore(args.train, subjects=args.train_subjects, augment=True, device=device)
    val_set = DeviceFeatureStore(args.val, subjects=args.val_subjects, device=device)
    sampler = MixedShardBatchSampler(train_set, batch_size=args.batch_size, shuffle=True, drop_last=True, seed=0)
    head = make_head(device)
    optim = AdamW(head, lr=args.lr, weight_decay=1e-2)
    clip, decay, warmup = clip_ema_options(args)
    optim.max_grad_norm = clip
    if decay is not None:
        optim.ema = WeightEMA(head, decay, warmup)
    run = Run(device, train_set, val_set, sampler, head, optim, GradScaler(), CosineLR(args.lr, args.epochs), 0, float("inf"))
    if args.resume and os.path.isfile(args.resume):
        ckpt = load_checkpoint(args.resume, head, optim)
        run.schedule.load_group(ckpt["optim"])
        run.start_epoch = int(ckpt.get("epoch", 0)) + 1
        run.best_val = float(ckpt.get("best_val", run.best_val))
        print(f"Resumed from {args.resume} (start_epoch={run.start_epoch}, best_val={run.best_val:.4f})")
    return run


def head_from_checkpoint(args: argparse.Namespace, cls, **kwargs):
    """``make_head`` of the stages that start from weights: ``cls`` at the dimensions of ``--init`` (or, without it, ``--resume``),
    loaded with that state.  A state that carries the hallucinator (``f_hal.*``) gets a head built with
    ``hallucinator=True``: the stage leaves those four tensors as they are and its checkpoints keep them."""
    from .model import has_hallucinator
    from .results import infer_head_dims, load_head_state

    def make_head(device):
        state = load_head_state(args.init, getattr(args, "weights_from", "auto")) if args.init else load_head_state(args.resume, "model")
        latent_dim, joints_num, number_blocks = infer_head_dims(state)
        extra = {"hallucinator": True} if has_hallucinator(state) else {}
        head = cls(latent_dim, joints_num, number_blocks, precision=args.precision, **kwargs, **extra)
        head.load_state_dict(state, strict=True)
        return head.to(device)
    return make_head


def fit(run: Run, args: argparse.Namespace, banner: Sequence[str], epoch_fn, score_label: str, epoch_note=None) -> float:
    """The epoch loop of every stage's driver, in the reference's order (src/train.py:407-465).  Per epoch: the sampler's epoch and
    the schedule's LR handed to the optimizer, ``epoch_fn(epoch)`` (trains and validates; returns the validation score, the epoch's
    JSON fields without ``epoch`` and ``lr``, and the ``Train:`` / ``Val:`` lines), the scheduler step (the saved optimizer state
    carries the scheduler's next LR, as torch's does), the prints and the JSON line, ``last.pt``, ``best.pt`` when the score improved
    by more than ``--early-stop-min-delta``, the patience counter.  ``epoch_note(epoch)``: text appended to the epoch's header.
    Returns the best score."""
    head, optim, schedule, best_val, no_improve_epochs = run.head, run.optim, run.schedule, run.best_val, 0
    for text in banner:
        print(text)
    for epoch in range(run.start_epoch, args.epochs):
        run.sampler.set_epoch(epoch)
        optim.lr, optim.initial_lr = schedule.lr, schedule.initial_lr
        print(f"\nEpoch {epoch + 1}/{args.epochs}" + (epoch_note(epoch) if epoch_note is not None else ""))
        t0 = time.time()
        epoch_lr = optim.lr
        score, fields, lines = epoch_fn(epoch)
        schedule.step()
        optim.lr = schedule.lr
        for text in lines:
            print(text)
        print(f"Epoch time: {time.time() - t0:.2f}s")
        print(json.dumps({"epoch": epoch, "lr": epoch_lr, **fields}))

        save_checkpoint(os.path.join(args.outdir, "last.pt"), head, optim, epoch, best_val, args)
        if (best_val - score) > args.early_stop_min_delta:
            best_val = score
            no_improve_epochs = 0
            save_checkpoint(os.path.join(args.outdir, "best.pt"), head, optim, epoch, best_val, args)
            print(f"New best val {score_label}: {best_val:.3f} (saved best.pt)")
        else:
            no_improve_epochs += 1
            print(f"No improvement for {no_improve_epochs}/{args.early_stop_patience} epochs "
                  f"(best {best_val:.3f}, current {score:.3f})")
        if args.early_stop_patience > 0 and no_improve_epochs >= args.early_stop_patience:
            print(f"Early stopping triggered at epoch {epoch + 1}. Best val {score_label}: {best_val:.3f}")
            break
    print("\nDone.")
    print(f"Best val {score_label}: {best_val:.3f}")
    return best_val


def run(args: argparse.Namespace, geo_for_epoch=None) -> float:
    """``main``'s body on parsed arguments.  ``geo_for_epoch``: None (phase 1 as the reference runs it), or a function
    epoch -> ``GeoWeights`` (``train_geo``): the epoch then trains and validates under section N's composite loss with those weights,
    and its JSON line gains the geometric numbers and ``lambda_2d_active``."""
    def make_head(device):
        head = TrainableHead(1024, JOINTS_NUM, 2, precision=args.precision)
        head.load_state_dict(default_state_dict(1024, JOINTS_NUM, 2, seed=args.seed))
        return head.to(device)

    r = open_run(args, make_head)

    def epoch_fn(epoch):
        geo = geo_for_epoch(epoch) if geo_for_epoch is not None else None
        tr_loss, tr_mpjpe, steps, skipped, *tr_geo = train_epoch(r.head, r.train_set, r.sampler, r.optim, r.scaler, args.seed, epoch,
                                                                 args.log_every, geo=geo)
        lambda_2d = geo.lambda_2d if geo is not None else args.lambda_2d      # the weight this epoch applied (0 during the 2D warm-up)

        def validate():
            va_loss, va_mpjpe, va_l3d, va_l2d = evaluate(r.head, r.val_set, args.batch_size, geo=geo)
            va = {"val_loss": va_loss, "val_mpjpe": va_mpjpe}
            if geo is not None:
                va.update(geo_json("val", r.head.last_eval_geo))
            return va_mpjpe, va, f"Val:   loss={va_loss:.6f} (3d {va_l3d:.6f} + {lambda_2d:.3g}*2d {va_l2d:.6f}) | mpjpe={va_mpjpe:.3f}"

        score, va_fields, va_lines = validate_with_ema(r, validate)
        fields = {"train_loss": tr_loss, "train_mpjpe": tr_mpjpe, "steps": steps, "skipped": skipped, "val_loss": va_fields.pop("val_loss"),
                  "val_mpjpe": va_fields.pop("val_mpjpe")}
        if geo is not None:
            fields.update(geo_json("train", tr_geo[0]))
        fields.update(va_fields)
        if geo is not None:
            fields["lambda_2d_active"] = geo.lambda_2d
        fields.update(clip_fields(r))
        return score, fields, (f"Train: loss={tr_loss:.6f} | mpjpe={tr_mpjpe:.3f}",) + va_lines

    return fit(r, args, ("===== Phase-1 training =====", f"Device: {r.device} ({args.precision})",
                         f"Train clips: {len(r.train_set)} | Val clips: {len(r.val_set)}",
                         f"Batch size: {args.batch_size} | LR: {args.lr} | seed: {args.seed}", "============================"),
               epoch_fn, "MPJPE")


if __name__ == "__main__":
    main()
