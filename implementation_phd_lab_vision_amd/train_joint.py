"""Joint training of the lifting head on one MI355X: input_proj, f_movie, f_AR and f_3D under one loss (DESIGN.md "f joint",
INTEGRATION.md section M).  ``python -m implementation_phd_lab_vision_amd.train_joint``.

Phase 1 (train.py) freezes f_AR, as the reference does (src/train.py:375-376); phase 2 and the rollout objective (train_ar.py) train
f_AR alone on a frozen f_movie.  The paper the reference implements trains the strip encoder and the predictor together, and the
reference's ``PHDFor3DJoints.forward(feats, predict_future=True)`` returns every output such a loss needs (src/model.py:158-178).
This project's definition of the joint program, in the reference's idiom (tests/golden/make_golden_train_joint.py runs it on the
reference module itself)::

    model = PHD(latent_dim, 17, number_blocks)          # weights: a phase-1 / phase-2 / rollout checkpoint's "model", or a state dict
    for p in model.parameters(): p.requires_grad = True
    optim = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=1e-2)   # named_parameters() order
    scaler = torch.amp.GradScaler("cuda")
    model.train()                                        # every dropout site active: f_movie, f_AR, both f_3D calls
    with torch.autocast("cuda", dtype=torch.float16):
        phi, phi_hat, joints_phi, joints_hat = model(feats, predict_future=True)
        l3d     = (joints_phi - joints3d).pow(2).mean()                       # phase 1's term, all frames
        l3d_hat = (joints_hat[:, 1:] - joints3d[:, 1:]).pow(2).mean()         # phase 2's terms, frames s >= 1
        l_lat   = (phi_hat[:, 1:] - phi[:, 1:].detach()).pow(2).mean()
        loss    = l3d + args.lambda_future * l3d_hat + args.lambda_latent * l_lat
    scaler.scale(loss).backward(); scaler.step(optim); scaler.update()

The choices that are this project's, not the paper's:

* The latent target is detached, as in phase 2.  f_movie is trained by l3d (through f_3D(phi)) and by l3d_hat and l_lat through
  f_AR's INPUT; it is never pulled toward f_AR's prediction through the target.  Without the detach, l_lat could shrink by making
  the strips constant.
* Everything runs in train mode.  The two calls of f_3D draw independent dropout masks, and the detached target phi carries
  f_movie's dropout: what ``model.train()`` gives on the reference module.
* ``--lambda-future`` and ``--lambda-latent`` default to 1.0; no run has measured good values.
* lambda = 0 still applies AdamW's weight decay to f_AR: f_AR stays in the graph and its gradients are zeros, not None (on the
  reference module at number_blocks = 2: 48 parameters, f_AR's 24 with all-zero gradients).  The device does the same.
* The optimizer starts fresh from ``--init``: no checkpoint of another phase holds state for every parameter.
* ``best.pt`` and early stopping follow val ``mpjpe + mpjpe_hat``, which does not depend on the lambdas, so runs with different
  weights compare.

``JointTrainableHead`` keeps every parameter in flat fp32 master / 16-bit / gradient buffers in the GEMM layouts of
``train.TrainableHead`` and ``train_ar.ARTrainableHead``.  One step, eager launches through the C ABI: input_proj and f_movie forward
(saved; f_movie's last conv2 stores straight into the first half of a stacked (2*B*T, D) strip buffer), f_AR forward (saved), the
phi_hat shift into the second half, the regressor ONCE over the 2*B*T stacked rows (each half its own dropout masks),
``r50_op_joint_pose_loss_grad``, the regressor's backward over the stacked rows with weight gradients (bias gradients by
``r50_op_colsum_split``: ``r50_op_colsum``'s bits, spread over the chip), ``r50_op_ar_latent_grad`` on
the second half of the strip gradient, f_AR's backward with weight gradients (block 0's gn1 backward plus the skip connection
gives f_AR's gradient with respect to phi), the gradient of phi = the regressor's first half + f_AR's input gradient, f_movie's
backward and input_proj's dW, one overflow check over the 16-bit arena; then ``all_reduce_gradients``, ``check_finite``, AdamW,
the scaler.  No torch autograd, no CPU fallback.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .model import _AR_BLOCKS, _REG_HIDDEN, _REG_ITERS
from .train import (DROPOUT_P, GEO_EXTRA_KEYS, GEO_KEYS, AdamW, GeoWeights, GradScaler, TrainableHead, build_parser as _phase1_parser,
                    dropout_generator, fit, geo_pose_loss_grad, head_from_checkpoint, open_run, clip_fields, validate_clip_ema, validate_with_ema)
from .trainable import FlatItem, FlatTrainableHead, block_items, input_proj_items, regressor_items

LAMBDA_FUTURE = 1.0
LAMBDA_LATENT = 1.0
_BLOCK_PARAMS = ("gn1", "conv1.conv", "gn2", "conv2.conv")      # a ResidualBlock registers gn1, conv1, gn2, conv2 (src/model.py:39-44)


def joint_trainable_names(number_blocks: int) -> List[str]:
    """``[n for n, _ in model.named_parameters()]`` of the reference module with every parameter trainable: f_movie's blocks, f_AR's
    blocks, f_3D's three Linears, input_proj (src/model.py:142-146); ``f_3D.y0`` is a buffer.  The numbering of the optimizer state."""
    names: List[str] = []
    for net, nb in (("f_movie", number_blocks), ("f_AR", _AR_BLOCKS)):
        for i in range(nb):
            for m in _BLOCK_PARAMS:
                names += [f"{net}.blocks.{i}.{m}.weight", f"{net}.blocks.{i}.{m}.bias"]
    for j in (0, 3, 5):
        names += [f"f_3D.mlp.{j}.weight", f"f_3D.mlp.{j}.bias"]
    return names + ["input_proj.weight", "input_proj.bias"]


def joint_items(number_blocks: int) -> List[FlatItem]:
    """The joint flat buffer, in order: f_movie's blocks, f_AR's blocks (each gn1, conv1, gn2, conv2), the regressor, input_proj."""
    items: List[FlatItem] = []
    for net, nb in (("f_movie", number_blocks), ("f_AR", _AR_BLOCKS)):
        for i in range(nb):
            items += block_items(f"{net}.blocks.{i}")
    return items + regressor_items() + input_proj_items()


class JointTrainableHead(FlatTrainableHead):
    """``PHDFor3DJoints`` with every parameter trainable in flat fp32 / 16-bit buffers."""

    _no_transpose = frozenset({"input_proj.w"})
    _clip_rule = (2, "joint training")

    def __init__(self, latent_dim: int = 2048, joints_num: int = 17, number_blocks: int = 3, precision: str = "fp16",
                 lambda_future: float = LAMBDA_FUTURE, lambda_latent: float = LAMBDA_LATENT, hallucinator: bool = False):
        super().__init__(latent_dim, joints_num, number_blocks, precision, hallucinator)
        if self.number_blocks < 1:
            raise ValueError("joint training needs at least one f_movie block (its last conv2 stores phi)")
        self.lambda_future = float(lambda_future)
        self.lambda_latent = float(lambda_latent)

    def _flat_items(self) -> List[FlatItem]:
        return joint_items(self.number_blocks)

    def trainable_parameter_names(self) -> List[str]:
        """The names of the optimizer's parameters, in its numbering: ``joint_trainable_names(number_blocks)``."""
        return joint_trainable_names(self.number_blocks)

    def _dropout_sites(self) -> List[Tuple[str, int]]:
        """One per f_movie block and one per f_AR block after its conv1 (src/model.py:52); one per iteration of f_3D(phi) ("f_3D.i")
        and then of f_3D(phi_hat) ("f_3D_hat.i") after the regressor's first ReLU (:98).  The f_movie and f_3D(phi) entries are
        phase 1's sites under phase 1's names."""
        return [(f"{net}.blocks.{i}", self.latent_dim) for net, nb in (("f_movie", self.number_blocks), ("f_AR", _AR_BLOCKS))
                for i in range(nb)] + [(f"{site}.{i}", _REG_HIDDEN) for site in ("f_3D", "f_3D_hat") for i in range(_REG_ITERS)]

    def _upload(self) -> None:
        super()._upload()
        self._colsum_part = torch.empty(16 * max(self.latent_dim, _REG_HIDDEN, self._op), dtype=torch.float32, device=self._device)

    def _bias_grad(self, dy: torch.Tensor, gb: torch.Tensor, inv_scale: float, accumulate: bool) -> None:
        """By ``r50_op_colsum_split``: ``r50_op_colsum``'s bits, spread over the chip (one-workgroup-per-64-columns column sums over
        the stacked 2*B*T rows were the step's largest cost)."""
        assert 16 * dy.shape[1] <= self._colsum_part.numel()
        _lib.check(_lib.load_library().r50_op_colsum_split(dy.data_ptr(), dy.shape[0], dy.shape[1], dy.shape[1], inv_scale,
                                                            self._colsum_part.data_ptr(), gb.data_ptr(), int(accumulate), self._et,
                                                            self._stream()), None, "r50_op_colsum_split")

    # ---- launches -------------------------------------------------------------------------------
    def _joint_pose_loss(self, y: torch.Tensor, gt: torch.Tensor, b: int, t: int, lambda_future: float, loss_scale: float,
                         dy: torch.Tensor, out: torch.Tensor) -> None:
        """out[0:4] = [l3d, mpjpe, l3d_hat, mpjpe_hat]; dy (2*B*T, J*3) fp32 = the gradients of l3d and lambda_future * l3d_hat,
        * loss_scale (0 on the frame-0 rows of the second half)."""
        _lib.check(_lib.load_library().r50_op_joint_pose_loss_grad(y.data_ptr(), gt.data_ptr(), b, t, self.joints_num, lambda_future,
                                                                    loss_scale, dy.data_ptr(), out.data_ptr(), self._stream()), None,
                   "r50_op_joint_pose_loss_grad")

    _check_geo = TrainableHead._check_geo

    def _geo_pose_loss(self, y: torch.Tensor, gt: torch.Tensor, gt2d: torch.Tensor, kmat: torch.Tensor, b: int, t: int, geo: GeoWeights,
                       lambda_future: float, loss_scale: float, dy: Optional[torch.Tensor], out: torch.Tensor) -> torch.Tensor:
        """``_joint_pose_loss`` under section N's composite loss: two ``r50_op_geo_pose_loss_grad`` launches over the stacked rows, the
        first half at s0 = 0, term_scale = 1, the second at s0 = 1 (frame 0 of phi_hat is zeros), term_scale = lambda_future.
        out[0:4] as ``_joint_pose_loss`` fills it; returns the two halves' out8 as a (2, 8) fp32 device tensor."""
        if t < 3 and geo.lambda_vel != 0:
            raise ValueError("geo: the velocity term of joints_hat[:, 1:] needs clips of at least 3 frames")
        rows = b * t
        out16 = torch.empty((2, 8), dtype=torch.float32, device=self._device)
        yv = y.view(2, rows, self.out_dim)
        dv = dy.view(2, rows, self.out_dim) if dy is not None else (None, None)
        geo_pose_loss_grad(yv[0], gt, gt2d, kmat, b, t, self.joints_num, geo, out16[0], dy=dv[0], loss_scale=loss_scale, stream=self._stream())
        geo_pose_loss_grad(yv[1], gt, gt2d, kmat, b, t, self.joints_num, geo, out16[1], dy=dv[1], s0=1, term_scale=lambda_future,
                           loss_scale=loss_scale, stream=self._stream())
        out[0:2].copy_(out16[0, 1:3])
        out[2:4].copy_(out16[1, 1:3])
        return out16

    def _latent_loss(self, ar: torch.Tensor, phi: torch.Tensor, dphi_hat: torch.Tensor, b: int, t: int, lambda_latent: float,
                     loss_scale: float, dar: torch.Tensor, out: torch.Tensor) -> None:
        """out[0] = l_lat; dar (B*T, D) 16-bit = f_AR's output gradient: dphi_hat shifted back + lambda_latent * dl_lat, * loss_scale."""
        part = torch.empty(b * t, dtype=torch.float32, device=self._device)
        _lib.check(_lib.load_library().r50_op_ar_latent_grad(ar.data_ptr(), phi.data_ptr(), dphi_hat.data_ptr(), b, t, self.latent_dim,
                                                              lambda_latent, loss_scale, dar.data_ptr(), out.data_ptr(), part.data_ptr(),
                                                              self._et, self._stream()), None, "r50_op_ar_latent_grad")

    def _shift_into(self, ar: torch.Tensor, dst: torch.Tensor, b: int, t: int) -> None:
        """dst = phi_hat: dst[:, 1:] = ar[:, :-1], dst[:, 0] = 0 (src/model.py:165-166)."""
        d = self.latent_dim
        v = dst.view(b, t, d)
        v[:, 0, :].zero_()
        v[:, 1:, :] = ar.view(b, t, d)[:, :-1, :]

    def forward_backward(self, feats: torch.Tensor, joints3d: torch.Tensor, loss_scale: float = 1.0,
                         masks: Optional[Dict[str, torch.Tensor]] = None, joints2d: Optional[torch.Tensor] = None,
                         K: Optional[torch.Tensor] = None,
                         geo: Optional[GeoWeights] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The joint forward (train mode when ``masks`` is given or ``self.training``; else dropout is identity), the loss
        l3d + lambda_future * l3d_hat + lambda_latent * l_lat, backward into ``flat_grad`` (UNSCALED: the 16-bit backward runs on
        loss_scale * loss, the fp32 buffer receives grad / loss_scale).  ``self._found`` is raised when a 16-bit gradient overflowed.
        Returns (joints_phi (B,T,J,3) fp32, joints_hat (B,T,J,3) fp32, losses = [l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat] fp32 device
        tensor).
        ``geo`` (with ``joints2d`` (B,T,J,2) and ``K`` (B,3,3) or (3,3)): both pose terms gain section N's geometric terms, loss =
        l3d + geo(joints_phi) + lambda_future * (l3d_hat + geo(joints_hat[:, 1:])) + lambda_latent * l_lat; two launches of
        ``r50_op_geo_pose_loss_grad`` take the place of ``r50_op_joint_pose_loss_grad`` and ``self._geo_out16`` holds their numbers."""
        b, t = self._check_batch(feats, joints3d)
        if geo is not None:
            gt2d, kmat = self._check_geo(b, t, joints2d, K)
        if masks is None and self.training:
            masks = self.make_dropout_masks(b, t)
        keep_scale = 1.0 / (1.0 - DROPOUT_P)
        lib = _lib.load_library()
        rows, d, o = b * t, self.latent_dim, self.out_dim
        rows2 = 2 * rows
        inv = 1.0 / loss_scale
        self._arena.reset()
        self._found.zero_()
        with torch.cuda.device(self._device):
            # ---------------- forward: input_proj and f_movie (phase 1's), saved; phi lands in the strip buffer's first half ----------------
            f = feats.to(torch.float32).contiguous()
            x0 = torch.empty((rows, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), rows, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None, "r50_op_cast_rows")
            strips = torch.empty((rows2, d), dtype=self._dtype, device=self._device)       # [phi ; phi_hat]
            phi, phi_hat = strips[:rows], strips[rows:]
            x = self._gemm(x0, "input_proj", relu=False)
            _, saved_movie = self._blocks_forward_saved("f_movie", self.number_blocks, x, b, t, masks, keep_scale, out_last=phi)
            # ---------------- f_AR over phi (phase 2's), saved; the shift into the second half ----------------
            ar, saved_ar = self._blocks_forward_saved("f_AR", _AR_BLOCKS, phi, b, t, masks, keep_scale)
            self._shift_into(ar, phi_hat, b, t)
            # ---------------- the regressor once over the 2*B*T stacked rows, each half its own masks ----------------
            y = self._dev["y0"].view(1, o).expand(rows2, o).contiguous()
            reg = []
            for i in range(_REG_ITERS):
                inp = torch.empty((rows2, self._dp), dtype=self._dtype, device=self._device)
                _lib.check(lib.r50_op_concat_pad(strips.data_ptr(), d, y.data_ptr(), o, rows2, inp.data_ptr(), self._dp, self._et,
                                                 self._stream()), None, "r50_op_concat_pad")
                h1 = self._gemm(inp, "mlp0", relu=True)
                if masks is not None:
                    self._mask_scale(h1[:rows], masks[f"f_3D.{i}"], keep_scale)
                    self._mask_scale(h1[rows:], masks[f"f_3D_hat.{i}"], keep_scale)
                h2 = self._gemm(h1, "mlp3", relu=True)
                dy = self._gemm(h2, "mlp5", relu=False)
                _lib.check(lib.r50_op_add_rows(y.data_ptr(), o, dy.data_ptr(), self._op, rows2, self._et, self._stream()), None, "r50_op_add_rows")
                reg.append((inp, h1, h2))
            # ---------------- both pose terms and their gradients ----------------
            gt = joints3d.to(torch.float32).contiguous()
            dyacc = torch.empty((rows2, o), dtype=torch.float32, device=self._device)
            losses = torch.empty(5, dtype=torch.float32, device=self._device)
            if geo is None:
                self._joint_pose_loss(y, gt, b, t, self.lambda_future, loss_scale, dyacc, losses)
            else:
                self._geo_out16 = self._geo_pose_loss(y, gt, gt2d, kmat, b, t, geo, self.lambda_future, loss_scale, dyacc, losses)
            # ---------------- backward: the regressor over the stacked rows, with weight gradients (phase 1's launches) ----------------
            relu1_scale = keep_scale if masks is not None else 1.0
            dstrips, _g5 = self._regressor_backward(reg, dyacc, rows2, inv, relu1_scale, weights=True)     # [dphi from f_3D(phi) ; dphi_hat]
            # ---------------- shift backward + latent loss + cast: f_AR's output gradient, in the arena ----------------
            dx = self._arena.take(rows, d)
            self._latent_loss(ar, phi, dstrips[rows:], b, t, self.lambda_latent, loss_scale, dx, losses[4:])
            # ---------------- backward: f_AR blocks, last first (phase 2's launches) ----------------
            for i in reversed(range(_AR_BLOCKS)):
                dx = self._block_backward(f"f_AR.blocks.{i}", saved_ar[i], dx, b, t, inv, keep_scale)     # + the skip connection: block 0 gives f_AR's d/dphi
            # ---------------- the gradient of phi: f_3D(phi)'s + f_AR's input gradient ----------------
            dphi = dstrips[:rows]
            _lib.check(lib.r50_op_add_rows(dphi.data_ptr(), d, dx.data_ptr(), d, rows, self._et, self._stream()), None, "r50_op_add_rows")
            dx = torch.empty((rows, d), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(dphi.data_ptr(), rows, d, dx.data_ptr(), d, self._et, self._stream()), None, "r50_op_cast_rows")
            # ---------------- backward: f_movie blocks, last first, and input_proj's dW (phase 1's launches) ----------------
            for i in reversed(range(self.number_blocks)):
                dx = self._block_backward(f"f_movie.blocks.{i}", saved_movie[i], dx, b, t, inv, keep_scale)
            self._wgrad("input_proj.w", dx, x0, inv, False, bias="input_proj.b")
            self._check_arena()                                               # every 16-bit gradient the GEMMs and the latent kernel wrote
        yv = y.view(2, b, t, self.joints_num, 3)
        return yv[0], yv[1], losses

    def train_step(self, feats: torch.Tensor, joints3d: torch.Tensor, optim: AdamW, scaler: Optional[GradScaler] = None,
                   masks: Optional[Dict[str, torch.Tensor]] = None, group=None, joints2d: Optional[torch.Tensor] = None,
                   K: Optional[torch.Tensor] = None, geo: Optional[GeoWeights] = None) -> Tuple[float, float, bool]:
        """One joint step (``TrainableHead.train_step``'s contract): forward + loss, scaled backward, inf check, AdamW over every
        parameter, scale update.  Returns (loss, mpjpe, skipped); ``last_losses`` holds loss, l3d, mpjpe, l3d_hat, mpjpe_hat and l_lat,
        and with ``geo`` also l2d, reproj_px, l_vel, l_bone, n_clamped of each half (the second under ``*_hat``)."""
        scale = scaler.get_scale() if scaler is not None else 1.0
        _, _, losses = self.forward_backward(feats, joints3d, scale, masks, joints2d, K, geo)
        found = self._finish_step(optim, scaler, group)
        l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat = losses.tolist()
        g16 = self._geo_out16.tolist() if geo is not None else None
        loss = l3d + self.lambda_future * l3d_hat + self.lambda_latent * l_lat
        self.last_losses = {"loss": loss, "l3d": l3d, "mpjpe": mpjpe, "l3d_hat": l3d_hat, "mpjpe_hat": mpjpe_hat, "l_lat": l_lat}
        if geo is not None:
            loss = self.last_losses["loss"] = g16[0][0] + self.lambda_future * g16[1][0] + self.lambda_latent * l_lat
            self.last_losses.update(geo_halves(g16))
        return loss, mpjpe, found

    def joint_losses(self, feats: torch.Tensor, gt: torch.Tensor, joints2d: Optional[torch.Tensor] = None,
                     K: Optional[torch.Tensor] = None, geo: Optional[GeoWeights] = None):
        """Eval-mode forward of one batch: ([l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat] fp32 device tensor, joints_phi (B,T,J,3) fp32).
        The launches of ``__call__(feats, predict_future=True)`` (the regressor on phi and on phi_hat separately, as evaluation has
        always run it), the pose terms by ``r50_op_joint_pose_loss_grad`` and l_lat by ``r50_op_ar_latent_grad`` (their gradients go
        to scratch).  The second half's sums are ``r50_op_future_pose_loss_grad``'s, so l3d_hat / mpjpe_hat are phase 2's numbers.
        ``geo``: the pose terms by two ``r50_op_geo_pose_loss_grad`` calls with ``dy = NULL`` instead, and a third value is returned:
        their out8 as a (2, 8) fp32 device tensor."""
        b, t = self._check_batch(feats, gt)
        if geo is not None:
            gt2d, kmat = self._check_geo(b, t, joints2d, K)
        rows, d, o = b * t, self.latent_dim, self.out_dim
        lib = _lib.load_library()
        with torch.cuda.device(self._device):
            f = feats.to(torch.float32).contiguous()
            x0 = torch.empty((rows, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), rows, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None, "r50_op_cast_rows")
            phi = self._temporal_net(self._gemm(x0, "input_proj", relu=False), b, t, "f_movie", self.number_blocks)
            ar = self._temporal_net(phi, b, t, "f_AR", _AR_BLOCKS)
            phi_hat = torch.empty_like(phi)
            self._shift_into(ar, phi_hat, b, t)
            joints_phi = self._regressor(phi, b, t)
            joints_hat = self._regressor(phi_hat, b, t)
            y = torch.cat([joints_phi.reshape(rows, o), joints_hat.reshape(rows, o)])
            gtc = gt.to(torch.float32).contiguous()
            losses = torch.empty(5, dtype=torch.float32, device=self._device)
            out16 = None
            if geo is None:
                self._joint_pose_loss(y, gtc, b, t, 1.0, 1.0, torch.empty((2 * rows, o), dtype=torch.float32, device=self._device), losses)
            else:
                out16 = self._geo_pose_loss(y, gtc, gt2d, kmat, b, t, geo, 1.0, 1.0, None, losses)
            self._latent_loss(ar, phi, torch.zeros((rows, d), dtype=torch.float32, device=self._device), b, t, 1.0, 1.0,
                              torch.empty((rows, d), dtype=self._dtype, device=self._device), losses[4:])
        return (losses, joints_phi) if geo is None else (losses, joints_phi, out16)


def geo_halves(g16) -> Dict[str, float]:
    """The geometric numbers of the two halves of a joint step by name: l2d, reproj_px, l_vel, l_bone, n_clamped of joints_phi, and the
    same under ``*_hat`` of joints_hat[:, 1:]."""
    out = {k: g16[0][GEO_KEYS.index(k)] for k in GEO_EXTRA_KEYS}
    out.update({k + "_hat": g16[1][GEO_KEYS.index(k)] for k in GEO_EXTRA_KEYS})
    return out


GEO_JOINT_KEYS = GEO_EXTRA_KEYS + tuple(k + "_hat" for k in GEO_EXTRA_KEYS)


@torch.no_grad()
def evaluate_joint(head: JointTrainableHead, store, batch_size: int,
                   geo: Optional[GeoWeights] = None) -> Tuple[float, float, float, float, float, float]:
    """The joint validation pass: (loss, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat), each the mean over batches of the per-batch mean,
    the items of ``store`` in order, ``batch_size`` at a time, the last batch kept even if short (as ``train.evaluate``).  l3d and
    mpjpe over all frames by ``r50_op_pose_metrics`` (the numbers ``train.evaluate`` reports); l3d_hat, mpjpe_hat and l_lat over
    frames s >= 1 (the numbers ``train_ar.evaluate_future`` reports); loss = l3d + lambda_future * l3d_hat + lambda_latent * l_lat
    of the means.  The sums stay on the device and are read once per pass.  The head's mode is restored; its weights are not touched.
    ``geo``: the loss is the composite of section N (each half's geometric terms at the weights of ``geo``), and
    ``head.last_eval_geo`` holds the means of ``GEO_JOINT_KEYS`` (``n_clamped*``: totals)."""
    was_training = head.training
    head.train(False)
    lib = _lib.load_library()
    dev = head._device
    try:
        with torch.cuda.device(dev):
            acc = torch.zeros(6, dtype=torch.float64, device=dev)        # [sum l3d_hat, sum mpjpe_hat, sum l_lat | l3d, mpjpe, batches]
            acc16 = torch.zeros((2, 8), dtype=torch.float64, device=dev)
            for s in range(0, len(store), batch_size):
                batch = store.get_batch(list(range(s, min(s + batch_size, len(store)))))
                gt = batch[1].to(device=dev, dtype=torch.float32).contiguous()
                if geo is None:
                    losses, joints_phi = head.joint_losses(batch[0], gt)
                else:
                    losses, joints_phi, out16 = head.joint_losses(batch[0], gt, batch[2], batch[3], geo)
                    acc16 += out16.double()
                acc[:3] += losses[2:].double()
                _lib.check(lib.r50_op_pose_metrics(joints_phi.data_ptr(), gt.data_ptr(), gt.shape[0] * gt.shape[1], head.joints_num,
                                                   acc[3:].data_ptr(), head._stream()), None, "r50_op_pose_metrics")
            l3d_hat, mpjpe_hat, l_lat, l3d, mpjpe, n = acc.tolist()
            g16 = acc16.tolist()
    finally:
        head.train(was_training)
    n = max(n, 1.0)
    l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat = l3d / n, mpjpe / n, l3d_hat / n, mpjpe_hat / n, l_lat / n
    if geo is None:
        return l3d + head.lambda_future * l3d_hat + head.lambda_latent * l_lat, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat
    means = geo_halves([[v / n for v in half] for half in g16])
    means["n_clamped"], means["n_clamped_hat"] = g16[0][7], g16[1][7]
    head.last_eval_geo = means
    return g16[0][0] / n + head.lambda_future * g16[1][0] / n + head.lambda_latent * l_lat, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat


LOSS_KEYS = ("loss", "l3d", "mpjpe", "l3d_hat", "mpjpe_hat", "l_lat")


def train_joint_epoch(head: JointTrainableHead, store, sampler, optim: AdamW, scaler: Optional[GradScaler], seed: int, epoch: int,
                      log_every: int = 500, geo: Optional[GeoWeights] = None) -> Tuple[Dict[str, float], int, int]:
    """``train.train_epoch`` for the joint step: one ``train_step`` per batch of ``sampler`` (its epoch already set), masks from
    ``make_dropout_masks`` with ``dropout_generator(seed, epoch, it)``.  Returns (the means of ``LOSS_KEYS`` over the batches,
    applied steps, skipped steps); with ``geo`` the steps run section N's composite loss and the means include ``GEO_JOINT_KEYS``
    (``n_clamped*``: totals)."""
    head.train()
    sums = {k: 0.0 for k in LOSS_KEYS + (GEO_JOINT_KEYS if geo is not None else ())}
    n_batches = skipped = 0
    for it, idx in enumerate(sampler):
        batch = store.get_batch(idx)
        feats, joints3d = batch[:2]
        masks = head.make_dropout_masks(feats.shape[0], feats.shape[1], generator=dropout_generator(seed, epoch, it, head._device))
        if geo is None:
            _, _, found = head.train_step(feats, joints3d, optim, scaler, masks=masks)
        else:
            _, _, found = head.train_step(feats, joints3d, optim, scaler, masks=masks, joints2d=batch[2], K=batch[3], geo=geo)
        for k in sums:
            sums[k] += head.last_losses[k]
        n_batches += 1
        skipped += int(found)
        if log_every > 0 and (it + 1) % log_every == 0:
            print(f"[joint] iter {it + 1:05d}/{len(sampler):05d} | loss {sums['loss'] / n_batches:.6f} | "
                  f"mpjpe {sums['mpjpe'] / n_batches:.3f} | future mpjpe {sums['mpjpe_hat'] / n_batches:.3f}")
    return {k: v if k.startswith("n_clamped") else v / max(n_batches, 1) for k, v in sums.items()}, n_batches - skipped, skipped


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    """Phase 1's flags and defaults (``train.build_parser``), ``--outdir ./runs/joint``, plus ``--init``, ``--lambda-future`` and
    ``--lambda-latent``."""
    p = argparse.ArgumentParser("Joint training: input_proj, f_movie, f_AR and f_3D under l3d + lambda_future * l3d_hat + lambda_latent * l_lat",
                                parents=[_phase1_parser()], add_help=False)
    p.set_defaults(outdir="./runs/joint")
    p.add_argument("--init", type=str, default=None,
                   help="phase-1 / phase-2 / rollout checkpoint (its 'model') or plain state dict to start from; required unless --resume "
                        "names an existing file")
    p.add_argument("--lambda-future", type=float, default=LAMBDA_FUTURE,
                   help="weight of the future-pose loss mean((joints_hat - gt)^2) over frames >= 1, >= 0 (no run has measured a good value)")
    p.add_argument("--lambda-latent", type=float, default=LAMBDA_LATENT,
                   help="weight of the latent loss mean((phi_hat - phi.detach())^2) over frames >= 1, >= 0 (no run has measured a good value)")
    p.add_argument("--weights-from", choices=("auto", "model", "ema"), default=argparse.SUPPRESS,
                   help="which weights of --init to start from: auto (default) = its EMA weights when it has them, else the raw ones")
    return p


def validate_args(p: argparse.ArgumentParser, args: argparse.Namespace) -> argparse.Namespace:
    """The joint driver's rules on parsed arguments (``p.error`` on a breach); shared with ``train_geo --stage joint``."""
    if not args.init and not (args.resume and os.path.isfile(args.resume)):
        p.error("--init is required unless --resume names an existing checkpoint")
    if not (args.lambda_future >= 0 and args.lambda_latent >= 0):          # also refuses nan
        p.error("--lambda-future and --lambda-latent must be >= 0")
    return validate_clip_ema(p, args)


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = build_parser()
    return validate_args(p, p.parse_args(argv))


def main(argv: Optional[List[str]] = None) -> float:
    """Joint training on one MI355X.  Per epoch, in ``train.main``'s order: train, evaluate, scheduler step, ``last.pt``, ``best.pt``
    when val mpjpe + mpjpe_hat improved by more than ``--early-stop-min-delta``, patience counter.  ``--resume`` loads model and
    optimizer; the head's dimensions come from the checkpoint.  Prints one JSON line per epoch.  Returns the best val
    mpjpe + mpjpe_hat."""
    return run(parse_args(argv))


def run(args: argparse.Namespace, geo_for_epoch=None) -> float:
    """``main``'s body on parsed arguments.  ``geo_for_epoch``: None, or a function epoch -> ``GeoWeights`` (``train_geo``): the epoch
    then trains and validates under section N's composite loss with those weights, and its JSON line gains the geometric numbers of
    both halves and ``lambda_2d_active``."""
    r = open_run(args, head_from_checkpoint(args, JointTrainableHead, lambda_future=args.lambda_future, lambda_latent=args.lambda_latent))

    def epoch_fn(epoch):
        geo = geo_for_epoch(epoch) if geo_for_epoch is not None else None
        tr, steps, skipped = train_joint_epoch(r.head, r.train_set, r.sampler, r.optim, r.scaler, args.seed, epoch, args.log_every, geo=geo)

        def validate():
            va = dict(zip(LOSS_KEYS, evaluate_joint(r.head, r.val_set, args.batch_size, geo=geo)))
            if geo is not None:
                va.update(r.head.last_eval_geo)
            va_score = va["mpjpe"] + va["mpjpe_hat"]
            va_fields = {f"val_{k}": v for k, v in va.items()}
            va_fields["val_mpjpe_sum"] = va_score
            return va_score, va_fields, (
                f"Val:   loss={va['loss']:.6f} | l3d={va['l3d']:.6f} | l3d_hat={va['l3d_hat']:.6f} | l_lat={va['l_lat']:.6f} | "
                f"mpjpe={va['mpjpe']:.3f} | future mpjpe={va['mpjpe_hat']:.3f}")

        va_score, va_fields, va_lines = validate_with_ema(r, validate)
        fields = {f"train_{k}": v for k, v in tr.items()}
        fields.update({"steps": steps, "skipped": skipped})
        fields.update(va_fields)
        if geo is not None:
            fields["lambda_2d_active"] = geo.lambda_2d
        fields.update(clip_fields(r))
        return va_score, fields, (
            f"Train: loss={tr['loss']:.6f} | l3d={tr['l3d']:.6f} | l3d_hat={tr['l3d_hat']:.6f} | l_lat={tr['l_lat']:.6f} | "
            f"mpjpe={tr['mpjpe']:.3f} | future mpjpe={tr['mpjpe_hat']:.3f}",) + va_lines

    return fit(r, args, ("===== Joint training (input_proj, f_movie, f_AR, f_3D) =====",
                         f"Device: {r.device} ({args.precision}) | head: latent {r.head.latent_dim}, {r.head.number_blocks} f_movie blocks",
                         f"Train clips: {len(r.train_set)} | Val clips: {len(r.val_set)}",
                         f"Batch size: {args.batch_size} | LR: {args.lr} | lambda_future: {args.lambda_future} | "
                         f"lambda_latent: {args.lambda_latent} | seed: {args.seed}",
                         "============================================================"), epoch_fn, "mpjpe + future mpjpe")


if __name__ == "__main__":
    main()
