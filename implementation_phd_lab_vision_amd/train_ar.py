"""Phase 2: training the autoregressive predictor f_AR of the lifting head on one MI355X (DESIGN.md "f next #2", INTEGRATION.md
section I).  ``python -m implementation_phd_lab_vision_amd.train_ar``.

The reference stops at phase 1: it freezes f_AR and never runs it (src/train.py:375-376), while its model computes ``phi_hat`` /
``joints_hat`` for a later phase (src/model.py:158-166).  This project defines phase 2 as the following program, written in the
reference's idiom (tests/golden/make_golden_train_ar.py runs it on the reference module itself)::

    model = PHD(latent_dim, 17, number_blocks)                  # weights: a phase-1 checkpoint's "model"
    for p in model.parameters(): p.requires_grad = False
    for p in model.f_AR.parameters(): p.requires_grad = True
    optim = torch.optim.AdamW(f_AR parameters, lr=args.lr, weight_decay=1e-2); scaler = torch.amp.GradScaler("cuda")
    model.train(); model.f_movie.eval(); model.f_3D.eval()
    with torch.autocast("cuda", dtype=torch.float16):
        phi, phi_hat, _joints_phi, joints_hat = model(feats, predict_future=True)
        l3d_hat = (joints_hat[:, 1:] - joints3d[:, 1:]).pow(2).mean()
        l_lat   = (phi_hat[:, 1:] - phi[:, 1:].detach()).pow(2).mean()
        loss    = l3d_hat + args.lambda_latent * l_lat
    scaler.scale(loss).backward(); scaler.step(optim); scaler.update()

Two choices are this project's, not the paper's: the frozen modules run in eval mode (the teacher ``phi`` is the one evaluation
sees, f_3D is a fixed decoder; only f_AR's dropout is active), and frame 0 is excluded from both terms (its ``phi_hat`` is the
constant 0, it carries no gradient).  ``--lambda-latent`` defaults to 1.0; no run has measured a good value.

``ARTrainableHead`` keeps f_AR's 24 parameters in flat fp32 master / 16-bit / gradient buffers (as ``train.TrainableHead`` does for
the phase-1 set); everything else stays as ``PHDFor3DJoints`` uploaded it.  One step, eager launches through the C ABI: input_proj
and f_movie forward (nothing saved), f_AR forward (saved, dropout masks after each block's conv1), the ``phi_hat`` shift, the
regressor on ``phi_hat``; ``r50_op_future_pose_loss_grad``; the regressor's backward for dX only; ``r50_op_ar_latent_grad`` (shift
backward + latent-loss gradient + cast into the step's 16-bit arena); f_AR's backward with weight gradients (the launches of
phase 1's f_movie backward); one overflow check over the arena; then ``all_reduce_gradients``, ``check_finite``, ``train.AdamW``,
``train.GradScaler``.  ``joints_phi`` is not computed in the step: it does not enter the loss.  No CPU fallback.

``--objective rollout`` trains f_AR on its own multi-step rollouts instead.  The reference names the step
(src/config.py ``CURRICULUM_STEPS = 25``) but never uses it; this project's definition
(tests/golden/make_golden_train_rollout.py runs it on the reference module itself)::

    # model: PHD(latent_dim, 17, number_blocks) from a phase-1 or phase-2 checkpoint; only f_AR trains
    model.train(); model.f_movie.eval(); model.f_3D.eval()              # as phase 2: only f_AR's dropout is active
    with torch.autocast("cuda", dtype=torch.float16):
        with torch.no_grad():
            phi_obs = model.f_movie(model.input_proj(feats[:, :I]))      # observed strips only (as rollout(): no future leak)
            phi_all = model.f_movie(model.input_proj(feats))             # latent teacher = phase 2's teacher
        seq = phi_obs
        for _ in range(k):                                               # k = curriculum steps this epoch, 1 <= k <= P
            seq = torch.cat([seq, model.f_AR(seq)[:, -1:]], dim=1)       # f_AR recomputed over the whole sequence, dropout each call
        fut = seq[:, I:]                                                 # (B, k, D)
        l3d  = (model.f_3D(fut) - joints3d[:, I:I + k]).pow(2).mean()
        l_lat = (fut - phi_all[:, I:I + k]).pow(2).mean()
        loss = l3d + args.lambda_latent * l_lat
    scaler.scale(loss).backward(); scaler.step(optim); scaler.update()

Full backpropagation through time: the gradient flows through every appended strip into all later steps, no truncation, no
detach.  Curriculum: in epoch e (0-based) k(e) = min(P, 1 + (e * P) // C), C = ``--curriculum-steps`` (C = 0: k = P throughout);
on ``--resume`` k follows the epoch number.  Validation is ``forecast.evaluate_rollout`` at the full P, and ``best.pt`` / early
stopping follow its ``mpjpe_mean``.  ``ARTrainableHead.rollout_train_step`` runs ``rollout``'s launches on its time-major sequence
buffer, keeping each (step, block)'s activations, then walks the steps last first: ``r50_op_rollout_pose_loss_grad`` and
``r50_op_rollout_latent_grad`` put the loss gradients into an fp32 time-major buffer, and each step's strip gradient, cast to 16 bits,
runs back through f_AR with ``r50_op_gn_relu_causal3_tm_bwd`` (t0 = L-1 for the last block's conv2, which only the new frame needs).
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .model import _AR_BLOCKS, _GN_EPS, _GROUPS, _REG_HIDDEN, _REG_ITERS, PHDFor3DJoints
from .train import (DROPOUT_P, AdamW, CosineLR, GradScaler, _Arena, _BackwardLaunches, all_reduce_gradients, build_parser as _phase1_parser,
                    dropout_generator, save_checkpoint, load_checkpoint, sync_overflow_flag, train_epoch)

LAMBDA_LATENT = 1.0
INPUT_LEN = 15             # src/config.py
PRED_LEN = 25
CURRICULUM_STEPS = 25      # src/config.py: "Slowly increase autoregressive steps from 1 to 25"


def ar_trainable_names() -> List[str]:
    """``[n for n, p in model.named_parameters() if p.requires_grad]`` with only f_AR trainable: its blocks in order, a
    ResidualBlock registering gn1, conv1, gn2, conv2 (src/model.py:39-44).  This is the numbering of the optimizer's state."""
    names: List[str] = []
    for i in range(_AR_BLOCKS):
        for m in ("gn1", "conv1.conv", "gn2", "conv2.conv"):
            names += [f"f_AR.blocks.{i}.{m}.weight", f"f_AR.blocks.{i}.{m}.bias"]
    return names


class ARTrainableHead(_BackwardLaunches, PHDFor3DJoints):
    """``PHDFor3DJoints`` with f_AR trainable (phase 2) in flat fp32 / 16-bit buffers; input_proj, f_movie and f_3D frozen."""

    def __init__(self, latent_dim: int = 2048, joints_num: int = 17, number_blocks: int = 3, precision: str = "fp16",
                 lambda_latent: float = LAMBDA_LATENT):
        super().__init__(latent_dim, joints_num, number_blocks, precision)
        self.lambda_latent = float(lambda_latent)
        self.flat_master: Optional[torch.Tensor] = None
        self._layout: List[Tuple[str, int, Tuple[int, ...]]] = []
        self.last_losses: Dict[str, float] = {}

    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    # ---- flat parameter buffers (GEMM layout) -------------------------------------------------
    def _upload(self) -> None:
        super()._upload()                      # every weight eval() needs; the f_AR entries are re-pointed into the flat buffers below
        sd, dev, d = self._sd, self._device, self.latent_dim
        items: List[Tuple[str, torch.Tensor]] = []
        for i in range(_AR_BLOCKS):
            p = f"f_AR.blocks.{i}"
            for gn, cv in (("gn1", "conv1"), ("gn2", "conv2")):
                items += [(f"{p}.{gn}.g", sd[f"{p}.{gn}.weight"]), (f"{p}.{gn}.b", sd[f"{p}.{gn}.bias"]),
                          (f"{p}.{cv}.w", sd[f"{p}.{cv}.conv.weight"].permute(0, 2, 1).reshape(d, 3 * d)),
                          (f"{p}.{cv}.b", sd[f"{p}.{cv}.conv.bias"])]
        self._layout, off = [], 0
        for name, t in items:
            assert t.numel() % 64 == 0
            self._layout.append((name, off, tuple(t.shape)))
            off += t.numel()
        self.flat_master = torch.cat([t.reshape(-1).to(torch.float32) for _, t in items]).to(dev)
        self.flat_w16 = self.flat_master.to(self._dtype)
        self.flat_grad = torch.zeros_like(self.flat_master)
        self._off = {name: (o_, shape) for name, o_, shape in self._layout}
        for name, o_, shape in self._layout:       # weights: the 16-bit copy; biases and GroupNorm parameters: the fp32 master itself
            n = int(torch.Size(shape).numel())
            src = self.flat_w16 if name.endswith(".w") else self.flat_master
            self._dev[name] = src[o_: o_ + n].view(shape)
        self._wt: Dict[str, torch.Tensor] = {}     # transposed 16-bit weights for the dX products
        lib = _lib.load_library()
        for name in ("mlp0.w", "mlp3.w", "mlp5.w"):   # the frozen regressor's, once
            n, k = self._dev[name].shape
            self._wt[name] = torch.empty((k, n), dtype=self._dtype, device=dev)
            _lib.check(lib.r50_op_transpose16(self._dev[name].data_ptr(), n, k, self._wt[name].data_ptr(), n, self._stream()), None,
                       "r50_op_transpose16")
        self._refresh_transposes()
        self._zero_bias = torch.zeros(max(3 * d, 2048, self._dp, _REG_HIDDEN), dtype=torch.float32, device=dev)
        self._found = torch.zeros(1, dtype=torch.int32, device=dev)
        self._arena = _Arena(dev, self._dtype)

    def _refresh_transposes(self) -> None:
        lib = _lib.load_library()
        for name, _, shape in self._layout:
            if not name.endswith(".w"):
                continue
            n, k = shape
            if name not in self._wt:
                self._wt[name] = torch.zeros((k, n), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_transpose16(self._dev[name].data_ptr(), n, k, self._wt[name].data_ptr(), n, self._stream()), None,
                       "r50_op_transpose16")

    def trainable_parameter_names(self) -> List[str]:
        return ar_trainable_names()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's keys and layouts (fp32, CPU): f_AR from the flat master buffer, every other entry as loaded."""
        out = {k: v.clone() for k, v in self._sd.items()}
        out.update(self.flat_to_reference(self.flat_master))
        return out

    def named_gradients(self) -> Dict[str, torch.Tensor]:
        """flat_grad under the reference's names and layouts (fp32, CPU): what ``p.grad`` of the f_AR parameters holds."""
        return self.flat_to_reference(self.flat_grad)

    def flat_to_reference(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """A buffer in the flat layout (master, gradient, AdamW moments) under the reference's f_AR names and layouts (fp32, CPU)."""
        d = self.latent_dim

        def g(name):
            o_, shape = self._off[name]
            return flat[o_: o_ + int(torch.Size(shape).numel())].view(shape).cpu()
        out = {}
        for i in range(_AR_BLOCKS):
            p = f"f_AR.blocks.{i}"
            for gn, cv in (("gn1", "conv1"), ("gn2", "conv2")):
                out[f"{p}.{gn}.weight"], out[f"{p}.{gn}.bias"] = g(f"{p}.{gn}.g"), g(f"{p}.{gn}.b")
                out[f"{p}.{cv}.conv.weight"] = g(f"{p}.{cv}.w").view(d, 3, d).permute(0, 2, 1).contiguous()
                out[f"{p}.{cv}.conv.bias"] = g(f"{p}.{cv}.b")
        return out

    def flat_from_reference(self, named: Dict[str, torch.Tensor]) -> torch.Tensor:
        """Inverse of ``flat_to_reference``: a new device buffer in the flat layout."""
        d = self.latent_dim
        flat = torch.zeros_like(self.flat_master)

        def put(name, key, view=lambda v: v):
            o_, shape = self._off[name]
            dst = view(flat[o_: o_ + int(torch.Size(shape).numel())].view(shape))
            t = named[key].detach().to(torch.float32)
            if tuple(t.shape) != tuple(dst.shape):
                raise ValueError(f"{key}: shape {tuple(t.shape)}, expected {tuple(dst.shape)}")
            dst.copy_(t)

        for i in range(_AR_BLOCKS):
            p = f"f_AR.blocks.{i}"
            for gn, cv in (("gn1", "conv1"), ("gn2", "conv2")):
                put(f"{p}.{gn}.g", f"{p}.{gn}.weight"); put(f"{p}.{gn}.b", f"{p}.{gn}.bias")
                put(f"{p}.{cv}.w", f"{p}.{cv}.conv.weight", lambda v: v.view(d, 3, d).permute(0, 2, 1))
                put(f"{p}.{cv}.b", f"{p}.{cv}.conv.bias")
        return flat

    def refresh_weights16(self) -> None:
        """The 16-bit weights and their transposes from ``flat_master`` (after its values were replaced from outside)."""
        self.flat_w16.copy_(self.flat_master.to(self._dtype))
        self._refresh_transposes()

    def make_dropout_masks(self, b: int, t: int, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """Byte keep-masks (1 = keep, probability 1 - p) for the dropout sites of one phase-2 step: one per f_AR block, after its
        conv1 (src/model.py:52).  f_movie and f_3D run in eval mode."""
        return {f"f_AR.blocks.{i}": (torch.rand(b * t, self.latent_dim, device=self._device, generator=generator) >= DROPOUT_P)
                .to(torch.uint8) for i in range(_AR_BLOCKS)}

    # ---- launches -------------------------------------------------------------------------------
    def _check_batch(self, feats: torch.Tensor, joints3d: torch.Tensor) -> Tuple[int, int]:
        if self.flat_master is None:
            raise _lib.R50Error("call .load_state_dict(...) and .to('cuda:N') first")
        if feats.dim() != 3 or feats.shape[-1] != 2048 or feats.device != self._device:
            raise ValueError("feats: expected (B,T,2048) on the head's device")
        b, t, _ = feats.shape
        if tuple(joints3d.shape) != (b, t, self.joints_num, 3) or joints3d.device != self._device:
            raise ValueError("joints3d: expected (B,T,J,3) on the head's device")
        if b < 1 or t < 2:
            raise ValueError("phase 2 needs clips of at least 2 frames (frame 0 has no prediction)")
        return b, t

    def _phi(self, feats: torch.Tensor, b: int, t: int) -> torch.Tensor:
        """input_proj + f_movie, nothing saved: the teacher phi (B*T, D) 16-bit."""
        lib = _lib.load_library()
        f = feats.to(torch.float32).contiguous()
        x0 = torch.empty((b * t, 2048), dtype=self._dtype, device=self._device)
        _lib.check(lib.r50_op_cast_rows(f.data_ptr(), b * t, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None, "r50_op_cast_rows")
        return self._temporal_net(self._gemm(x0, "input_proj", relu=False), b, t, "f_movie", self.number_blocks)

    def _shift(self, ar: torch.Tensor, b: int, t: int) -> torch.Tensor:
        """phi_hat[:, 1:] = ar[:, :-1], phi_hat[:, 0] = 0 (src/model.py:159-160)."""
        d = self.latent_dim
        phi_hat = torch.zeros((b * t, d), dtype=self._dtype, device=self._device)
        phi_hat.view(b, t, d)[:, 1:, :] = ar.view(b, t, d)[:, :-1, :]
        return phi_hat

    def _pose_loss(self, y: torch.Tensor, gt: torch.Tensor, b: int, t: int, loss_scale: float, dy: torch.Tensor, out: torch.Tensor) -> None:
        """out[0:2] = [l3d_hat, mpjpe_hat] over frames s >= 1; dy (B*T, J*3) fp32 = their gradient * loss_scale (0 on frame 0)."""
        _lib.check(_lib.load_library().r50_op_future_pose_loss_grad(y.data_ptr(), gt.data_ptr(), b, t, self.joints_num, loss_scale,
                                                                     dy.data_ptr(), out.data_ptr(), self._stream()), None,
                   "r50_op_future_pose_loss_grad")

    def _latent_loss(self, ar: torch.Tensor, phi: torch.Tensor, dphi_hat: torch.Tensor, b: int, t: int, lambda_latent: float,
                     loss_scale: float, dar: torch.Tensor, out: torch.Tensor) -> None:
        """out[2] = l_lat; dar (B*T, D) 16-bit = f_AR's output gradient: dphi_hat shifted back + lambda_latent * dl_lat, * loss_scale."""
        part = torch.empty(b * t, dtype=torch.float32, device=self._device)
        _lib.check(_lib.load_library().r50_op_ar_latent_grad(ar.data_ptr(), phi.data_ptr(), dphi_hat.data_ptr(), b, t, self.latent_dim,
                                                              lambda_latent, loss_scale, dar.data_ptr(), out[2:].data_ptr(), part.data_ptr(),
                                                              self._et, self._stream()), None, "r50_op_ar_latent_grad")

    def forward_backward(self, feats: torch.Tensor, joints3d: torch.Tensor, loss_scale: float = 1.0,
                         masks: Optional[Dict[str, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The phase-2 forward (f_AR in train mode when ``masks`` is given or ``self.training``; else dropout is identity), the loss
        l3d_hat + lambda_latent * l_lat, backward into ``flat_grad`` (UNSCALED: the 16-bit backward runs on loss_scale * loss, the fp32
        buffer receives grad / loss_scale).  ``self._found`` is raised when a 16-bit gradient overflowed.
        Returns (joints_hat (B,T,J,3) fp32, losses = [l3d_hat, mpjpe_hat, l_lat] fp32 device tensor)."""
        b, t = self._check_batch(feats, joints3d)
        if masks is None and self.training:
            masks = self.make_dropout_masks(b, t)
        keep_scale = 1.0 / (1.0 - DROPOUT_P)
        lib = _lib.load_library()
        rows, d, o = b * t, self.latent_dim, self.out_dim
        inv = 1.0 / loss_scale
        self._arena.reset()
        self._found.zero_()
        with torch.cuda.device(self._device):
            # ---------------- forward: phi (frozen, nothing saved), then f_AR keeping what its backward needs ----------------
            phi = self._phi(feats, b, t)
            x, saved = phi, []
            for i in range(_AR_BLOCKS):
                p = f"f_AR.blocks.{i}"
                r1 = self._gn_relu_rows(x, b, t, p + ".gn1")
                h = self._gemm(r1, p + ".conv1", relu=False)
                m = masks[p] if masks is not None else None
                if m is not None:
                    self._mask_scale(h, m, keep_scale)
                r2 = self._gn_relu_rows(h, b, t, p + ".gn2")
                xo = self._gemm(r2, p + ".conv2", relu=False, residual=x)
                saved.append((x, r1, h, r2, m))
                x = xo
            ar = x
            phi_hat = self._shift(ar, b, t)
            # ---------------- the frozen regressor on phi_hat (eval mode: no dropout) ----------------
            y = self._dev["y0"].view(1, o).expand(rows, o).contiguous()
            reg = []
            for _ in range(_REG_ITERS):
                inp = torch.empty((rows, self._dp), dtype=self._dtype, device=self._device)
                _lib.check(lib.r50_op_concat_pad(phi_hat.data_ptr(), d, y.data_ptr(), o, rows, inp.data_ptr(), self._dp, self._et,
                                                 self._stream()), None, "r50_op_concat_pad")
                h1 = self._gemm(inp, "mlp0", relu=True)
                h2 = self._gemm(h1, "mlp3", relu=True)
                dy = self._gemm(h2, "mlp5", relu=False)
                _lib.check(lib.r50_op_add_rows(y.data_ptr(), o, dy.data_ptr(), self._op, rows, self._et, self._stream()), None, "r50_op_add_rows")
                reg.append((h1, h2))
            # ---------------- future-pose loss and its gradient ----------------
            gt = joints3d.to(torch.float32).contiguous()
            dyacc = torch.empty((rows, o), dtype=torch.float32, device=self._device)
            losses = torch.empty(3, dtype=torch.float32, device=self._device)
            self._pose_loss(y, gt, b, t, loss_scale, dyacc, losses)
            # ---------------- backward through the regressor: dX only (its weights are frozen) ----------------
            dphi_hat = torch.zeros((rows, d), dtype=torch.float32, device=self._device)
            g5 = torch.empty((rows, self._op), dtype=self._dtype, device=self._device)
            for i in reversed(range(_REG_ITERS)):
                h1, h2 = reg[i]
                _lib.check(lib.r50_op_cast_rows(dyacc.data_ptr(), rows, o, g5.data_ptr(), self._op, self._et, self._stream()), None, "r50_op_cast_rows")
                dh2 = self._mm(g5, self._wt["mlp5.w"])                         # (rows, H)
                self._relu_bwd(dh2, h2, 1.0)
                dh1 = self._mm(dh2, self._wt["mlp3.w"])
                self._relu_bwd(dh1, h1, 1.0)
                dinp = self._mm(dh1, self._wt["mlp0.w"])                       # (rows, Dp) = [dphi_hat | dy | 0]
                _lib.check(lib.r50_op_add_rows(dphi_hat.data_ptr(), d, dinp.data_ptr(), self._dp, rows, self._et, self._stream()), None,
                           "r50_op_add_rows")
                if i > 0:
                    _lib.check(lib.r50_op_add_rows(dyacc.data_ptr(), o, dinp.data_ptr() + 2 * d, self._dp, rows, self._et, self._stream()),
                               None, "r50_op_add_rows")
            # ---------------- shift backward + latent loss + cast: f_AR's output gradient, in the arena ----------------
            dx = self._arena.take(rows, d)
            self._latent_loss(ar, phi, dphi_hat, b, t, self.lambda_latent, loss_scale, dx, losses)
            # ---------------- backward: f_AR blocks, last first (phase 1's f_movie launches) ----------------
            for i in reversed(range(_AR_BLOCKS)):
                p = f"f_AR.blocks.{i}"
                xin, r1, h, r2, m = saved[i]
                self._wgrad(p + ".conv2.w", dx, r2, inv, False, bias=p + ".conv2.b")
                dr2 = self._mm(dx, self._wt[p + ".conv2.w"])                   # (rows, 3D)
                dh = self._gn_bwd(dr2, h, b, t, p + ".gn2", None, inv)
                if m is not None:
                    self._mask_scale(dh, m, keep_scale)
                self._wgrad(p + ".conv1.w", dh, r1, inv, False, bias=p + ".conv1.b")
                dr1 = self._mm(dh, self._wt[p + ".conv1.w"])
                dx = self._gn_bwd(dr1, xin, b, t, p + ".gn1", dx, inv)         # + the skip connection's gradient (unused after block 0)
            for chunk, used in zip(self._arena.chunks, self._arena.used):     # every 16-bit gradient the GEMMs and the latent kernel wrote
                if used:
                    _lib.check(lib.r50_op_check_overflow16(chunk.data_ptr(), used, self._found.data_ptr(), self._et, self._stream()), None,
                               "r50_op_check_overflow16")
        return y.view(b, t, self.joints_num, 3), losses

    def train_step(self, feats: torch.Tensor, joints3d: torch.Tensor, optim: AdamW, scaler: Optional[GradScaler] = None,
                   masks: Optional[Dict[str, torch.Tensor]] = None, group=None) -> Tuple[float, float, bool]:
        """One phase-2 step: forward + loss, scaled backward, inf check, AdamW over f_AR, scale update (``TrainableHead.train_step``'s
        contract).  Returns (loss, mpjpe_hat, skipped); ``last_losses`` holds loss, l3d_hat, l_lat and mpjpe_hat of the step."""
        scale = scaler.get_scale() if scaler is not None else 1.0
        _, losses = self.forward_backward(feats, joints3d, scale, masks)
        lib = _lib.load_library()
        with torch.cuda.device(self._device):
            all_reduce_gradients(self.flat_grad, group)
            _lib.check(lib.r50_op_check_finite(self.flat_grad.data_ptr(), self.flat_grad.numel(), self._found.data_ptr(), self._stream()), None,
                       "r50_op_check_finite")
            sync_overflow_flag(self._found, group)
            found = bool(self._found.item())
            if not found:
                optim.step(self._found)
                self._refresh_transposes()
            if scaler is not None:
                scaler.update(found)
            l3d_hat, mpjpe_hat, l_lat = losses.tolist()
        loss = l3d_hat + self.lambda_latent * l_lat
        self.last_losses = {"loss": loss, "l3d_hat": l3d_hat, "l_lat": l_lat, "mpjpe_hat": mpjpe_hat}
        return loss, mpjpe_hat, found

    # ---- the rollout objective -------------------------------------------------------------------
    def make_rollout_dropout_masks(self, b: int, input_len: int, k: int,
                                   generator: Optional[torch.Generator] = None) -> List[Dict[str, torch.Tensor]]:
        """Byte keep-masks of one rollout step: masks[j]["f_AR.blocks.i"] ((I+j)*B, D), time-major like the sequence, after block i's
        conv1 at rollout step j; drawn in (step, block) order."""
        return [{f"f_AR.blocks.{i}": (torch.rand((input_len + j) * b, self.latent_dim, device=self._device, generator=generator)
                                      >= DROPOUT_P).to(torch.uint8) for i in range(_AR_BLOCKS)} for j in range(k)]

    def _gn_bwd_tm(self, dr: torch.Tensor, x: torch.Tensor, b: int, t: int, t0: int, prefix: str, add: Optional[torch.Tensor],
                   inv_scale: float, accumulate: bool) -> torch.Tensor:
        """``r50_op_gn_relu_causal3_tm_bwd``: dx (t*b, D) time-major; the GroupNorm parameter gradients [+]= into flat_grad."""
        d = self.latent_dim
        lib = _lib.load_library()
        dx = torch.empty((b * t, d), dtype=self._dtype, device=self._device)
        part = torch.empty((2, b, d), dtype=torch.float32, device=self._device)
        _lib.check(lib.r50_op_gn_relu_causal3_tm_bwd(dr.data_ptr(), x.data_ptr(), b, t, t0, d, _GROUPS, self._dev[prefix + ".g"].data_ptr(),
                                                     self._dev[prefix + ".b"].data_ptr(), _GN_EPS, add.data_ptr() if add is not None else None,
                                                     dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), self._et, self._stream()), None,
                   "r50_op_gn_relu_causal3_tm_bwd")
        for j, suffix in ((0, ".g"), (1, ".b")):
            _lib.check(lib.r50_op_colsum_f32(part[j].data_ptr(), b, d, inv_scale, self.grad_view(prefix + suffix).data_ptr(),
                                             int(accumulate), self._stream()), None, "r50_op_colsum_f32")
        return dx

    def _check_arena(self) -> None:
        lib = _lib.load_library()
        for chunk, used in zip(self._arena.chunks, self._arena.used):
            if used:
                _lib.check(lib.r50_op_check_overflow16(chunk.data_ptr(), used, self._found.data_ptr(), self._et, self._stream()), None,
                           "r50_op_check_overflow16")

    def rollout_forward_backward(self, feats: torch.Tensor, joints3d: torch.Tensor, input_len: int, k: int, loss_scale: float = 1.0,
                                 masks: Optional[List[Dict[str, torch.Tensor]]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The rollout objective's forward (f_AR in train mode when ``masks`` is given or ``self.training``; else dropout is identity),
        loss l3d + lambda_latent * l_lat over the k rolled-out frames, and full backpropagation through time into ``flat_grad``
        (UNSCALED, as ``forward_backward``).  ``self._found`` is raised when a 16-bit gradient overflowed.
        Returns (future joints (B,k,J,3) fp32, losses = [l3d, mpjpe, l_lat] fp32 device tensor).

        The sequence is ``rollout``'s time-major buffer of (I+k)*B rows and the forward issues ``rollout``'s launches, keeping each
        (step, block)'s input, GroupNorm rows, conv1 output and mask.  The backward walks the steps last first: the gradient of the
        strip step j appended (fp32 rows of ``dseq``, which every later step has already added into) is cast to 16 bits, runs back
        through the last block (conv2 over B rows, GroupNorm with t0 = L-1, the skip connection onto frame L-1 only) and the two
        blocks before it, and what reaches the sequence is added into ``dseq``'s predicted rows (the observed ones feed frozen
        f_movie only).  The 16-bit arena is checked for overflow and reused once per step."""
        b, t = self._check_batch(feats, joints3d)
        i_len, k = int(input_len), int(k)
        if i_len < 1 or k < 1 or i_len + k > t:
            raise ValueError(f"rollout training needs 1 <= input_len, 1 <= k and input_len + k <= T (got {i_len}, {k}, T={t})")
        if masks is None and self.training:
            masks = self.make_rollout_dropout_masks(b, i_len, k)
        if masks is not None and len(masks) != k:
            raise ValueError(f"expected {k} per-step dropout mask sets, got {len(masks)}")
        keep_scale = 1.0 / (1.0 - DROPOUT_P)
        lib = _lib.load_library()
        d, o = self.latent_dim, self.out_dim
        rows = k * b
        inv = 1.0 / loss_scale
        last = _AR_BLOCKS - 1
        self._arena.reset()
        self._found.zero_()
        with torch.cuda.device(self._device):
            # ---------------- forward: the observed strips, the teacher, then the rollout keeping what BPTT needs ----------------
            phi_obs = self._phi(feats[:, :i_len], b, i_len)
            phi_all = self._phi(feats, b, t)
            seq = torch.empty(((i_len + k) * b, d), dtype=self._dtype, device=self._device)
            seq[: i_len * b].view(i_len, b, d).copy_(phi_obs.view(b, i_len, d).transpose(0, 1))
            saved: List[List[tuple]] = []
            for j in range(k):
                n = i_len + j
                x, step = seq[: n * b], []
                for i in range(_AR_BLOCKS):
                    p = f"f_AR.blocks.{i}"
                    r1 = self._gn_relu_rows_tm(x, b, n, 0, p + ".gn1")
                    h = self._gemm(r1, p + ".conv1", relu=False)
                    m = masks[j][p] if masks is not None else None
                    if m is not None:
                        self._mask_scale(h, m, keep_scale)
                    if i < last:
                        r2 = self._gn_relu_rows_tm(h, b, n, 0, p + ".gn2")
                        xo = self._gemm(r2, p + ".conv2", relu=False, residual=x)
                    else:
                        r2 = self._gn_relu_rows_tm(h, b, n, n - 1, p + ".gn2")
                        xo = self._gemm(r2, p + ".conv2", relu=False, residual=x[(n - 1) * b:], out=seq[n * b: (n + 1) * b])
                    step.append((x, r1, h, r2, m))
                    x = xo
                saved.append(step)
            fut = seq[i_len * b:]                                                 # (k*B, D) time-major
            # ---------------- the frozen regressor on the predicted strips ----------------
            y = self._dev["y0"].view(1, o).expand(rows, o).contiguous()
            reg = []
            for _ in range(_REG_ITERS):
                inp = torch.empty((rows, self._dp), dtype=self._dtype, device=self._device)
                _lib.check(lib.r50_op_concat_pad(fut.data_ptr(), d, y.data_ptr(), o, rows, inp.data_ptr(), self._dp, self._et,
                                                 self._stream()), None, "r50_op_concat_pad")
                h1 = self._gemm(inp, "mlp0", relu=True)
                h2 = self._gemm(h1, "mlp3", relu=True)
                dy = self._gemm(h2, "mlp5", relu=False)
                _lib.check(lib.r50_op_add_rows(y.data_ptr(), o, dy.data_ptr(), self._op, rows, self._et, self._stream()), None, "r50_op_add_rows")
                reg.append((h1, h2))
            # ---------------- losses and their gradients into dseq (fp32, time-major) ----------------
            gt = joints3d.to(torch.float32).contiguous()
            dyacc = torch.empty((rows, o), dtype=torch.float32, device=self._device)
            losses = torch.empty(3, dtype=torch.float32, device=self._device)
            _lib.check(lib.r50_op_rollout_pose_loss_grad(y.data_ptr(), gt.data_ptr(), b, k, t, i_len, self.joints_num, loss_scale,
                                                         dyacc.data_ptr(), losses.data_ptr(), self._stream()), None,
                       "r50_op_rollout_pose_loss_grad")
            dseq = torch.zeros(((i_len + k) * b, d), dtype=torch.float32, device=self._device)
            dfut = dseq[i_len * b:]
            g5 = torch.empty((rows, self._op), dtype=self._dtype, device=self._device)
            for i in reversed(range(_REG_ITERS)):
                h1, h2 = reg[i]
                _lib.check(lib.r50_op_cast_rows(dyacc.data_ptr(), rows, o, g5.data_ptr(), self._op, self._et, self._stream()), None, "r50_op_cast_rows")
                dh2 = self._mm(g5, self._wt["mlp5.w"])
                self._relu_bwd(dh2, h2, 1.0)
                dh1 = self._mm(dh2, self._wt["mlp3.w"])
                self._relu_bwd(dh1, h1, 1.0)
                dinp = self._mm(dh1, self._wt["mlp0.w"])                       # (rows, Dp) = [dfut | dy | 0]
                _lib.check(lib.r50_op_add_rows(dfut.data_ptr(), d, dinp.data_ptr(), self._dp, rows, self._et, self._stream()), None,
                           "r50_op_add_rows")
                if i > 0:
                    _lib.check(lib.r50_op_add_rows(dyacc.data_ptr(), o, dinp.data_ptr() + 2 * d, self._dp, rows, self._et, self._stream()),
                               None, "r50_op_add_rows")
            part = torch.empty(rows, dtype=torch.float32, device=self._device)
            _lib.check(lib.r50_op_rollout_latent_grad(fut.data_ptr(), phi_all.data_ptr(), b, k, t, i_len, d, self.lambda_latent, loss_scale,
                                                      dfut.data_ptr(), losses[2:].data_ptr(), part.data_ptr(), self._et, self._stream()),
                       None, "r50_op_rollout_latent_grad")
            # ---------------- BPTT: the steps last first ----------------
            for j in reversed(range(k)):
                n = i_len + j
                acc = j < k - 1                                                # the first step processed writes the gradients
                self._check_arena()
                self._arena.reset()
                dnew = self._arena.take(b, d)                                  # the appended strip's gradient, 16-bit
                _lib.check(lib.r50_op_cast_rows(dseq[n * b:].data_ptr(), b, d, dnew.data_ptr(), d, self._et, self._stream()), None,
                           "r50_op_cast_rows")
                dx = None
                for i in reversed(range(_AR_BLOCKS)):
                    p = f"f_AR.blocks.{i}"
                    xin, r1, h, r2, m = saved[j][i]
                    if i == last:
                        self._wgrad(p + ".conv2.w", dnew, r2, inv, acc, bias=p + ".conv2.b")
                        dr2 = self._mm(dnew, self._wt[p + ".conv2.w"])         # (B, 3D)
                        dh = self._gn_bwd_tm(dr2, h, b, n, n - 1, p + ".gn2", None, inv, acc)
                        skip = torch.zeros((n * b, d), dtype=self._dtype, device=self._device)
                        skip[(n - 1) * b:].copy_(dnew)                          # the residual reaches frame L-1 only
                    else:
                        self._wgrad(p + ".conv2.w", dx, r2, inv, acc, bias=p + ".conv2.b")
                        dr2 = self._mm(dx, self._wt[p + ".conv2.w"])
                        dh = self._gn_bwd_tm(dr2, h, b, n, 0, p + ".gn2", None, inv, acc)
                        skip = dx
                    if m is not None:
                        self._mask_scale(dh, m, keep_scale)
                    self._wgrad(p + ".conv1.w", dh, r1, inv, acc, bias=p + ".conv1.b")
                    dr1 = self._mm(dh, self._wt[p + ".conv1.w"])
                    dx = self._gn_bwd_tm(dr1, xin, b, n, 0, p + ".gn1", skip, inv, acc)
                if j > 0:                                                      # rows of predicted strips; the observed ones are frozen
                    _lib.check(lib.r50_op_add_rows(dseq[i_len * b:].data_ptr(), d, dx[i_len * b:].data_ptr(), d, (n - i_len) * b, self._et,
                                                   self._stream()), None, "r50_op_add_rows")
            self._check_arena()
        return y.view(k, b, self.joints_num, 3).transpose(0, 1).contiguous(), losses

    def rollout_train_step(self, feats: torch.Tensor, joints3d: torch.Tensor, input_len: int, k: int, optim: AdamW,
                           scaler: Optional[GradScaler] = None, masks: Optional[List[Dict[str, torch.Tensor]]] = None,
                           group=None) -> Tuple[float, float, bool]:
        """One step of the rollout objective (``train_step``'s contract): forward + loss, scaled BPTT, inf check, AdamW over f_AR,
        scale update.  Returns (loss, mpjpe, skipped); ``last_losses`` holds loss, l3d, l_lat and mpjpe of the step."""
        scale = scaler.get_scale() if scaler is not None else 1.0
        _, losses = self.rollout_forward_backward(feats, joints3d, input_len, k, scale, masks)
        lib = _lib.load_library()
        with torch.cuda.device(self._device):
            all_reduce_gradients(self.flat_grad, group)
            _lib.check(lib.r50_op_check_finite(self.flat_grad.data_ptr(), self.flat_grad.numel(), self._found.data_ptr(), self._stream()), None,
                       "r50_op_check_finite")
            sync_overflow_flag(self._found, group)
            found = bool(self._found.item())
            if not found:
                optim.step(self._found)
                self._refresh_transposes()
            if scaler is not None:
                scaler.update(found)
            l3d, mpjpe, l_lat = losses.tolist()
        loss = l3d + self.lambda_latent * l_lat
        self.last_losses = {"loss": loss, "l3d": l3d, "l_lat": l_lat, "mpjpe": mpjpe}
        return loss, mpjpe, found

    def future_losses(self, feats: torch.Tensor, gt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Eval-mode forward of one batch: ([l3d_hat, mpjpe_hat, l_lat] fp32 device tensor, joints_phi (B,T,J,3) fp32).  The launches
        of ``__call__(feats, predict_future=True)``; the losses by the phase-2 loss kernels (their gradients go to scratch)."""
        b, t = self._check_batch(feats, gt)
        rows, d = b * t, self.latent_dim
        with torch.cuda.device(self._device):
            phi = self._phi(feats, b, t)
            ar = self._temporal_net(phi, b, t, "f_AR", _AR_BLOCKS)
            joints_phi = self._regressor(phi, b, t)
            joints_hat = self._regressor(self._shift(ar, b, t), b, t)
            losses = torch.empty(3, dtype=torch.float32, device=self._device)
            self._pose_loss(joints_hat, gt, b, t, 1.0, torch.empty((rows, self.out_dim), dtype=torch.float32, device=self._device), losses)
            self._latent_loss(ar, phi, torch.zeros((rows, d), dtype=torch.float32, device=self._device), b, t, 1.0, 1.0,
                              torch.empty((rows, d), dtype=self._dtype, device=self._device), losses)
        return losses, joints_phi


@torch.no_grad()
def evaluate_future(head: ARTrainableHead, store, batch_size: int) -> Tuple[float, float, float, float]:
    """The phase-2 validation pass: (l3d_hat, mpjpe_hat, l_lat, mpjpe), each the mean over batches of the per-batch mean, the items
    of ``store`` in order, ``batch_size`` at a time, the last batch kept even if short (as ``train.evaluate``).  l3d_hat and mpjpe_hat
    over frames s >= 1; mpjpe is phase 1's MPJPE of joints_phi (``r50_op_pose_metrics``, the numbers ``train.evaluate`` reports).
    The sums stay on the device and are read once per pass.  The head's mode is restored; its weights are not touched."""
    was_training = head.training
    head.train(False)
    lib = _lib.load_library()
    dev = head._device
    try:
        with torch.cuda.device(dev):
            acc = torch.zeros(6, dtype=torch.float64, device=dev)        # [sum l3d_hat, sum mpjpe_hat, sum l_lat | l3d, mpjpe, batches]
            for s in range(0, len(store), batch_size):
                batch = store.get_batch(list(range(s, min(s + batch_size, len(store)))))
                gt = batch[1].to(device=dev, dtype=torch.float32).contiguous()
                losses, joints_phi = head.future_losses(batch[0], gt)
                acc[:3] += losses.double()
                _lib.check(lib.r50_op_pose_metrics(joints_phi.data_ptr(), gt.data_ptr(), gt.shape[0] * gt.shape[1], head.joints_num,
                                                   acc[3:].data_ptr(), head._stream()), None, "r50_op_pose_metrics")
            l3d_hat, mpjpe_hat, l_lat, _, mpjpe, n = acc.tolist()
    finally:
        head.train(was_training)
    n = max(n, 1.0)
    return l3d_hat / n, mpjpe_hat / n, l_lat / n, mpjpe / n


# ---- the phase-2 driver -----------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    """Phase 1's flags and defaults (``train.build_parser``), ``--outdir ./runs/phase2``, plus ``--init`` and ``--lambda-latent``."""
    p = argparse.ArgumentParser("Phase-2 training: freeze input_proj, f_movie and f_3D, train f_AR (future 3D joints + latent strips)",
                                parents=[_phase1_parser()], add_help=False)
    p.set_defaults(outdir="./runs/phase2")
    p.add_argument("--init", type=str, default=None,
                   help="phase-1 checkpoint (its 'model') or plain state dict to start from; required unless --resume names an existing file")
    p.add_argument("--lambda-latent", type=float, default=LAMBDA_LATENT,
                   help="weight of the latent loss mean((phi_hat - phi)^2) over frames >= 1 (no run has measured a good value)")
    # The rollout objective's flags.  Their defaults are applied by parse_args only for --objective rollout,
    # so a teacher run's namespace -- and the "args" its checkpoints record -- is what it was before these flags existed.
    p.add_argument("--objective", choices=("teacher", "rollout"), default=argparse.SUPPRESS,
                   help="teacher (default): one teacher-forced step over the clip (section I); rollout: f_AR on its own k-step rollouts")
    p.add_argument("--input-len", type=int, default=argparse.SUPPRESS, help=f"rollout: observed frames I (default {INPUT_LEN})")
    p.add_argument("--pred-len", type=int, default=argparse.SUPPRESS, help=f"rollout: predicted frames P (default {PRED_LEN})")
    p.add_argument("--curriculum-steps", type=int, default=argparse.SUPPRESS,
                   help=f"rollout: epochs over which k grows from 1 to P, 0 = k = P throughout (default {CURRICULUM_STEPS})")
    return p


ROLLOUT_DEFAULTS = {"objective": "teacher", "input_len": INPUT_LEN, "pred_len": PRED_LEN, "curriculum_steps": CURRICULUM_STEPS}


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    """The driver's arguments.  With ``--objective rollout`` the namespace holds objective, input_len, pred_len and
    curriculum_steps (defaults ``ROLLOUT_DEFAULTS``); without it, none of them."""
    p = build_parser()
    args = p.parse_args(argv)
    if not args.init and not (args.resume and os.path.isfile(args.resume)):
        p.error("--init is required unless --resume names an existing checkpoint")
    if getattr(args, "objective", "teacher") == "rollout":
        for k, v in ROLLOUT_DEFAULTS.items():
            if not hasattr(args, k):
                setattr(args, k, v)
        if args.input_len < 1 or args.pred_len < 1 or args.curriculum_steps < 0:
            p.error("--input-len and --pred-len must be >= 1, --curriculum-steps >= 0")
    else:
        extra = [k for k in ("input_len", "pred_len", "curriculum_steps") if hasattr(args, k)]
        if extra:
            p.error(f"--{extra[0].replace('_', '-')} applies to --objective rollout only")
    return args


def curriculum_k(epoch: int, pred_len: int, curriculum_steps: int) -> int:
    """Rollout steps of epoch ``epoch`` (0-based): min(P, 1 + (e * P) // C), and P throughout for C = 0."""
    p, c = int(pred_len), int(curriculum_steps)
    if c <= 0:
        return p
    return min(p, 1 + (int(epoch) * p) // c)


def train_rollout_epoch(head: ARTrainableHead, store, sampler, optim: AdamW, scaler: Optional[GradScaler], seed: int, epoch: int,
                        input_len: int, k: int, log_every: int = 500) -> Tuple[float, float, int, int, Dict[str, float]]:
    """``train.train_epoch`` for the rollout objective: one ``rollout_train_step`` per batch of ``sampler`` (its epoch already set),
    masks from ``make_rollout_dropout_masks`` with ``dropout_generator(seed, epoch, it)``.  Returns (mean loss, mean mpjpe, applied
    steps, skipped steps, means of l3d / l_lat / mpjpe)."""
    head.train()
    sums = {"loss": 0.0, "l3d": 0.0, "l_lat": 0.0, "mpjpe": 0.0}
    n_batches = skipped = 0
    for it, idx in enumerate(sampler):
        feats, joints3d = store.get_batch(idx)[:2]
        masks = head.make_rollout_dropout_masks(feats.shape[0], input_len, k, generator=dropout_generator(seed, epoch, it, head._device))
        _, _, found = head.rollout_train_step(feats, joints3d, input_len, k, optim, scaler, masks=masks)
        for key in sums:
            sums[key] += head.last_losses[key]
        n_batches += 1
        skipped += int(found)
        if log_every > 0 and (it + 1) % log_every == 0:
            print(f"[AR]  iter {it + 1:05d}/{len(sampler):05d} | k {k} | loss {sums['loss'] / n_batches:.6f} | "
                  f"mpjpe {sums['mpjpe'] / n_batches:.3f}")
    means = {key: v / max(n_batches, 1) for key, v in sums.items()}
    return means["loss"], means["mpjpe"], n_batches - skipped, skipped, means


def main(argv: Optional[List[str]] = None) -> float:
    """Phase 2 on one MI355X.  Per epoch, in ``train.main``'s order: train, evaluate, scheduler step, ``last.pt``, ``best.pt`` when the
    validation future MPJPE improved by more than ``--early-stop-min-delta``, patience counter.  ``--resume`` loads model and
    optimizer; the head's dimensions come from the checkpoint.  Prints one JSON line per epoch.  Returns the best val future MPJPE."""
    from .feature_store import DeviceFeatureStore
    from .results import infer_head_dims, load_head_state
    from .samplers import MixedShardBatchSampler

    args = parse_args(argv)
    rollout = getattr(args, "objective", "teacher") == "rollout"
    if rollout:                                # the clip length rule of forecast.evaluate_rollout, before any other work
        clip_len = int(DeviceFeatureStore(args.val, subjects=args.val_subjects, max_clips=1, device="cpu").feats.shape[1])
        if args.input_len + args.pred_len > clip_len:
            raise ValueError(f"--input-len + --pred-len = {args.input_len + args.pred_len} exceeds the stores' clip length {clip_len}")
    if not torch.cuda.is_available():
        raise _lib.R50Error("the training driver runs on an MI355X only; there is no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.outdir, exist_ok=True)
    train_set = DeviceFeatureStore(args.train, subjects=args.train_subjects, augment=True, device=device)
    val_set = DeviceFeatureStore(args.val, subjects=args.val_subjects, device=device)
    sampler = MixedShardBatchSampler(train_set, batch_size=args.batch_size, shuffle=True, drop_last=True, seed=0)

    resume = bool(args.resume and os.path.isfile(args.resume))
    state = load_head_state(args.init if args.init else args.resume)
    latent_dim, joints_num, number_blocks = infer_head_dims(state)
    head = ARTrainableHead(latent_dim, joints_num, number_blocks, precision=args.precision, lambda_latent=args.lambda_latent)
    head.load_state_dict(state, strict=True)
    head.to(device)
    optim = AdamW(head, lr=args.lr, weight_decay=1e-2)
    scaler = GradScaler()
    schedule = CosineLR(args.lr, args.epochs)

    start_epoch, best_val, no_improve_epochs = 0, float("inf"), 0
    if resume:
        ckpt = load_checkpoint(args.resume, head, optim)
        schedule.load_group(ckpt["optim"])
        start_epoch = int(ckpt.get("epoch", 0)) + 1
        best_val = float(ckpt.get("best_val", best_val))
        print(f"Resumed from {args.resume} (start_epoch={start_epoch}, best_val={best_val:.4f})")

    if rollout:
        return _main_rollout(args, head, optim, scaler, schedule, train_set, val_set, sampler, start_epoch, best_val, device,
                             latent_dim, number_blocks)
    print("===== Phase-2 training (f_AR) =====")
    print(f"Device: {device} ({args.precision}) | head: latent {latent_dim}, {number_blocks} f_movie blocks")
    print(f"Train clips: {len(train_set)} | Val clips: {len(val_set)}")
    print(f"Batch size: {args.batch_size} | LR: {args.lr} | lambda_latent: {args.lambda_latent} | seed: {args.seed}")
    print("===================================")
    for epoch in range(start_epoch, args.epochs):
        sampler.set_epoch(epoch)
        optim.lr, optim.initial_lr = schedule.lr, schedule.initial_lr
        print(f"\nEpoch {epoch + 1}/{args.epochs}")
        t0 = time.time()
        epoch_lr = optim.lr
        tr_loss, tr_mpjpe_hat, steps, skipped = train_epoch(head, train_set, sampler, optim, scaler, args.seed, epoch, args.log_every)
        va_l3d_hat, va_mpjpe_hat, va_l_lat, va_mpjpe = evaluate_future(head, val_set, args.batch_size)
        schedule.step()
        optim.lr = schedule.lr
        print(f"Train: loss={tr_loss:.6f} | future mpjpe={tr_mpjpe_hat:.3f}")
        print(f"Val:   l3d_hat={va_l3d_hat:.6f} | l_lat={va_l_lat:.6f} | future mpjpe={va_mpjpe_hat:.3f} | mpjpe={va_mpjpe:.3f}")
        print(f"Epoch time: {time.time() - t0:.2f}s")
        print(json.dumps({"epoch": epoch, "lr": epoch_lr, "train_loss": tr_loss, "train_mpjpe_hat": tr_mpjpe_hat, "steps": steps,
                          "skipped": skipped, "val_l3d_hat": va_l3d_hat, "val_mpjpe_hat": va_mpjpe_hat, "val_l_lat": va_l_lat,
                          "val_mpjpe": va_mpjpe}))

        save_checkpoint(os.path.join(args.outdir, "last.pt"), head, optim, epoch, best_val, args)
        if (best_val - va_mpjpe_hat) > args.early_stop_min_delta:
            best_val = va_mpjpe_hat
            no_improve_epochs = 0
            save_checkpoint(os.path.join(args.outdir, "best.pt"), head, optim, epoch, best_val, args)
            print(f"New best val future MPJPE: {best_val:.3f} (saved best.pt)")
        else:
            no_improve_epochs += 1
            print(f"No improvement for {no_improve_epochs}/{args.early_stop_patience} epochs "
                  f"(best {best_val:.3f}, current {va_mpjpe_hat:.3f})")
        if args.early_stop_patience > 0 and no_improve_epochs >= args.early_stop_patience:
            print(f"Early stopping triggered at epoch {epoch + 1}. Best val future MPJPE: {best_val:.3f}")
            break
    print("\nDone.")
    print(f"Best val future MPJPE: {best_val:.3f}")
    return best_val


def _main_rollout(args, head, optim, scaler, schedule, train_set, val_set, sampler, start_epoch, best_val, device, latent_dim,
                  number_blocks) -> float:
    """``main``'s epoch loop for the rollout objective: training with k(e) steps, validation by ``forecast.evaluate_rollout`` at the
    full P, ``best.pt`` and early stopping on the validation rollout's mpjpe_mean."""
    from .forecast import evaluate_rollout
    i_len, p_len, c = args.input_len, args.pred_len, args.curriculum_steps
    no_improve_epochs = 0
    print("===== Phase-2 training (f_AR), rollout objective =====")
    print(f"Device: {device} ({args.precision}) | head: latent {latent_dim}, {number_blocks} f_movie blocks")
    print(f"Train clips: {len(train_set)} | Val clips: {len(val_set)}")
    print(f"Batch size: {args.batch_size} | LR: {args.lr} | lambda_latent: {args.lambda_latent} | seed: {args.seed}")
    print(f"Input len: {i_len} | pred len: {p_len} | curriculum steps: {c}")
    print("======================================================")
    for epoch in range(start_epoch, args.epochs):
        k = curriculum_k(epoch, p_len, c)
        sampler.set_epoch(epoch)
        optim.lr, optim.initial_lr = schedule.lr, schedule.initial_lr
        print(f"\nEpoch {epoch + 1}/{args.epochs} (k = {k})")
        t0 = time.time()
        epoch_lr = optim.lr
        tr_loss, tr_mpjpe, steps, skipped, tr = train_rollout_epoch(head, train_set, sampler, optim, scaler, args.seed, epoch, i_len, k,
                                                                    args.log_every)
        va = evaluate_rollout(head, val_set, i_len, p_len, args.batch_size)
        schedule.step()
        optim.lr = schedule.lr
        va_mean = va["mpjpe_mean"]
        print(f"Train: loss={tr_loss:.6f} | l3d={tr['l3d']:.6f} | l_lat={tr['l_lat']:.6f} | mpjpe={tr_mpjpe:.3f}")
        print(f"Val:   rollout mpjpe @1={va['mpjpe'][0]:.3f} | @{min(10, p_len)}={va['mpjpe'][min(10, p_len) - 1]:.3f} | "
              f"@{p_len}={va['mpjpe'][-1]:.3f} | mean={va_mean:.3f}")
        print(f"Epoch time: {time.time() - t0:.2f}s")
        print(json.dumps({"epoch": epoch, "lr": epoch_lr, "k": k, "train_loss": tr_loss, "train_l3d": tr["l3d"], "train_l_lat": tr["l_lat"],
                          "train_mpjpe": tr_mpjpe, "steps": steps, "skipped": skipped, "val_mpjpe_1": va["mpjpe"][0],
                          "val_mpjpe_10": va["mpjpe"][min(10, p_len) - 1], f"val_mpjpe_{p_len}": va["mpjpe"][-1], "val_mpjpe_mean": va_mean}))

        save_checkpoint(os.path.join(args.outdir, "last.pt"), head, optim, epoch, best_val, args)
        if (best_val - va_mean) > args.early_stop_min_delta:
            best_val = va_mean
            no_improve_epochs = 0
            save_checkpoint(os.path.join(args.outdir, "best.pt"), head, optim, epoch, best_val, args)
            print(f"New best val rollout MPJPE: {best_val:.3f} (saved best.pt)")
        else:
            no_improve_epochs += 1
            print(f"No improvement for {no_improve_epochs}/{args.early_stop_patience} epochs "
                  f"(best {best_val:.3f}, current {va_mean:.3f})")
        if args.early_stop_patience > 0 and no_improve_epochs >= args.early_stop_patience:
            print(f"Early stopping triggered at epoch {epoch + 1}. Best val rollout MPJPE: {best_val:.3f}")
            break
    print("\nDone.")
    print(f"Best val rollout MPJPE: {best_val:.3f}")
    return best_val


if __name__ == "__main__":
    main()
