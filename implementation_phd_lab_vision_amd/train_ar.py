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
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .model import _AR_BLOCKS, _REG_ITERS
from .train import (DROPOUT_P, AdamW, GradScaler, build_parser as _phase1_parser, dropout_generator, fit, head_from_checkpoint, open_run,
                    train_epoch, clip_fields, validate_clip_ema, validate_with_ema)
from .trainable import FlatItem, FlatTrainableHead, block_items

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


def ar_items() -> List[FlatItem]:
    """Phase 2's flat buffer: f_AR's blocks in order, each gn1, conv1, gn2, conv2."""
    return [item for i in range(_AR_BLOCKS) for item in block_items(f"f_AR.blocks.{i}")]


class ARTrainableHead(FlatTrainableHead):
    """``PHDFor3DJoints`` with f_AR trainable (phase 2) in flat fp32 / 16-bit buffers; input_proj, f_movie and f_3D frozen."""

    _frozen_transposes = ("mlp0.w", "mlp3.w", "mlp5.w")        # the frozen regressor's dX products
    _clip_rule = (2, "phase 2")

    def __init__(self, latent_dim: int = 2048, joints_num: int = 17, number_blocks: int = 3, precision: str = "fp16",
                 lambda_latent: float = LAMBDA_LATENT, hallucinator: bool = False):
        super().__init__(latent_dim, joints_num, number_blocks, precision, hallucinator)
        self.lambda_latent = float(lambda_latent)

    def _flat_items(self) -> List[FlatItem]:
        return ar_items()

    def trainable_parameter_names(self) -> List[str]:
        return ar_trainable_names()

    def _dropout_sites(self) -> List[Tuple[str, int]]:
        """One per f_AR block, after its conv1 (src/model.py:52).  f_movie and f_3D run in eval mode."""
        return [(f"f_AR.blocks.{i}", self.latent_dim) for i in range(_AR_BLOCKS)]

    # ---- launches -------------------------------------------------------------------------------
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
            ar, saved = self._blocks_forward_saved("f_AR", _AR_BLOCKS, phi, b, t, masks, keep_scale)
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
                reg.append((None, h1, h2))
            # ---------------- future-pose loss and its gradient ----------------
            gt = joints3d.to(torch.float32).contiguous()
            dyacc = torch.empty((rows, o), dtype=torch.float32, device=self._device)
            losses = torch.empty(3, dtype=torch.float32, device=self._device)
            self._pose_loss(y, gt, b, t, loss_scale, dyacc, losses)
            # ---------------- backward through the regressor: dX only (its weights are frozen) ----------------
            dphi_hat, _g5 = self._regressor_backward(reg, dyacc, rows, inv, 1.0, weights=False)
            # ---------------- shift backward + latent loss + cast: f_AR's output gradient, in the arena ----------------
            dx = self._arena.take(rows, d)
            self._latent_loss(ar, phi, dphi_hat, b, t, self.lambda_latent, loss_scale, dx, losses)
            # ---------------- backward: f_AR blocks, last first (phase 1's f_movie launches) ----------------
            for i in reversed(range(_AR_BLOCKS)):
                dx = self._block_backward(f"f_AR.blocks.{i}", saved[i], dx, b, t, inv, keep_scale)     # after block 0: d/dphi, unused (f_movie is frozen)
            self._check_arena()                                                  # every 16-bit gradient the GEMMs and the latent kernel wrote
        return y.view(b, t, self.joints_num, 3), losses

    def train_step(self, feats: torch.Tensor, joints3d: torch.Tensor, optim: AdamW, scaler: Optional[GradScaler] = None,
                   masks: Optional[Dict[str, torch.Tensor]] = None, group=None) -> Tuple[float, float, bool]:
        """One phase-2 step: forward + loss, scaled backward, inf check, AdamW over f_AR, scale update (``TrainableHead.train_step``'s
        contract).  Returns (loss, mpjpe_hat, skipped); ``last_losses`` holds loss, l3d_hat, l_lat and mpjpe_hat of the step."""
        scale = scaler.get_scale() if scaler is not None else 1.0
        _, losses = self.forward_backward(feats, joints3d, scale, masks)
        found = self._finish_step(optim, scaler, group)
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
            # ``_regressor_backward(weights=False)``'s launches, written out because they add into dseq's predicted rows, not a new buffer
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
                        dh = self._gn_bwd(dr2, h, b, n, p + ".gn2", None, inv, n - 1, acc)
                        skip = torch.zeros((n * b, d), dtype=self._dtype, device=self._device)
                        skip[(n - 1) * b:].copy_(dnew)                          # the residual reaches frame L-1 only
                    else:
                        self._wgrad(p + ".conv2.w", dx, r2, inv, acc, bias=p + ".conv2.b")
                        dr2 = self._mm(dx, self._wt[p + ".conv2.w"])
                        dh = self._gn_bwd(dr2, h, b, n, p + ".gn2", None, inv, 0, acc)
                        skip = dx
                    if m is not None:
                        self._mask_scale(dh, m, keep_scale)
                    self._wgrad(p + ".conv1.w", dh, r1, inv, acc, bias=p + ".conv1.b")
                    dr1 = self._mm(dh, self._wt[p + ".conv1.w"])
                    dx = self._gn_bwd(dr1, xin, b, n, p + ".gn1", skip, inv, 0, acc)
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
        found = self._finish_step(optim, scaler, group)
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
    p.add_argument("--weights-from", choices=("auto", "model", "ema"), default=argparse.SUPPRESS,
                   help="which weights of --init to start from: auto (default) = its EMA weights when it has them, else the raw ones")
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
    args = validate_clip_ema(p, p.parse_args(argv))
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
    """Phase 2 on one MI355X.  Per epoch, in ``train.main``'s order (``train.fit``): train, evaluate, scheduler step, ``last.pt``,
    ``best.pt`` when the validation score improved by more than ``--early-stop-min-delta``, patience counter.  The score is the
    validation future MPJPE; with ``--objective rollout`` training runs k(e) rollout steps and the score is the ``mpjpe_mean`` of
    ``forecast.evaluate_rollout`` at the full P.  ``--resume`` loads model and optimizer; the head's dimensions come from the
    checkpoint.  Prints one JSON line per epoch.  Returns the best score."""
    from .feature_store import DeviceFeatureStore

    args = parse_args(argv)
    rollout = getattr(args, "objective", "teacher") == "rollout"
    if rollout:                                # the clip length rule of forecast.evaluate_rollout, before any other work
        clip_len = int(DeviceFeatureStore(args.val, subjects=args.val_subjects, max_clips=1, device="cpu").feats.shape[1])
        if args.input_len + args.pred_len > clip_len:
            raise ValueError(f"--input-len + --pred-len = {args.input_len + args.pred_len} exceeds the stores' clip length {clip_len}")
    r = open_run(args, head_from_checkpoint(args, ARTrainableHead, lambda_latent=args.lambda_latent))
    title = "===== Phase-2 training (f_AR), rollout objective =====" if rollout else "===== Phase-2 training (f_AR) ====="
    banner = [title, f"Device: {r.device} ({args.precision}) | head: latent {r.head.latent_dim}, {r.head.number_blocks} f_movie blocks",
              f"Train clips: {len(r.train_set)} | Val clips: {len(r.val_set)}",
              f"Batch size: {args.batch_size} | LR: {args.lr} | lambda_latent: {args.lambda_latent} | seed: {args.seed}"]
    if not rollout:
        def epoch_fn(epoch):
            tr_loss, tr_mpjpe_hat, steps, skipped = train_epoch(r.head, r.train_set, r.sampler, r.optim, r.scaler, args.seed, epoch,
                                                                args.log_every)

            def validate():
                va_l3d_hat, va_mpjpe_hat, va_l_lat, va_mpjpe = evaluate_future(r.head, r.val_set, args.batch_size)
                return va_mpjpe_hat, {"val_l3d_hat": va_l3d_hat, "val_mpjpe_hat": va_mpjpe_hat, "val_l_lat": va_l_lat, "val_mpjpe": va_mpjpe}, \
                    f"Val:   l3d_hat={va_l3d_hat:.6f} | l_lat={va_l_lat:.6f} | future mpjpe={va_mpjpe_hat:.3f} | mpjpe={va_mpjpe:.3f}"

            score, va_fields, va_lines = validate_with_ema(r, validate)
            return score, {"train_loss": tr_loss, "train_mpjpe_hat": tr_mpjpe_hat, "steps": steps, "skipped": skipped, **va_fields,
                           **clip_fields(r)}, (f"Train: loss={tr_loss:.6f} | future mpjpe={tr_mpjpe_hat:.3f}",) + va_lines

        return fit(r, args, banner + ["=" * len(title)], epoch_fn, "future MPJPE")

    from .forecast import evaluate_rollout
    i_len, p_len, c = args.input_len, args.pred_len, args.curriculum_steps

    def rollout_epoch_fn(epoch):
        k = curriculum_k(epoch, p_len, c)
        tr_loss, tr_mpjpe, steps, skipped, tr = train_rollout_epoch(r.head, r.train_set, r.sampler, r.optim, r.scaler, args.seed, epoch,
                                                                    i_len, k, args.log_every)

        def validate():
            va = evaluate_rollout(r.head, r.val_set, i_len, p_len, args.batch_size)
            va_mean = va["mpjpe_mean"]
            return va_mean, {"val_mpjpe_1": va["mpjpe"][0], "val_mpjpe_10": va["mpjpe"][min(10, p_len) - 1],
                             f"val_mpjpe_{p_len}": va["mpjpe"][-1], "val_mpjpe_mean": va_mean}, \
                (f"Val:   rollout mpjpe @1={va['mpjpe'][0]:.3f} | @{min(10, p_len)}={va['mpjpe'][min(10, p_len) - 1]:.3f} | "
                 f"@{p_len}={va['mpjpe'][-1]:.3f} | mean={va_mean:.3f}")

        score, va_fields, va_lines = validate_with_ema(r, validate)
        return score, {"k": k, "train_loss": tr_loss, "train_l3d": tr["l3d"], "train_l_lat": tr["l_lat"], "train_mpjpe": tr_mpjpe,
                       "steps": steps, "skipped": skipped, **va_fields, **clip_fields(r)}, \
            (f"Train: loss={tr_loss:.6f} | l3d={tr['l3d']:.6f} | l_lat={tr['l_lat']:.6f} | mpjpe={tr_mpjpe:.3f}",) + va_lines

    return fit(r, args, banner + [f"Input len: {i_len} | pred len: {p_len} | curriculum steps: {c}", "=" * len(title)], rollout_epoch_fn,
               "rollout MPJPE", epoch_note=lambda epoch: f" (k = {curriculum_k(epoch, p_len, c)})")


if __name__ == "__main__":
    main()
