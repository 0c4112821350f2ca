"""The hallucinator stage: training f_hal of the lifting head on one MI355X.
``python -m implementation_phd_lab_vision_amd.train_hal --init CKPT --train ... --val ...``.

The paper ("Predicting 3D Human Dynamics from Video") maps the representation of a SINGLE frame to the movie strip f_movie would have
produced with temporal context, so that f_3D and f_AR give a 3D pose and a forecast from one still image.  The reference never builds
that module (src/model.py has none).  This project defines it and the stage as the following program, written in the reference's
idiom (tests/hal_reference.py restates it on the oracle's modules)::

    class Hallucinator(nn.Module):                   # the paper: two fully connected layers with a skip connection
        def __init__(self, latent_dim):
            super().__init__()
            self.fc1 = nn.Linear(latent_dim, latent_dim)
            self.fc2 = nn.Linear(latent_dim, latent_dim)
        def forward(self, x):                        # x: (..., D) = input_proj(feats), one frame per row
            return x + self.fc2(F.relu(self.fc1(x)))

    model = PHD(latent_dim, 17, number_blocks)       # weights: a checkpoint's "model" (--init)
    model.f_hal = Hallucinator(latent_dim)
    for p in model.parameters(): p.requires_grad = False
    for p in model.f_hal.parameters(): p.requires_grad = True
    optim = torch.optim.AdamW(f_hal parameters, lr=args.lr, weight_decay=1e-2); scaler = torch.amp.GradScaler("cuda")
    model.eval()                                     # no dropout site is active: f_hal has none, the rest is frozen
    with torch.autocast("cuda", dtype=torch.float16):
        x   = model.input_proj(feats)                # (B,T,D)
        phi = model.f_movie(x).detach()              # the teacher: what evaluation sees
        phi_tilde = model.f_hal(x)                   # row by row, no temporal context
        l3d_tilde = (model.f_3D(phi_tilde) - joints3d).pow(2).mean()      # all frames
        l_lat     = (phi_tilde - phi).pow(2).mean()
        loss = l3d_tilde + args.lambda_latent * l_lat
    scaler.scale(loss).backward(); scaler.step(optim); scaler.update()

The choices that are this project's: the module's shape (two Linears of width D, ReLU between, the skip connection from its own
input), its input (``input_proj``'s output, the per-frame representation the head has), the two loss terms over every frame, the
frozen rest in eval mode, and a fresh f_hal drawn as ``torch.nn.Linear`` draws it on the CPU under ``torch.manual_seed(--seed)``.
``--lambda-latent`` defaults to 1.0; no run has measured a good value.

``HalTrainableHead`` keeps f_hal's four parameters in flat fp32 master / 16-bit / gradient buffers; everything else stays as
``PHDFor3DJoints`` uploaded it.  One step, eager launches through the C ABI: cast, input_proj (``x`` kept), f_movie forward (nothing
saved), f_hal's two GEMMs (``x`` and the hidden rows kept), the frozen regressor on ``phi_tilde``; ``r50_op_mse_loss_grad`` over all
frames; the regressor's backward for dX only; ``r50_op_hal_latent_grad`` (latent-loss gradient + the regressor's dX + the cast into
the step's 16-bit arena; include/r50_hal.h); f_hal's two weight gradients with one dX product and one ReLU backward between them
(nothing flows further: input_proj is frozen); one overflow check over the arena; then ``all_reduce_gradients``, the finite check or
the clip, ``train.AdamW``, ``train.GradScaler``.  No CPU fallback.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .model import _REG_ITERS, HAL_KEYS, has_hallucinator
from .train import (AdamW, GradScaler, build_parser as _phase1_parser, clip_fields, fit, open_run, train_epoch, validate_clip_ema,
                    validate_with_ema)
from .trainable import FlatItem, FlatTrainableHead

LAMBDA_LATENT = 1.0


def hal_trainable_names() -> List[str]:
    """``[n for n, p in model.named_parameters() if p.requires_grad]`` with only f_hal trainable: fc1 then fc2, weight then bias.
    This is the numbering of the optimizer's state."""
    return list(HAL_KEYS)


def hal_items() -> List[FlatItem]:
    """The stage's flat buffer: f_hal.fc1's weight and bias, then f_hal.fc2's."""
    return [(f"f_hal.{fc}.{s}", f"f_hal.{fc}.{name}", "plain") for fc in ("fc1", "fc2") for s, name in (("w", "weight"), ("b", "bias"))]


def fresh_hallucinator_state(latent_dim: int, seed: int) -> Dict[str, torch.Tensor]:
    """A new f_hal: ``torch.nn.Linear``'s default initialisation, fc1 then fc2, drawn on the CPU under ``torch.manual_seed(seed)``
    (the caller's generator state is restored)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        fc1, fc2 = torch.nn.Linear(latent_dim, latent_dim), torch.nn.Linear(latent_dim, latent_dim)
    return {"f_hal.fc1.weight": fc1.weight.detach().clone(), "f_hal.fc1.bias": fc1.bias.detach().clone(),
            "f_hal.fc2.weight": fc2.weight.detach().clone(), "f_hal.fc2.bias": fc2.bias.detach().clone()}


class HalTrainableHead(FlatTrainableHead):
    """``PHDFor3DJoints`` with f_hal trainable in flat fp32 / 16-bit buffers; input_proj, f_movie, f_AR and f_3D frozen."""

    _no_transpose = frozenset({"f_hal.fc1.w"})                 # nothing flows past fc1: input_proj is frozen
    _frozen_transposes = ("mlp0.w", "mlp3.w", "mlp5.w")        # the frozen regressor's dX products

    def __init__(self, latent_dim: int = 2048, joints_num: int = 17, number_blocks: int = 3, precision: str = "fp16",
                 lambda_latent: float = LAMBDA_LATENT, hallucinator: bool = True):
        if not hallucinator:
            raise ValueError("the hallucinator stage trains f_hal: hallucinator=False makes no sense here")
        super().__init__(latent_dim, joints_num, number_blocks, precision, True)
        self.lambda_latent = float(lambda_latent)

    def _flat_items(self) -> List[FlatItem]:
        return hal_items()

    def trainable_parameter_names(self) -> List[str]:
        return hal_trainable_names()

    def _dropout_sites(self) -> List[Tuple[str, int]]:
        """None: f_hal has no dropout and the rest runs in eval mode."""
        return []

    def _latent_loss(self, h: torch.Tensor, phi: torch.Tensor, dh_reg: torch.Tensor, rows: int, lambda_latent: float, loss_scale: float,
                     dh: torch.Tensor, out: torch.Tensor) -> None:
        """out[0] = l_lat; dh (rows, D) 16-bit = f_hal's output gradient: dh_reg + lambda_latent * dl_lat * loss_scale."""
        part = torch.empty(rows, dtype=torch.float32, device=self._device)
        _lib.check(_lib.load_library().r50_op_hal_latent_grad(h.data_ptr(), phi.data_ptr(), dh_reg.data_ptr(), rows, self.latent_dim,
                                                               lambda_latent, loss_scale, dh.data_ptr(), out.data_ptr(), part.data_ptr(),
                                                               self._et, self._stream()), None, "r50_op_hal_latent_grad")

    def forward_backward(self, feats: torch.Tensor, joints3d: torch.Tensor, loss_scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """The stage's forward, the loss l3d_tilde + lambda_latent * l_lat, backward into ``flat_grad`` (UNSCALED: the 16-bit backward
        runs on loss_scale * loss, the fp32 buffer receives grad / loss_scale).  ``self._found`` is raised when a 16-bit gradient
        overflowed.  ``self._last_dh`` is the latent kernel's output (f_hal's output gradient, in the arena) and ``self._last_dh_reg``
        the regressor's dX it read, until the next step.
        Returns (joints_tilde (B,T,J,3) fp32, losses = [l3d_tilde, mpjpe_tilde, l_lat] fp32 device tensor)."""
        b, t = self._check_batch(feats, joints3d)
        lib = _lib.load_library()
        rows, d, o = b * t, self.latent_dim, self.out_dim
        inv = 1.0 / loss_scale
        self._arena.reset()
        self._found.zero_()
        with torch.cuda.device(self._device):
            # ---------------- forward: x, the teacher phi (frozen, nothing saved), then f_hal keeping x and its hidden rows ----------------
            f = feats.to(torch.float32).contiguous()
            x0 = torch.empty((rows, 2048), dtype=self._dtype, device=self._device)
            _lib.check(lib.r50_op_cast_rows(f.data_ptr(), rows, 2048, x0.data_ptr(), 2048, self._et, self._stream()), None, "r50_op_cast_rows")
            x = self._gemm(x0, "input_proj", relu=False)
            phi = self._temporal_net(x, b, t, "f_movie", self.number_blocks)
            h1 = self._gemm(x, "f_hal.fc1", relu=True)
            phi_tilde = self._gemm(h1, "f_hal.fc2", relu=False, residual=x)
            # ---------------- the frozen regressor on phi_tilde (eval mode: no dropout) ----------------
            y = self._dev["y0"].view(1, o).expand(rows, o).contiguous()
            reg = []
            for _ in range(_REG_ITERS):
                inp = torch.empty((rows, self._dp), dtype=self._dtype, device=self._device)
                _lib.check(lib.r50_op_concat_pad(phi_tilde.data_ptr(), d, y.data_ptr(), o, rows, inp.data_ptr(), self._dp, self._et,
                                                 self._stream()), None, "r50_op_concat_pad")
                r1 = self._gemm(inp, "mlp0", relu=True)
                r2 = self._gemm(r1, "mlp3", relu=True)
                dy = self._gemm(r2, "mlp5", relu=False)
                _lib.check(lib.r50_op_add_rows(y.data_ptr(), o, dy.data_ptr(), self._op, rows, self._et, self._stream()), None, "r50_op_add_rows")
                reg.append((None, r1, r2))
            # ---------------- the pose loss over all frames and its gradient ----------------
            gt = joints3d.to(torch.float32).contiguous()
            dyacc = torch.empty((rows, o), dtype=torch.float32, device=self._device)
            losses = torch.empty(3, dtype=torch.float32, device=self._device)
            _lib.check(lib.r50_op_mse_loss_grad(y.data_ptr(), gt.data_ptr(), rows * o, loss_scale, dyacc.data_ptr(), losses.data_ptr(),
                                                self._stream()), None, "r50_op_mse_loss_grad")
            # ---------------- backward through the regressor: dX only (its weights are frozen) ----------------
            dh_reg, _g5 = self._regressor_backward(reg, dyacc, rows, inv, 1.0, weights=False)
            # ---------------- latent loss + cast: f_hal's output gradient, in the arena ----------------
            dh = self._arena.take(rows, d)
            self._latent_loss(phi_tilde, phi, dh_reg, rows, self.lambda_latent, loss_scale, dh, losses[2:])
            self._last_dh, self._last_dh_reg = dh, dh_reg
            # ---------------- backward: fc2, the ReLU, fc1; input_proj is frozen, so no dX beyond that ----------------
            self._wgrad("f_hal.fc2.w", dh, h1, inv, False, bias="f_hal.fc2.b")
            dh1 = self._mm(dh, self._wt["f_hal.fc2.w"])
            self._relu_bwd(dh1, h1, 1.0)
            self._wgrad("f_hal.fc1.w", dh1, x, inv, False, bias="f_hal.fc1.b")
            self._check_arena()                                                  # every 16-bit gradient the GEMMs and the latent kernel wrote
        return y.view(b, t, self.joints_num, 3), losses

    def train_step(self, feats: torch.Tensor, joints3d: torch.Tensor, optim: AdamW, scaler: Optional[GradScaler] = None,
                   masks: Optional[Dict[str, torch.Tensor]] = None, group=None) -> Tuple[float, float, bool]:
        """One step of the stage: forward + loss, scaled backward, inf check, AdamW over f_hal, scale update
        (``TrainableHead.train_step``'s contract; ``masks`` is accepted for the shared epoch loop and must be empty: the stage has no
        dropout site).  Returns (loss, mpjpe_tilde, skipped); ``last_losses`` holds loss, l3d_tilde, l_lat and mpjpe_tilde."""
        if masks:
            raise ValueError("the hallucinator stage has no dropout site: masks must be empty")
        scale = scaler.get_scale() if scaler is not None else 1.0
        _, losses = self.forward_backward(feats, joints3d, scale)
        found = self._finish_step(optim, scaler, group)
        l3d_tilde, mpjpe_tilde, l_lat = losses.tolist()
        loss = l3d_tilde + self.lambda_latent * l_lat
        self.last_losses = {"loss": loss, "l3d_tilde": l3d_tilde, "l_lat": l_lat, "mpjpe_tilde": mpjpe_tilde}
        return loss, mpjpe_tilde, found


@torch.no_grad()
def evaluate_hal(head, store, batch_size: int) -> Tuple[float, float]:
    """The stage's validation pass: (l3d_tilde, mpjpe_tilde) of ``head.hallucinate`` -- every frame reconstructed from itself alone --,
    each the mean over batches of the per-batch mean, the items of ``store`` in order, ``batch_size`` at a time, the last batch kept
    even if short (as ``train.evaluate``).  One ``r50_op_pose_metrics`` launch per batch adds into a device accumulator, read once.
    The head's mode is restored; its weights are not touched."""
    was_training = head.training
    head.train(False)
    lib = _lib.load_library()
    dev = head._device
    try:
        with torch.cuda.device(dev):
            acc = torch.zeros(3, dtype=torch.float64, device=dev)
            for s in range(0, len(store), batch_size):
                batch = store.get_batch(list(range(s, min(s + batch_size, len(store)))))
                pred = head.hallucinate(batch[0])[1]
                gt = batch[1].to(device=dev, dtype=torch.float32).contiguous()
                _lib.check(lib.r50_op_pose_metrics(pred.data_ptr(), gt.data_ptr(), pred.shape[0] * pred.shape[1], head.joints_num,
                                                   acc.data_ptr(), head._stream()), None, "r50_op_pose_metrics")
            l3d, mpjpe, n = acc.tolist()
    finally:
        head.train(was_training)
    n = max(n, 1.0)
    return l3d / n, mpjpe / n


# ---- the driver -------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    """Phase 1's flags and defaults (``train.build_parser``; ``--seed`` also seeds a fresh f_hal), ``--outdir ./runs/hal``, plus
    ``--init`` and ``--lambda-latent``."""
    p = argparse.ArgumentParser("Hallucinator training: freeze input_proj, f_movie, f_AR and f_3D, train f_hal (3D joints + latent strips "
                                "from single frames)", parents=[_phase1_parser()], add_help=False)
    p.set_defaults(outdir="./runs/hal")
    p.add_argument("--init", type=str, default=None,
                   help="checkpoint (its 'model') or plain state dict to start from; an f_hal it carries is trained on, else a fresh one "
                        "is drawn under --seed; required unless --resume names an existing file")
    p.add_argument("--lambda-latent", type=float, default=LAMBDA_LATENT,
                   help="weight of the latent loss mean((phi_tilde - phi)^2) over all frames (no run has measured a good value)")
    p.add_argument("--weights-from", choices=("auto", "model", "ema"), default=argparse.SUPPRESS,
                   help="which weights of --init to start from: auto (default) = its EMA weights when it has them, else the raw ones")
    return p


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = build_parser()
    args = validate_clip_ema(p, p.parse_args(argv))
    if not args.init and not (args.resume and os.path.isfile(args.resume)):
        p.error("--init is required unless --resume names an existing checkpoint")
    return args


def hal_head_from_checkpoint(args: argparse.Namespace):
    """``make_head`` of the stage: ``HalTrainableHead`` at the dimensions of ``--init`` (or, without it, ``--resume``), loaded with that
    state plus, where it has no f_hal, ``fresh_hallucinator_state(latent_dim, --seed)``."""
    from .results import infer_head_dims, load_head_state

    def make_head(device):
        state = load_head_state(args.init, getattr(args, "weights_from", "auto")) if args.init else load_head_state(args.resume, "model")
        latent_dim, joints_num, number_blocks = infer_head_dims(state)
        if not has_hallucinator(state):
            state = {**state, **fresh_hallucinator_state(latent_dim, args.seed)}
        head = HalTrainableHead(latent_dim, joints_num, number_blocks, precision=args.precision, lambda_latent=args.lambda_latent)
        head.load_state_dict(state, strict=True)
        return head.to(device)
    return make_head


def main(argv: Optional[List[str]] = None) -> float:
    """The hallucinator stage on one MI355X.  Per epoch, in ``train.main``'s order (``train.fit``): train, evaluate, scheduler step,
    ``last.pt``, ``best.pt`` when the validation score improved by more than ``--early-stop-min-delta``, patience counter.  The score
    is the validation ``mpjpe_tilde`` (``evaluate_hal``).  ``--resume`` loads model and optimizer; the head's dimensions come from the
    checkpoint.  Checkpoints hold the whole model, ``f_hal.*`` included, and the optimizer in ``torch.optim.AdamW``'s layout over the
    four parameters.  Prints one JSON line per epoch.  Returns the best score."""
    args = parse_args(argv)
    r = open_run(args, hal_head_from_checkpoint(args))
    title = "===== Hallucinator training (f_hal) ====="
    banner = [title, f"Device: {r.device} ({args.precision}) | head: latent {r.head.latent_dim}, {r.head.number_blocks} f_movie blocks",
              f"Train clips: {len(r.train_set)} | Val clips: {len(r.val_set)}",
              f"Batch size: {args.batch_size} | LR: {args.lr} | lambda_latent: {args.lambda_latent} | seed: {args.seed}", "=" * len(title)]

    def epoch_fn(epoch):
        tr_loss, tr_mpjpe, steps, skipped = train_epoch(r.head, r.train_set, r.sampler, r.optim, r.scaler, args.seed, epoch, args.log_every)

        def validate():
            va_l3d, va_mpjpe = evaluate_hal(r.head, r.val_set, args.batch_size)
            return va_mpjpe, {"val_l3d_tilde": va_l3d, "val_mpjpe_tilde": va_mpjpe}, \
                f"Val:   l3d_tilde={va_l3d:.6f} | single-frame mpjpe={va_mpjpe:.3f}"

        score, va_fields, va_lines = validate_with_ema(r, validate)
        return score, {"train_loss": tr_loss, "train_mpjpe_tilde": tr_mpjpe, "steps": steps, "skipped": skipped, **va_fields,
                       **clip_fields(r)}, (f"Train: loss={tr_loss:.6f} | single-frame mpjpe={tr_mpjpe:.3f}",) + va_lines

    return fit(r, args, banner, epoch_fn, "single-frame MPJPE")


if __name__ == "__main__":
    main()
