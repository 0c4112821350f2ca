"""CPU restatement of the rollout objective (``ARTrainableHead.rollout_train_step``) with torch autograd,
for the tests::

    phi_obs = f_movie(input_proj(feats[:, :I])); phi_all = f_movie(input_proj(feats))      # frozen, no gradient
    seq = phi_obs
    for _ in range(k): seq = cat([seq, f_AR(seq)[:, -1:]], 1)                             # full BPTT through every strip
    fut = seq[:, I:]
    loss = mean((f_3D(fut) - gt[:, I:I+k])^2) + lambda_latent * mean((fut - phi_all[:, I:I+k])^2)

f_AR in train mode with explicit keep-masks (``masks[j]["f_AR.blocks.i"]``, ((I+j)*B, D), time-major as the device draws them) or
in eval mode (None).  ``store16`` ("fp16" / "bf16") emulates the device's 16-bit storage in fp64 in BOTH directions: every tensor
the device stores in 16 bits in the forward (as tests/rollout_reference.py) is rounded, and so is the gradient that reaches it in
the backward -- the device's dX products, GroupNorm-backward outputs, casts of the fp32 strip gradients and regressor gradients are
16-bit too.  It rounds the gradient of a GroupNorm output once where the device rounds each of its three conv taps, and keeps the
weight-gradient products wide: an emulation for sizing tolerances, not a bit model.  Pinned by tests/golden/train_rollout_golden.pt
(the reference module itself)."""
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import lifting_oracle as lo
from tests.rollout_reference import _DT16, _blocks, _params

AR_BLOCKS = 3


class _Round16(torch.autograd.Function):
    """Round to the 16-bit type in the forward and the gradient in the backward (both kept in the input's dtype)."""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).to(g.dtype), None


def _q(x: torch.Tensor, store16: Optional[str]) -> torch.Tensor:
    return x if store16 is None else _Round16.apply(x, _DT16[store16])


def _f_ar(p: Dict[str, torch.Tensor], seq: torch.Tensor, masks: Optional[Dict[str, torch.Tensor]], store16: Optional[str],
          keep: float = 0.5) -> torch.Tensor:
    """f_AR (src/model.py:37-78) on seq (B, L, D); a mask (L*B, D) time-major after each block's conv1, None: identity."""
    b, n, d = seq.shape
    x = seq.permute(0, 2, 1)
    for i in range(AR_BLOCKS):
        q = f"f_AR.blocks.{i}"
        h = _q(F.relu(F.group_norm(x, 32, p[q + ".gn1.weight"], p[q + ".gn1.bias"], eps=1e-5)), store16)
        h = _q(lo._causal_conv1d(h, p[q + ".conv1.conv.weight"], p[q + ".conv1.conv.bias"]), store16)
        if masks is not None:
            h = _q(h * masks[q].view(n, b, d).permute(1, 2, 0).to(h.dtype) / keep, store16)
        h = _q(F.relu(F.group_norm(h, 32, p[q + ".gn2.weight"], p[q + ".gn2.bias"], eps=1e-5)), store16)
        x = _q(lo._causal_conv1d(h, p[q + ".conv2.conv.weight"], p[q + ".conv2.conv.bias"]) + x, store16)
    return x.permute(0, 2, 1)


def _regressor(fut: torch.Tensor, p: Dict[str, torch.Tensor], store16: Optional[str], iters: int = 3) -> torch.Tensor:
    """JointRegressor (src/model.py:87-126) in eval mode; y stays wide, as on the device."""
    b, t, _ = fut.shape
    y = p["f_3D.y0"].view(1, 1, -1).expand(b, t, -1)
    for _ in range(iters):
        h = torch.cat([fut, _q(y, store16)], dim=-1)
        h = _q(F.relu(F.linear(h, p["f_3D.mlp.0.weight"], p["f_3D.mlp.0.bias"])), store16)
        h = _q(F.relu(F.linear(h, p["f_3D.mlp.3.weight"], p["f_3D.mlp.3.bias"])), store16)
        y = y + _q(F.linear(h, p["f_3D.mlp.5.weight"], p["f_3D.mlp.5.bias"]), store16)
    return y.view(b, t, -1, 3)


def _teacher(p, feats, store16):
    x = _q(F.linear(_q(feats, store16), p["input_proj.weight"], p["input_proj.bias"]), store16)
    return _blocks(x, p, "f_movie", store16) if store16 is not None else lo._temporal_net(x, p, "f_movie")


def rollout_losses(p: Dict[str, torch.Tensor], feats: torch.Tensor, gt: torch.Tensor, input_len: int, k: int, lambda_latent: float,
                   masks: Optional[List[Dict[str, torch.Tensor]]] = None, store16: Optional[str] = None):
    """(loss, l3d, l_lat, mpjpe, future joints (B,k,J,3)) of one batch, differentiable in p's f_AR entries."""
    with torch.no_grad():
        phi_obs = _teacher(p, feats[:, :input_len], store16)
        phi_all = _teacher(p, feats, store16)
    seq = phi_obs
    for j in range(k):
        seq = torch.cat([seq, _f_ar(p, seq, masks[j] if masks is not None else None, store16)[:, -1:]], dim=1)
    fut = seq[:, input_len:]
    joints = _regressor(fut, p, store16)
    l3d = (joints - gt[:, input_len:input_len + k]).pow(2).mean()
    l_lat = (fut - phi_all[:, input_len:input_len + k]).pow(2).mean()
    mpjpe = torch.norm(joints.detach() - gt[:, input_len:input_len + k], dim=-1).mean()
    return l3d + lambda_latent * l_lat, l3d, l_lat, mpjpe, joints.detach()


def train_rollout_steps_reference(sd: Dict[str, torch.Tensor], batches, input_len: int, k: int, masks_per_step=None, lr: float = 1e-4,
                                  lambda_latent: float = 1.0, weight_decay: float = 1e-2, dtype=torch.float32,
                                  store16: Optional[str] = None, loss_scale: float = 1.0):
    """len(batches) steps of the rollout objective.  batches: [(feats (B,T,2048), joints3d (B,T,17,3))].  ``loss_scale``: the
    backward runs on loss_scale * loss and the gradients are divided back (what GradScaler does; it matters to the 16-bit emulation).
    Returns (per step [loss, l3d, l_lat, mpjpe], gradients of the FIRST step, final state dict)."""
    p = {n: v.detach().clone().to(dtype) for n, v in sd.items()}          # the wide master copies
    frozen16 = _params(sd, dtype, store16)                                 # the frozen weights as the device's GEMMs read them
    trainable = [n for n in p if n.startswith("f_AR.")]
    for n in trainable:
        p[n].requires_grad_(True)
    opt = torch.optim.AdamW([p[n] for n in trainable], lr=lr, weight_decay=weight_decay)
    losses, first_grads = [], None
    for s, (feats, gt) in enumerate(batches):
        opt.zero_grad(set_to_none=True)
        pw = dict(frozen16)
        for n in trainable:                    # the GEMMs read the 16-bit copy of the master weights; the gradient reaches the master
            w = p[n]
            pw[n] = w + (w.to(_DT16[store16]).to(dtype) - w).detach() if store16 is not None and n.endswith("conv.weight") else w
        out = rollout_losses(pw, feats.to(dtype), gt.to(dtype), input_len, k, lambda_latent,
                             masks_per_step[s] if masks_per_step is not None else None, store16)
        (out[0] * loss_scale).backward()
        if loss_scale != 1.0:
            for n in trainable:
                p[n].grad.div_(loss_scale)
        if first_grads is None:
            first_grads = {n: p[n].grad.detach().clone() for n in trainable}
        opt.step()
        losses.append([float(v.detach()) for v in out[:4]])
    return losses, first_grads, {n: v.detach().clone() for n, v in p.items()}
