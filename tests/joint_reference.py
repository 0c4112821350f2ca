"""CPU restatement of the joint training step (``JointTrainableHead.train_step``) with torch autograd, for
the tests::

    phi = f_movie(input_proj(feats)); ar = f_AR(phi); phi_hat = [0, ar[:, :-1]]
    loss = mean((f_3D(phi) - gt)^2) + lambda_future * mean((f_3D(phi_hat)[:, 1:] - gt[:, 1:])^2)
           + lambda_latent * mean((phi_hat[:, 1:] - phi[:, 1:].detach())^2)

every parameter trainable, ``torch.optim.AdamW`` over them in ``named_parameters()`` order.  Dropout with explicit keep-masks, laid
out as ``JointTrainableHead.make_dropout_masks`` draws them ("f_movie.blocks.i" / "f_AR.blocks.i" (B*T, D) after each block's conv1,
"f_3D.i" / "f_3D_hat.i" (B*T, 1024) after the regressor's first ReLU of f_3D(phi) / f_3D(phi_hat)), or eval mode (None).  Built from
the lifting oracle's pieces as tests/ar_reference.py is.

``store16`` ("fp16" / "bf16") emulates the device's 16-bit storage in fp64 in both directions, as tests/rollout_train_reference.py
does: every tensor the device stores in 16 bits in the forward is rounded, and so is the gradient that reaches it; the GEMMs read
16-bit copies of the master weights, whose gradients reach the wide master.  It keeps the weight-gradient products wide and rounds a
GroupNorm output's gradient once where the device rounds each of its three conv taps: an emulation for sizing tolerances, not a bit
model.  Pinned by tests/golden/train_joint_golden.pt (the reference module itself)."""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import lifting_oracle as lo
from tests.rollout_reference import _DT16
from tests.rollout_train_reference import _q

AR_BLOCKS = 3
_W16 = ("input_proj.weight", "f_3D.mlp.0.weight", "f_3D.mlp.3.weight", "f_3D.mlp.5.weight")     # + every conv.weight


def _net(p: Dict[str, torch.Tensor], x_btd: torch.Tensor, prefix: str, nb: int, masks: Optional[Dict[str, torch.Tensor]],
         store16: Optional[str], keep: float = 0.5) -> torch.Tensor:
    """CausalTemporalNet (src/model.py:37-78) on (B, T, D); masks[prefix.blocks.i] (B*T, D) batch-major after conv1, None: identity."""
    b, t, _ = x_btd.shape
    x = x_btd.permute(0, 2, 1)
    for i in range(nb):
        q = f"{prefix}.blocks.{i}"
        h = _q(F.relu(F.group_norm(x, 32, p[q + ".gn1.weight"], p[q + ".gn1.bias"], eps=1e-5)), store16)
        h = _q(lo._causal_conv1d(h, p[q + ".conv1.conv.weight"], p[q + ".conv1.conv.bias"]), store16)
        if masks is not None:
            h = _q(h * masks[q].view(b, t, -1).permute(0, 2, 1).to(h.dtype) / keep, store16)
        h = _q(F.relu(F.group_norm(h, 32, p[q + ".gn2.weight"], p[q + ".gn2.bias"], eps=1e-5)), store16)
        x = _q(lo._causal_conv1d(h, p[q + ".conv2.conv.weight"], p[q + ".conv2.conv.bias"]) + x, store16)
    return x.permute(0, 2, 1)


def _regressor(s: torch.Tensor, p: Dict[str, torch.Tensor], masks: Optional[Dict[str, torch.Tensor]], key: str,
               store16: Optional[str], iters: int = 3, keep: float = 0.5) -> torch.Tensor:
    """JointRegressor (src/model.py:87-126) on strips (B, T, D); masks[f"{key}.{i}"] (B*T, 1024) after the first ReLU of iteration
    i.  y stays wide, as on the device."""
    b, t, _ = s.shape
    y = p["f_3D.y0"].to(s.dtype).view(1, 1, -1).expand(b, t, -1)
    for i in range(iters):
        h = _q(F.relu(F.linear(torch.cat([s, _q(y, store16)], dim=-1), p["f_3D.mlp.0.weight"], p["f_3D.mlp.0.bias"])), store16)
        if masks is not None:
            h = _q(h * masks[f"{key}.{i}"].view(b, t, -1).to(h.dtype) / keep, store16)
        h = _q(F.relu(F.linear(h, p["f_3D.mlp.3.weight"], p["f_3D.mlp.3.bias"])), store16)
        y = y + _q(F.linear(h, p["f_3D.mlp.5.weight"], p["f_3D.mlp.5.bias"]), store16)
    return y.view(b, t, -1, 3)


def joint_losses(p: Dict[str, torch.Tensor], feats: torch.Tensor, gt: torch.Tensor, lambda_future: float, lambda_latent: float,
                 masks: Optional[Dict[str, torch.Tensor]] = None, store16: Optional[str] = None):
    """(loss, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat) of one batch, differentiable in every parameter of p."""
    nb = 0
    while f"f_movie.blocks.{nb}.gn1.weight" in p:
        nb += 1
    x = _q(F.linear(_q(feats, store16), p["input_proj.weight"], p["input_proj.bias"]), store16)
    phi = _net(p, x, "f_movie", nb, masks, store16)
    ar = _net(p, phi, "f_AR", AR_BLOCKS, masks, store16)
    phi_hat = torch.cat([torch.zeros_like(ar[:, :1]), ar[:, :-1]], dim=1)
    joints_phi = _regressor(phi, p, masks, "f_3D", store16)
    joints_hat = _regressor(phi_hat, p, masks, "f_3D_hat", store16)
    l3d = (joints_phi - gt).pow(2).mean()
    l3d_hat = (joints_hat[:, 1:] - gt[:, 1:]).pow(2).mean()
    l_lat = (phi_hat[:, 1:] - phi[:, 1:].detach()).pow(2).mean()
    mpjpe = torch.norm(joints_phi.detach() - gt, dim=-1).mean()
    mpjpe_hat = torch.norm(joints_hat[:, 1:].detach() - gt[:, 1:], dim=-1).mean()
    return l3d + lambda_future * l3d_hat + lambda_latent * l_lat, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat


def train_joint_steps_reference(sd: Dict[str, torch.Tensor], batches, masks_per_step=None, lr: float = 1e-4, lambda_future: float = 1.0,
                                lambda_latent: float = 1.0, weight_decay: float = 1e-2, dtype=torch.float32, store16: Optional[str] = None,
                                loss_scale: float = 1.0):
    """len(batches) joint steps.  batches: [(feats (B,T,2048), joints3d (B,T,17,3))].  ``loss_scale``: the backward runs on
    loss_scale * loss and the gradients are divided back (what GradScaler does; it matters to the 16-bit emulation).
    Returns (per step [loss, l3d, mpjpe, l3d_hat, mpjpe_hat, l_lat], gradients of the FIRST step, final state dict)."""
    p = {n: v.detach().clone().to(dtype) for n, v in sd.items()}          # the wide master copies
    trainable = [n for n in p if n != "f_3D.y0"]
    for n in trainable:
        p[n].requires_grad_(True)
    opt = torch.optim.AdamW([p[n] for n in trainable], lr=lr, weight_decay=weight_decay)
    losses, first_grads = [], None
    for s, (feats, gt) in enumerate(batches):
        opt.zero_grad(set_to_none=True)
        pw = dict(p)
        if store16 is not None:                # the GEMMs read the 16-bit copy of the master weights; the gradient reaches the master
            for n in trainable:
                if n.endswith("conv.weight") or n in _W16:
                    w = p[n]
                    pw[n] = w + (w.to(_DT16[store16]).to(dtype) - w).detach()
        out = joint_losses(pw, feats.to(dtype), gt.to(dtype), lambda_future, lambda_latent,
                           masks_per_step[s] if masks_per_step is not None else None, store16)
        (out[0] * loss_scale).backward()
        if loss_scale != 1.0:
            for n in trainable:
                p[n].grad.div_(loss_scale)
        if first_grads is None:
            first_grads = {n: p[n].grad.detach().clone() for n in trainable}
        opt.step()
        losses.append([float(v.detach()) for v in out])
    return losses, first_grads, {n: v.detach().clone() for n, v in p.items()}
