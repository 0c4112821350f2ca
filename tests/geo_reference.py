"""CPU restatement of the geometric pose losses (``r50_op_geo_pose_loss_grad``) with torch autograd, for
the tests.  Written from the formulas of section N::

    uv     = (K P)[:2] / clamp((K P)[2], min=eps)            # the numerator is not clamped
    l3d    = mean (pred - g3d)^2
    l2d    = mean (uv - g2d)^2
    l_vel  = mean ((pred[:, 1:] - pred[:, :-1]) - (g3d[:, 1:] - g3d[:, :-1]))^2
    l_bone = mean (|pred[b] - pred[a]| - |g3d[b] - g3d[a]|)^2 over the edges (a, b)
    loss   = l3d + lambda_2d l2d + lambda_vel l_vel + lambda_bone l_bone

over the frames ``s >= s0`` of every clip.  ``torch.clamp`` passes the gradient at equality and ``torch.norm`` gives the
subgradient 0 at a zero-length bone, which is what the kernel reproduces.  Pinned by tests/golden/geo_golden.pt (the reference's
own ``project_with_K_torch`` / ``bone_length_loss`` under fp64 autograd)."""
from typing import Dict, Optional, Sequence, Tuple

import torch

OUT8 = ("loss", "l3d", "mpjpe", "l2d", "reproj_px", "l_vel", "l_bone", "n_clamped")


def project(p: torch.Tensor, k: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """(B,T,J,3) through K (B,3,3) -> (B,T,J,2)."""
    ph = torch.einsum("bij,btnj->btni", k, p)
    return ph[..., :2] / ph[..., 2:3].clamp(min=eps)


def bone_lengths(p: torch.Tensor, edges: Sequence[Tuple[int, int]]) -> torch.Tensor:
    a = torch.tensor([e[0] for e in edges], dtype=torch.long)
    b = torch.tensor([e[1] for e in edges], dtype=torch.long)
    return torch.norm(p[:, :, b] - p[:, :, a], dim=-1)


def geo_terms(pred: torch.Tensor, g3d: torch.Tensor, g2d: torch.Tensor, k: torch.Tensor, edges, s0: int = 0,
              eps: float = 1e-6) -> Dict[str, torch.Tensor]:
    """The unweighted terms over frames s >= s0, differentiable in ``pred``; empty means (one frame, no edges) are 0."""
    p, g, g2 = pred[:, s0:], g3d[:, s0:], g2d[:, s0:]
    ph = torch.einsum("bij,btnj->btni", k, p)
    uv = ph[..., :2] / ph[..., 2:3].clamp(min=eps)
    zero = pred.new_zeros(())
    return {"l3d": (p - g).pow(2).mean(), "mpjpe": torch.norm(p.detach() - g, dim=-1).mean(), "l2d": (uv - g2).pow(2).mean(),
            "reproj_px": torch.norm(uv.detach() - g2, dim=-1).mean(),
            "l_vel": ((p[:, 1:] - p[:, :-1]) - (g[:, 1:] - g[:, :-1])).pow(2).mean() if p.shape[1] > 1 else zero,
            "l_bone": (bone_lengths(p, edges) - bone_lengths(g, edges)).pow(2).mean() if len(edges) else zero,
            "n_clamped": (ph[..., 2].detach() < eps).sum().to(pred.dtype)}


def geo_loss(pred, g3d, g2d, k, edges, lambdas: Tuple[float, float, float], s0: int = 0, eps: float = 1e-6):
    """(loss, terms): a term whose weight is exactly 0 is left out of the sum (it is still in ``terms``)."""
    tm = geo_terms(pred, g3d, g2d, k, edges, s0, eps)
    loss = tm["l3d"]
    for lam, name in zip(lambdas, ("l2d", "l_vel", "l_bone")):
        if lam != 0:
            loss = loss + lam * tm[name]
    tm["loss"] = loss
    return loss, tm


def geo_loss_grad(pred, g3d, g2d, k, edges, lambdas, s0: int = 0, eps: float = 1e-6, scale: float = 1.0,
                  dtype: Optional[torch.dtype] = torch.float64):
    """(out8 as a tensor in OUT8's order, scale * d loss / d pred (B,T,J,3)) in ``dtype`` from the given inputs."""
    leaf = pred.detach().to(dtype).clone().requires_grad_(True)
    loss, tm = geo_loss(leaf, g3d.to(dtype), g2d.to(dtype), k.to(dtype), edges, lambdas, s0, eps)
    (grad,) = torch.autograd.grad(loss * scale, leaf)
    return torch.stack([tm[n].detach() for n in OUT8]), grad


# ---- the training steps under the composite loss (TrainableHead / JointTrainableHead with ``geo``) ---------------------------------
def head_geo_losses(p, feats, gt, g2d, k, edges, lambdas, joint=None, masks=None, store16=None):
    """One batch through the head restated by tests/joint_reference.py.  ``joint`` None: phase 1, loss = geo_loss(f_3D(phi)), returns
    (loss, [loss, l3d, l2d, l_vel, l_bone]).  ``joint`` = (lambda_future, lambda_latent): loss = geo_loss(joints_phi) + lambda_future *
    geo_loss(joints_hat[:, 1:]) + lambda_latent * l_lat, returns (loss, [loss, the four terms of each half, l_lat])."""
    import torch.nn.functional as F
    from tests.joint_reference import AR_BLOCKS, _net, _regressor
    from tests.rollout_train_reference import _q
    nb = 0
    while f"f_movie.blocks.{nb}.gn1.weight" in p:
        nb += 1
    x = _q(F.linear(_q(feats, store16), p["input_proj.weight"], p["input_proj.bias"]), store16)
    phi = _net(p, x, "f_movie", nb, masks, store16)
    c1, t1 = geo_loss(_regressor(phi, p, masks, "f_3D", store16), gt, g2d, k, edges, lambdas)
    names = ("l3d", "l2d", "l_vel", "l_bone")
    if joint is None:
        return c1, [c1] + [t1[n] for n in names]
    ar = _net(p, phi, "f_AR", AR_BLOCKS, masks, store16)
    phi_hat = torch.cat([torch.zeros_like(ar[:, :1]), ar[:, :-1]], dim=1)
    c2, t2 = geo_loss(_regressor(phi_hat, p, masks, "f_3D_hat", store16), gt, g2d, k, edges, lambdas, s0=1)
    l_lat = (phi_hat[:, 1:] - phi[:, 1:].detach()).pow(2).mean()
    loss = c1 + joint[0] * c2 + joint[1] * l_lat
    return loss, [loss] + [t1[n] for n in names] + [t2[n] for n in names] + [l_lat]


def geo_steps_reference(sd, trainable, batches, edges, lambdas, joint=None, masks_per_step=None, lr: float = 1e-4,
                        weight_decay: float = 1e-2, dtype=torch.float32, store16: Optional[str] = None, loss_scale: float = 1.0):
    """len(batches) AdamW steps over ``trainable`` (names, in the optimizer's order) under the composite loss; batches:
    [(feats, joints3d, joints2d, K)].  ``store16`` / ``loss_scale`` as tests/joint_reference.py's.  Returns (per step the list
    ``head_geo_losses`` gives, gradients of the FIRST step, final state dict)."""
    from tests.joint_reference import _W16
    from tests.rollout_reference import _DT16
    p = {n: v.detach().clone().to(dtype) for n, v in sd.items()}
    for n in trainable:
        p[n].requires_grad_(True)
    opt = torch.optim.AdamW([p[n] for n in trainable], lr=lr, weight_decay=weight_decay)
    losses, first_grads = [], None
    for s, (feats, gt, g2d, k) in enumerate(batches):
        opt.zero_grad(set_to_none=True)
        pw = dict(p)
        if store16 is not None:
            for n in p:
                if n.endswith("conv.weight") or n in _W16:
                    w = p[n]
                    pw[n] = w + (w.to(_DT16[store16]).to(dtype) - w).detach()
        loss, out = head_geo_losses(pw, feats.to(dtype), gt.to(dtype), g2d.to(dtype), k.to(dtype), edges, lambdas, joint,
                                    masks_per_step[s] if masks_per_step is not None else None, store16)
        (loss * loss_scale).backward()
        if loss_scale != 1.0:
            for n in trainable:
                p[n].grad.div_(loss_scale)
        if first_grads is None:
            first_grads = {n: p[n].grad.detach().clone() for n in trainable}
        opt.step()
        losses.append([float(v.detach()) for v in out])
    return losses, first_grads, {n: v.detach().clone() for n, v in p.items()}
