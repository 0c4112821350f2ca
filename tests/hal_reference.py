"""CPU restatement of the hallucinator stage (implementation_phd_lab_vision_amd/train_hal.py) with torch
autograd, for the tests: ``f_hal(x) = x + fc2(relu(fc1(x)))`` on ``x = input_proj(feats)``, everything but f_hal frozen and in eval
mode, loss ``l3d_tilde + lambda_latent * l_lat`` over all frames, torch.optim.AdamW over f_hal's four parameters; the single-frame
forward and the forecast from one frame.  Built from the lifting oracle's pieces (oracle/lifting_oracle.py, imported, not changed).
The reference has no such module, so nothing pins this file from outside: ``latent_grad_analytic`` against autograd (tests/test_hal_cpu.py)
guards the part the GPU kernel is held to."""
from typing import Dict, List

import torch
import torch.nn.functional as F

from oracle import lifting_oracle as lo

HAL_KEYS = ("f_hal.fc1.weight", "f_hal.fc1.bias", "f_hal.fc2.weight", "f_hal.fc2.bias")


def synthetic_hal_state(latent_dim: int, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded f_hal weights (NOT torch's initialisation: the tests pin the arithmetic); scales keep activations O(1)."""
    g = torch.Generator().manual_seed(seed)
    d = latent_dim
    return {"f_hal.fc1.weight": torch.randn(d, d, generator=g) * d ** -0.5, "f_hal.fc1.bias": torch.randn(d, generator=g) * 0.05,
            "f_hal.fc2.weight": torch.randn(d, d, generator=g) * d ** -0.5, "f_hal.fc2.bias": torch.randn(d, generator=g) * 0.05}


def f_hal(p: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """Hallucinator.forward on x (..., D)."""
    return x + F.linear(F.relu(F.linear(x, p["f_hal.fc1.weight"], p["f_hal.fc1.bias"])), p["f_hal.fc2.weight"], p["f_hal.fc2.bias"])


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


@torch.no_grad()
def hallucinate_reference(sd: Dict[str, torch.Tensor], feats: torch.Tensor, dtype=torch.float64):
    """(phi_tilde (B,T,D), joints (B,T,J,3)) of ``PHDFor3DJoints.hallucinate``."""
    p = _cast(sd, dtype)
    phi_tilde = f_hal(p, F.linear(feats.to(dtype), p["input_proj.weight"], p["input_proj.bias"]))
    return phi_tilde, lo._regressor(phi_tilde, p)


@torch.no_grad()
def rollout_from_reference(sd: Dict[str, torch.Tensor], seq: torch.Tensor, pred_len: int, dtype=torch.float64):
    """``seq`` (B, I, D) observed strips -> (future strips (B, P, D), future joints (B, P, J, 3)): f_AR over the whole sequence at every
    step, its last frame appended."""
    p = _cast(sd, dtype)
    seq = seq.to(dtype)
    i_len = seq.shape[1]
    for _ in range(pred_len):
        seq = torch.cat([seq, lo._temporal_net(seq, p, "f_AR")[:, -1:]], dim=1)
    return seq[:, i_len:], lo._regressor(seq[:, i_len:], p)


@torch.no_grad()
def hallucinated_rollout_reference(sd: Dict[str, torch.Tensor], feats: torch.Tensor, frame: int, pred_len: int, dtype=torch.float64):
    """``PHDFor3DJoints.hallucinated_rollout``: the rollout whose only observed strip is f_hal's for ``feats[:, frame]``."""
    phi_tilde, _ = hallucinate_reference(sd, feats[:, frame: frame + 1], dtype)
    return rollout_from_reference(sd, phi_tilde, pred_len, dtype)


def hal_losses(p: Dict[str, torch.Tensor], feats: torch.Tensor, gt: torch.Tensor, lambda_latent: float):
    """(loss, l3d_tilde, l_lat, mpjpe_tilde) of one batch, differentiable in p's f_hal entries."""
    x = F.linear(feats, p["input_proj.weight"], p["input_proj.bias"])
    phi = lo._temporal_net(x, p, "f_movie").detach()
    phi_tilde = f_hal(p, x)
    joints = lo._regressor(phi_tilde, p)
    l3d_tilde = (joints - gt).pow(2).mean()
    l_lat = (phi_tilde - phi).pow(2).mean()
    mpjpe_tilde = torch.norm(joints.detach() - gt, dim=-1).mean()
    return l3d_tilde + lambda_latent * l_lat, l3d_tilde, l_lat, mpjpe_tilde


def train_hal_steps_reference(sd: Dict[str, torch.Tensor], batches, lr: float = 1e-4, lambda_latent: float = 1.0, weight_decay: float = 1e-2,
                              dtype=torch.float32):
    """len(batches) steps of the stage (no loss scaling on the CPU).  batches: [(feats (B,T,2048), joints3d (B,T,17,3))].
    Returns (per step [loss, l3d_tilde, l_lat, mpjpe_tilde], per step the gradients, per step the f_hal parameters after it)."""
    p = {k: v.detach().clone().to(dtype) for k, v in sd.items()}
    for k in HAL_KEYS:
        p[k].requires_grad_(True)
    opt = torch.optim.AdamW([p[k] for k in HAL_KEYS], lr=lr, weight_decay=weight_decay)
    losses: List[List[float]] = []
    grads, params = [], []
    for feats, gt in batches:
        opt.zero_grad(set_to_none=True)
        out = hal_losses(p, feats.to(dtype), gt.to(dtype), lambda_latent)
        out[0].backward()
        grads.append({k: p[k].grad.detach().clone() for k in HAL_KEYS})
        opt.step()
        params.append({k: p[k].detach().clone() for k in HAL_KEYS})
        losses.append([float(v.detach()) for v in out])
    return losses, grads, params


def latent_grad_analytic(h: torch.Tensor, phi: torch.Tensor, dh_reg: torch.Tensor, lam: float, loss_scale: float):
    """What ``r50_op_hal_latent_grad`` computes before its cast, in the dtype of its arguments: (dh, l_lat) with
    ``dh = dh_reg + lam * 2 / n * loss_scale * (h - phi)``, ``l_lat = mean((h - phi)^2)``, n = h.numel()."""
    diff = h - phi
    return dh_reg + lam * 2.0 / diff.numel() * loss_scale * diff, diff.pow(2).mean()


# ---- fp64 emulation of the step's 16-bit storage (scripts/hal_emulation_distances.py; the numbers behind the bars that are not phase 1's) ----
# The cases of tests/test_hal_gpu.py::test_train_steps_equal_the_restatement: PHD(128, 17, 2) + f_hal, two AdamW steps.
STEP_CASES = ((4, 8), (2, 2))                        # (B, T)
STEP_LR, STEP_LAMBDA, STEP_LOSS_SCALE = 1e-3, 0.5, 1024.0


def step_case_state(b: int):
    """(state dict, the two batches) of the step case with batch size ``b``."""
    sd = {**lo.synthetic_head_state_dict(128, 2, 60 + b), **synthetic_hal_state(128, 1060 + b)}
    g = torch.Generator().manual_seed(600 + b)
    return sd, [(torch.randn(b, t_, 2048, generator=g).abs(), torch.randn(b, t_, 17, 3, generator=g) * 0.5)
                for t_ in [dict(STEP_CASES)[b]] * 2]


class _Store16(torch.autograd.Function):
    """A tensor the device stores in 16 bits: the value is rounded on the way forward and its gradient on the way back (the backward
    GEMM that produces it stores 16 bits too)."""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).to(g.dtype), None


def train_hal_steps_emulated(sd: Dict[str, torch.Tensor], batches, store16: str, lr: float = 1e-4, lambda_latent: float = 1.0,
                             weight_decay: float = 1e-2, loss_scale: float = 1024.0):
    """``train_hal_steps_reference`` in fp64 with the device's 16-bit storage emulated (tests/rollout_reference.py's rules for the
    forward; in the backward every gradient a GEMM or the latent kernel stores -- the regressor's dX chain, f_hal's output gradient,
    the hidden rows' gradient, the two weight gradients -- is rounded in the loss-scaled domain; bias gradients, the regressor's
    accumulated dy and dX, the masters and AdamW stay wide)."""
    from tests import rollout_reference as rr
    dt = rr._DT16[store16]
    s16 = lambda v: _Store16.apply(v, dt)                                   # noqa: E731
    frozen = rr._params({k: v for k, v in sd.items() if k not in HAL_KEYS}, torch.float64, store16)
    master = {k: sd[k].detach().double().clone().requires_grad_(True) for k in HAL_KEYS}
    opt = torch.optim.AdamW([master[k] for k in HAL_KEYS], lr=lr, weight_decay=weight_decay)
    losses: List[List[float]] = []
    grads, params = [], []
    for feats, gt in batches:
        opt.zero_grad(set_to_none=True)
        gt = gt.double()
        with torch.no_grad():
            x = rr._r16(F.linear(rr._r16(feats.double(), store16), frozen["input_proj.weight"], frozen["input_proj.bias"]), store16)
            phi = rr._blocks(x, frozen, "f_movie", store16)
        h1 = s16(F.relu(F.linear(x, s16(master["f_hal.fc1.weight"]), master["f_hal.fc1.bias"])))
        phi_tilde = s16(F.linear(h1, s16(master["f_hal.fc2.weight"]), master["f_hal.fc2.bias"]) + x)
        b, t, _ = phi_tilde.shape
        y = frozen["f_3D.y0"].view(1, 1, -1).expand(b, t, -1).contiguous()
        for _ in range(3):
            h = s16(torch.cat([phi_tilde, y], dim=-1))
            h = s16(F.relu(F.linear(h, frozen["f_3D.mlp.0.weight"], frozen["f_3D.mlp.0.bias"])))
            h = s16(F.relu(F.linear(h, frozen["f_3D.mlp.3.weight"], frozen["f_3D.mlp.3.bias"])))
            y = y + s16(F.linear(h, frozen["f_3D.mlp.5.weight"], frozen["f_3D.mlp.5.bias"]))
        joints = y.view(b, t, -1, 3)
        l3d = (joints - gt).pow(2).mean()
        l_lat = (phi_tilde - phi).pow(2).mean()
        (loss_scale * (l3d + lambda_latent * l_lat)).backward()
        for k in HAL_KEYS:
            master[k].grad /= loss_scale
        grads.append({k: master[k].grad.detach().clone() for k in HAL_KEYS})
        opt.step()
        params.append({k: master[k].detach().clone() for k in HAL_KEYS})
        mpjpe = torch.norm(joints.detach() - gt, dim=-1).mean()
        losses.append([float(l3d.detach() + lambda_latent * l_lat.detach()), float(l3d.detach()), float(l_lat.detach()), float(mpjpe)])
    return losses, grads, params


def step_distances(got, want, sd, lr: float) -> Dict[str, float]:
    """The six distances the step test bounds, the largest over the two steps and the four parameters: ``got`` / ``want`` are
    (losses, grads, params) of two runs of the same case.  loss: relative; grad_norm: relative; grad_head: relative L2 of the first 64
    entries; upd_median / upd_max: |update error| of the first 64 entries over lr; upd_rel: their relative L2."""
    d = {"loss": 0.0, "grad_norm": 0.0, "grad_head": 0.0, "upd_median": 0.0, "upd_rel": 0.0, "upd_max": 0.0}

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
    for s in range(len(want[0])):
        for g, w in zip(got[0][s], want[0][s]):
            d["loss"] = max(d["loss"], abs(g - w) / abs(w))
        for k in HAL_KEYS:
            gn, wn = float(got[1][s][k].norm()), float(want[1][s][k].norm())
            d["grad_norm"] = max(d["grad_norm"], abs(gn - wn) / wn)
            d["grad_head"] = max(d["grad_head"], rel(got[1][s][k].reshape(-1)[:64], want[1][s][k].reshape(-1)[:64]))
            dw = (want[2][s][k].double() - sd[k].double()).reshape(-1)[:64]
            dg = (got[2][s][k].double() - sd[k].double()).reshape(-1)[:64]
            err = (dg - dw).abs()
            d["upd_median"] = max(d["upd_median"], float(err.median()) / lr)
            d["upd_rel"] = max(d["upd_rel"], rel(dg, dw))
            d["upd_max"] = max(d["upd_max"], float(err.max()) / lr)
    return d
