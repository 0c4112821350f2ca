"""fp64 restatement of the tail of a training step with global-norm gradient clipping and EMA weights,
over a list of tensors:

    norm  = sqrt(sum over every tensor of g^2)                               torch.nn.utils.clip_grad_norm_
    coef  = min(1, max_norm / (norm + 1e-6))                                 (max_norm None: 1)
    g'    = g * coef
    p     = p * (1 - lr * wd);  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
    p    -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)         torch.optim.AdamW
    ema  += w * (p - ema)                                                    torch.optim.swa_utils.get_ema_multi_avg_fn, w = 1 - decay

tests/test_clip_ema_cpu.py holds it to torch's own functions; tests/test_clip_ema_gpu.py holds the device path to it."""
import math
from typing import List, Optional, Sequence

import torch


def global_norm(grads: Sequence[torch.Tensor]) -> float:
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))


def clip_coef(norm: float, max_norm: Optional[float]) -> float:
    if max_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, float(max_norm) / (norm + 1e-6))


def ema_weight(decay: float, updates: int, warmup: bool = True) -> float:
    """1 - (the effective decay of update ``updates``, 0-based): min(decay, (1 + u) / (10 + u)) with warm-up."""
    return 1.0 - (min(decay, (1.0 + updates) / (10.0 + updates)) if warmup else decay)


class ClipAdamWEMA:
    """The state of the restatement: parameters, AdamW moments and the EMA, all fp64."""

    def __init__(self, params: Sequence[torch.Tensor], lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_norm: Optional[float] = None, ema: bool = True):
        self.p = [t.detach().double().clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.ema: Optional[List[torch.Tensor]] = [t.clone() for t in self.p] if ema else None
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_norm
        self.t = 0
        self.coefs: List[float] = []
        self.norms: List[float] = []

    def step(self, grads: Sequence[torch.Tensor], w: float = 0.0) -> None:
        """One applied step from the UNCLIPPED gradients; ``w``: the EMA's lerp weight of this step."""
        norm = global_norm(grads)
        coef = clip_coef(norm, self.max_norm)
        self.norms.append(norm)
        self.coefs.append(coef)
        self.t += 1
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        for i, g in enumerate(grads):
            g = g.double() * coef
            self.p[i] = self.p[i] * (1.0 - self.lr * self.wd)
            self.m[i] = b1 * self.m[i] + (1.0 - b1) * g
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
            self.p[i] = self.p[i] - (self.lr / bc1) * self.m[i] / (self.v[i].sqrt() / math.sqrt(bc2) + self.eps)
            if self.ema is not None:
                self.ema[i] = self.ema[i] + w * (self.p[i] - self.ema[i])
