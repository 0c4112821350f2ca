"""CPU restatement of the autoregressive rollout (``PHDFor3DJoints.rollout``) for the tests, built from the
lifting oracle's pieces and tests/ar_reference.py's f_AR::

    phi = f_movie(input_proj(feats[:, :I]))                      # observed strips only
    seq = phi
    for _ in range(P): seq = cat([seq, f_AR(seq)[:, -1:]], 1)   # f_AR recomputed over the whole sequence
    future = seq[:, I:]; joints = f_3D(future)

``store16`` ("fp16" / "bf16") emulates the device's 16-bit storage in fp64: weights rounded once; every tensor the device stores
in 16 bits (the cast features, each GEMM output after bias and residual, each GroupNorm + ReLU output, the regressor's
[phi | y] input) rounded to it; biases, GroupNorm parameters and the regressor's running y stay wide (fp32 on the device).  Pinned
by tests/golden/rollout_golden.pt (the reference module itself)."""
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import lifting_oracle as lo
from tests.ar_reference import _f_ar

_DT16 = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _r16(x: torch.Tensor, store16: Optional[str]) -> torch.Tensor:
    return x if store16 is None else x.to(_DT16[store16]).to(x.dtype)


def _blocks(x_btd: torch.Tensor, p: Dict[str, torch.Tensor], prefix: str, store16: Optional[str]) -> torch.Tensor:
    """CausalTemporalNet (src/model.py:69-78) in eval mode with the device's 16-bit stores."""
    x = x_btd.permute(0, 2, 1)
    i = 0
    while f"{prefix}.blocks.{i}.gn1.weight" in p:
        q = f"{prefix}.blocks.{i}"
        h = _r16(F.relu(F.group_norm(x, 32, p[q + ".gn1.weight"], p[q + ".gn1.bias"], eps=1e-5)), store16)
        h = _r16(lo._causal_conv1d(h, p[q + ".conv1.conv.weight"], p[q + ".conv1.conv.bias"]), store16)
        h = _r16(F.relu(F.group_norm(h, 32, p[q + ".gn2.weight"], p[q + ".gn2.bias"], eps=1e-5)), store16)
        x = _r16(lo._causal_conv1d(h, p[q + ".conv2.conv.weight"], p[q + ".conv2.conv.bias"]) + x, store16)
        i += 1
    return x.permute(0, 2, 1)


def _regressor(phi: torch.Tensor, p: Dict[str, torch.Tensor], store16: Optional[str], iters: int = 3) -> torch.Tensor:
    b, t, _ = phi.shape
    y = p["f_3D.y0"].view(1, 1, -1).expand(b, t, -1).contiguous()
    for _ in range(iters):
        h = torch.cat([phi, _r16(y, store16)], dim=-1)
        h = _r16(F.relu(F.linear(h, p["f_3D.mlp.0.weight"], p["f_3D.mlp.0.bias"])), store16)
        h = _r16(F.relu(F.linear(h, p["f_3D.mlp.3.weight"], p["f_3D.mlp.3.bias"])), store16)
        y = y + _r16(F.linear(h, p["f_3D.mlp.5.weight"], p["f_3D.mlp.5.bias"]), store16)
    return y.view(b, t, -1, 3)


def _params(sd: Dict[str, torch.Tensor], dtype, store16: Optional[str]) -> Dict[str, torch.Tensor]:
    p = {k: v.detach().to(dtype) for k, v in sd.items()}
    if store16 is not None:
        for k in p:
            if k.endswith("conv.weight") or k in ("input_proj.weight", "f_3D.mlp.0.weight", "f_3D.mlp.3.weight", "f_3D.mlp.5.weight"):
                p[k] = _r16(p[k], store16)
    return p


@torch.no_grad()
def rollout_reference(sd: Dict[str, torch.Tensor], feats: torch.Tensor, input_len: int, pred_len: int, dtype=torch.float64,
                      store16: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(future_phi (B,P,D), future_joints (B,P,J,3)) in ``dtype``.  store16=None: the plain program (tests/ar_reference.py's f_AR);
    "fp16" / "bf16": with the device's 16-bit storage emulated."""
    p = _params(sd, dtype, store16)
    x = _r16(F.linear(_r16(feats[:, :input_len].to(dtype), store16), p["input_proj.weight"], p["input_proj.bias"]), store16)
    seq = _blocks(x, p, "f_movie", store16)
    for _ in range(pred_len):
        ar = _f_ar(p, seq, None) if store16 is None else _blocks(seq, p, "f_AR", store16)
        seq = torch.cat([seq, ar[:, -1:]], dim=1)
    future = seq[:, input_len:]
    return future, (lo._regressor(future, p) if store16 is None else _regressor(future, p, store16))


def case_feats(seed: int, b: int, t: int) -> torch.Tensor:
    """The features of a golden case (tests/golden/make_golden_rollout.py): (B, T, 2048) fp32, non-negative like pooled ResNet
    features.  feats[:, input_len:] exist only to show that the rollout never reads them."""
    return torch.randn(b, t, 2048, generator=torch.Generator().manual_seed(900 + seed)).abs()


def horizon_sums(pred: torch.Tensor, gt: torch.Tensor, input_len: int) -> torch.Tensor:
    """The accumulator r50_op_horizon_metrics adds, in fp64: [per-horizon distance sums (P) | squared-error sums (P) | clips]."""
    p = pred.shape[1]
    d = pred.double() - gt[:, input_len:input_len + p].double()
    return torch.cat([d.norm(dim=-1).sum(dim=(0, 2)), d.pow(2).sum(dim=(0, 2, 3)), torch.tensor([float(pred.shape[0])], dtype=torch.float64)])
