"""Golden joint training steps of the lifting head (input_proj, f_movie, f_AR and f_3D together; implementation_phd_lab_vision_amd/
train_joint.py): the REFERENCE module ``PHDFor3DJoints`` (src/model.py, imported from the reference
checkout with ``torchvision`` -- unused by the head -- replaced by an empty stub), every parameter trainable,
``torch.optim.AdamW(model.parameters(), lr, weight_decay=1e-2)``, two steps of

    phi, phi_hat, joints_phi, joints_hat = model(feats, predict_future=True)
    loss = (joints_phi - gt).pow(2).mean() + lambda_future * (joints_hat[:, 1:] - gt[:, 1:]).pow(2).mean()
           + lambda_latent * (phi_hat[:, 1:] - phi[:, 1:].detach()).pow(2).mean()

on the CPU in fp32.  Dropout is random and not seed-pinned upstream, so the module is stepped in eval mode (dropout = identity);
the dropout sites are covered by the tests' restatement with explicit masks.  The cases are phase 2's three (same weights, same
batches) and a fourth at lambda_future = lambda_latent = 0, where f_AR stays in the graph with all-zero gradients and moves by
AdamW's weight decay alone.  The fixture keeps the trainable names in the order of ``named_parameters()``, per step
[loss, l3d, l3d_hat, l_lat], and per parameter (row i = trainable[i]) the gradient's norm and first 64 entries after step 1
(grad_norm, grad_head) and the parameter's norm and first 64 entries after step 2 (param_norm, param_head).  f_3D.mlp.5.bias has
51 entries: its rows end in 13 NaN (``head_len`` holds each row's length).

    python tests/golden/make_golden_train_joint.py         # needs the reference sources (H36M_REFERENCE_SRC)
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = os.environ.get("H36M_REFERENCE_SRC", "/root/reference/src")
sys.path.insert(0, ROOT)

from tests.golden.make_golden_train_ar import batches_for  # noqa: E402  (phase 2's batches)

LR = 1e-4      # train.py's default (src/config.py LR)
# (latent_dim, number_blocks, B, T, seed, lambda_future, lambda_latent): phase 2's cases (tests/golden/make_golden_train_ar.py), then
# the weight-decay case at lambda = 0
CASES = ((64, 2, 3, 5, 11, 1.0, 1.0), (128, 2, 2, 40, 12, 1.0, 1.0), (256, 2, 8, 2, 13, 0.5, 0.5), (64, 2, 3, 5, 14, 0.0, 0.0))


def head_len(numel: int) -> int:
    return min(64, int(numel))


def _heads(tensors):
    """(len(tensors), 64) fp32: row i = the first 64 entries of tensors[i], NaN past its end."""
    out = torch.full((len(tensors), 64), float("nan"))
    for i, t in enumerate(tensors):
        out[i, : head_len(t.numel())] = t.reshape(-1)[:64]
    return out


def main():
    tv = types.ModuleType("torchvision"); tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"] = tv; sys.modules["torchvision.models"] = tv.models
    sys.path.insert(0, REF_SRC)
    import model as ref_model
    from oracle.lifting_oracle import synthetic_head_state_dict
    out = {"trainable": None, "cases": []}
    for latent, blocks, b, t, seed, lam_f, lam_l in CASES:
        m = ref_model.PHDFor3DJoints(latent_dim=latent, joints_num=17, number_blocks=blocks).eval()
        m.load_state_dict(synthetic_head_state_dict(latent, blocks, seed), strict=True)
        for p in m.parameters():
            p.requires_grad = True
        names = [k for k, _ in m.named_parameters()]
        assert out["trainable"] in (None, names)
        out["trainable"] = names
        out["head_len"] = [head_len(p.numel()) for p in m.parameters()]
        optim = torch.optim.AdamW(m.parameters(), lr=LR, weight_decay=1e-2)
        case = {"latent_dim": latent, "number_blocks": blocks, "seed": seed, "b": b, "t": t, "lr": LR, "lambda_future": lam_f,
                "lambda_latent": lam_l, "losses": []}
        for s, (feats, gt) in enumerate(batches_for(seed, b, t)):
            optim.zero_grad(set_to_none=True)
            phi, phi_hat, joints_phi, joints_hat = m(feats, predict_future=True)
            l3d = (joints_phi - gt).pow(2).mean()
            l3d_hat = (joints_hat[:, 1:] - gt[:, 1:]).pow(2).mean()
            l_lat = (phi_hat[:, 1:] - phi[:, 1:].detach()).pow(2).mean()
            loss = l3d + lam_f * l3d_hat + lam_l * l_lat
            loss.backward()
            if s == 0:                                  # row i: trainable[i]
                assert all(p.grad is not None for p in m.parameters())
                case["grad_norm"] = [float(p.grad.norm()) for p in m.parameters()]
                case["grad_head"] = _heads([p.grad for p in m.parameters()])
            optim.step()
            case["losses"].append([float(loss.detach()), float(l3d.detach()), float(l3d_hat.detach()), float(l_lat.detach())])
        case["param_norm"] = [float(p.detach().norm()) for p in m.parameters()]
        case["param_head"] = _heads([p.detach() for p in m.parameters()])
        print(latent, blocks, b, t, lam_f, lam_l, "losses", case["losses"])
        out["cases"].append(case)
    torch.save(out, os.path.join(HERE, "train_joint_golden.pt"))


if __name__ == "__main__":
    main()
