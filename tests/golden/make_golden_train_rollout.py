"""Golden steps of the rollout objective (training f_AR on its own multi-step rollouts; INTEGRATION.md section K,
implementation_phd_lab_vision_amd/train_ar.py ``rollout_train_step``): the REFERENCE module ``PHDFor3DJoints`` (src/model.py,
imported from the reference checkout with ``torchvision`` -- unused by the head -- replaced by an empty stub), every parameter
frozen but f_AR's, ``torch.optim.AdamW(f_AR parameters, lr, weight_decay=1e-2)``, run for two steps of

    phi_obs = model.f_movie(model.input_proj(feats[:, :I]))          # no gradient
    phi_all = model.f_movie(model.input_proj(feats))                 # no gradient: the teacher
    seq = phi_obs
    for _ in range(k): seq = torch.cat([seq, model.f_AR(seq)[:, -1:]], dim=1)
    fut = seq[:, I:]
    loss = (model.f_3D(fut) - gt[:, I:I + k]).pow(2).mean() + lambda_latent * (fut - phi_all[:, I:I + k]).pow(2).mean()

on the CPU in fp32, in eval mode (dropout is random and not seed-pinned upstream; the f_AR dropout sites are covered by the tests'
restatement with explicit masks).  The fixture has train_ar_golden.pt's layout: the trainable names, per step [loss, l3d, l_lat],
per parameter (row i = trainable[i]) the gradient's norm and first 64 entries after step 1 and the parameter's norm and first 64
entries after step 2; each case also records input_len and k.

    python tests/golden/make_golden_train_rollout.py      # needs the reference sources (H36M_REFERENCE_SRC)
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = os.environ.get("H36M_REFERENCE_SRC", "/root/reference/src")
sys.path.insert(0, ROOT)

LR = 1e-4      # train.py's default (src/config.py LR)
# (latent_dim, number_blocks, B, T, input_len, k, seed, lambda_latent)
# I = 1, k = 1: f_AR sees a single frame, so GroupNorm(32) normalises groups of C/32 values; 256 channels keep those groups at 8 (as
# train_ar_golden.pt's T = 2 case).  The small-D case has k = 3 and no latent term.  The last one is the paper's I = 15, P = 25.
CASES = ((256, 2, 3, 2, 1, 1, 21, 1.0), (64, 2, 3, 7, 4, 3, 22, 0.0), (256, 2, 2, 40, 15, 25, 23, 0.5))


def batches_for(case_seed, b, t):
    g = torch.Generator().manual_seed(800 + case_seed)
    out = []
    for _ in range(2):
        feats = torch.randn(b, t, 2048, generator=g).abs()
        gt = torch.randn(b, t, 17, 3, generator=g) * 0.5
        out.append((feats, gt))
    return out


def main():
    tv = types.ModuleType("torchvision"); tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"] = tv; sys.modules["torchvision.models"] = tv.models
    sys.path.insert(0, REF_SRC)
    import model as ref_model
    from oracle.lifting_oracle import synthetic_head_state_dict
    out = {"trainable": None, "cases": []}
    for latent, blocks, b, t, i_len, k, seed, lam in CASES:
        m = ref_model.PHDFor3DJoints(latent_dim=latent, joints_num=17, number_blocks=blocks).eval()
        m.load_state_dict(synthetic_head_state_dict(latent, blocks, seed), strict=True)
        for p in m.parameters():
            p.requires_grad = False
        for p in m.f_AR.parameters():
            p.requires_grad = True
        names = [n for n, p in m.named_parameters() if p.requires_grad]
        assert out["trainable"] in (None, names)
        out["trainable"] = names
        optim = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=LR, weight_decay=1e-2)
        case = {"latent_dim": latent, "number_blocks": blocks, "seed": seed, "b": b, "t": t, "input_len": i_len, "k": k, "lr": LR,
                "lambda_latent": lam, "losses": []}
        for s, (feats, gt) in enumerate(batches_for(seed, b, t)):
            optim.zero_grad(set_to_none=True)
            with torch.no_grad():
                phi_obs = m.f_movie(m.input_proj(feats[:, :i_len]))
                phi_all = m.f_movie(m.input_proj(feats))
            seq = phi_obs
            for _ in range(k):
                seq = torch.cat([seq, m.f_AR(seq)[:, -1:]], dim=1)
            fut = seq[:, i_len:]
            l3d = (m.f_3D(fut) - gt[:, i_len:i_len + k]).pow(2).mean()
            l_lat = (fut - phi_all[:, i_len:i_len + k]).pow(2).mean()
            loss = l3d + lam * l_lat
            loss.backward()
            if s == 0:                                  # row i: trainable[i]
                case["grad_norm"] = [float(p.grad.norm()) for p in m.parameters() if p.requires_grad]
                case["grad_head"] = torch.stack([p.grad.reshape(-1)[:64].clone() for p in m.parameters() if p.requires_grad])
            optim.step()
            case["losses"].append([float(loss.detach()), float(l3d.detach()), float(l_lat.detach())])
        case["param_norm"] = [float(p.detach().norm()) for p in m.parameters() if p.requires_grad]
        case["param_head"] = torch.stack([p.detach().reshape(-1)[:64].clone() for p in m.parameters() if p.requires_grad])
        print(latent, blocks, b, t, i_len, k, lam, "losses", case["losses"])
        out["cases"].append(case)
    torch.save(out, os.path.join(HERE, "train_rollout_golden.pt"))


if __name__ == "__main__":
    main()
