"""Golden autoregressive rollouts of the lifting head (``PHDFor3DJoints.rollout``): the program this
project defines, run on the REFERENCE module's own submodules (src/model.py, imported from the reference checkout with
``torchvision`` -- unused by the head -- replaced by an empty stub), in eval mode, fp32, on the CPU::

    phi = model.f_movie(model.input_proj(feats[:, :input_len]))
    seq = phi
    for _ in range(pred_len):
        nxt = model.f_AR(seq)[:, -1:]
        seq = torch.cat([seq, nxt], dim=1)
    future = seq[:, input_len:]
    joints = model.f_3D(future)

Per case the fixture keeps the dimensions, the seed of ``synthetic_head_state_dict`` (and of the features,
``tests.rollout_reference.case_feats``: regenerated, not stored, to stay small), the future latents (B, P, D), the future joints
(B, P, 17, 3) and the per-horizon latent norms (mean over clips of ``|future[b, k]|_2``), which show whether a case stays bounded.

    python tests/golden/make_golden_rollout.py          # needs the reference sources (H36M_REFERENCE_SRC)
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = os.environ.get("H36M_REFERENCE_SRC", "/root/reference/src")
sys.path.insert(0, ROOT)

# (latent_dim, number_blocks, B, T, input_len, pred_len, seed).  The third case observes ONE frame: GroupNorm over a single frame
# and the causal conv's replicate padding of a one-frame history.  With these synthetic weights the strips' norm grows LINEARLY
# with the horizon (each step adds f_AR's three residual increments: 15.8 observed -> 21.4 at k = 0 -> 621 at k = 24 in the
# 128-wide case), it does not blow up exponentially, and every value stays far inside fp16's range; so no case is shortened.
CASES = ((64, 2, 3, 14, 5, 7, 21), (128, 2, 2, 40, 15, 25, 22), (256, 2, 4, 6, 1, 3, 23))


def main():
    tv = types.ModuleType("torchvision"); tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"] = tv; sys.modules["torchvision.models"] = tv.models
    sys.path.insert(0, REF_SRC)
    import model as ref_model
    from oracle.lifting_oracle import synthetic_head_state_dict
    from tests.rollout_reference import case_feats
    out = []
    for latent, blocks, b, t, i_len, p_len, seed in CASES:
        m = ref_model.PHDFor3DJoints(latent_dim=latent, joints_num=17, number_blocks=blocks).eval()
        m.load_state_dict(synthetic_head_state_dict(latent, blocks, seed), strict=True)
        feats = case_feats(seed, b, t)
        with torch.no_grad():
            phi = m.f_movie(m.input_proj(feats[:, :i_len]))
            seq = phi
            for _ in range(p_len):
                nxt = m.f_AR(seq)[:, -1:]
                seq = torch.cat([seq, nxt], dim=1)
            future = seq[:, i_len:]
            joints = m.f_3D(future)
        norms = future.norm(dim=-1).mean(0)
        print(latent, blocks, b, t, i_len, p_len, "observed norm", float(phi.norm(dim=-1).mean()), "future norms", norms.tolist())
        out.append({"latent_dim": latent, "number_blocks": blocks, "seed": seed, "b": b, "t": t, "input_len": i_len, "pred_len": p_len,
                    "future_phi": future.clone(), "future_joints": joints.clone(), "future_norms": norms.clone(),
                    "observed_norm": float(phi.norm(dim=-1).mean())})
    torch.save(out, os.path.join(HERE, "rollout_golden.pt"))


if __name__ == "__main__":
    main()
