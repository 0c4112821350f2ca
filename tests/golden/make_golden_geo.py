"""Golden values of the geometric pose losses: what the REFERENCE's own ``project_with_K_torch``
(src/train.py:84-110) and ``bone_length_loss`` (:50-57, over its ``H36M_EDGES`` :29-35) compute, in fp64 under autograd on the CPU.
``import train`` from the reference checkout works with ``torchvision`` (unused here) replaced by an empty stub.  The velocity term
has only a parameter name upstream; it is this project's definition and is written out below.

    uv     = project_with_K_torch(pred, K)
    l3d    = (pred - joints3d).pow(2).mean()
    l2d    = (uv - joints2d).pow(2).mean()
    l_vel  = ((pred[:, 1:] - pred[:, :-1]) - (joints3d[:, 1:] - joints3d[:, :-1])).pow(2).mean()
    l_bone = bone_length_loss(pred, joints3d)
    loss   = l3d + lambda_2d * l2d + lambda_vel * l_vel + lambda_bone * l_bone

Op level ("op"): per case the fp32 inputs (pred, joints3d, joints2d, K (B,3,3)) and, per set of weights, the fp64 terms and
d loss / d pred.  Every joint's (K P)[2] is >= 1 or <= -0.1 and every predicted bone is exactly 0 or >= 1e-2, so fp32 and fp64 take
the same branch everywhere (asserted here).  Step level ("steps"): the reference module ``PHDFor3DJoints`` in eval mode, f_AR
frozen as src/train.py:375-376 does, two ``AdamW(lr 1e-4, wd 1e-2)`` steps under the composite loss at phase 1's two small cases,
stored as tests/golden/train_joint_golden.pt stores its cases (per step [loss, l3d, l2d, l_vel, l_bone]).  "joint_steps": the same
with every parameter trainable and ``predict_future=True`` under
``geo(joints_phi) + lambda_future * geo(joints_hat[:, 1:]) + lambda_latent * l_lat`` (geo = the composite above; per step [loss,
the four terms of joints_phi, the four of joints_hat[:, 1:], l_lat]).  The head's ``f_3D.y0`` has z = 4.5 and its last layer is
scaled down so that it predicts poses in front of the camera, as a head that has trained does (asserted: (K P)[2] >= 1).

    python tests/golden/make_golden_geo.py         # needs the reference sources (H36M_REFERENCE_SRC)
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = os.environ.get("H36M_REFERENCE_SRC", "/root/reference/src")
sys.path.insert(0, ROOT)

LR = 1e-4
LAMBDAS = (1e-4, 0.7, 1.3)          # the "all together" weights; each term alone takes its own and 0 for the others
Y0_Z, OUT_SCALE = 4.5, 0.02
# (name, B, T, what is special)
OP_CASES = (("plain", 3, 5), ("skew", 2, 40), ("row3", 8, 2), ("one_frame", 1, 1), ("behind", 3, 5), ("zero_bone", 3, 5))
STEP_CASES = ((64, 2, 3, 5, 11), (128, 2, 2, 40, 12))        # tests/golden/make_golden_train_head.py's
# (latent_dim, number_blocks, B, T, seed, lambda_future, lambda_latent): tests/golden/make_golden_train_joint.py's with T >= 3 (the
# velocity term of joints_hat[:, 1:] needs two predicted frames)
JOINT_CASES = ((64, 2, 3, 5, 11, 1.0, 1.0), (128, 2, 2, 40, 12, 0.5, 0.5))


def intrinsics(b: int, g: torch.Generator, kind: str = "plain") -> torch.Tensor:
    """One H3.6M-like K per clip (a 1000 x 1000 image cropped and resized to 224): fx, fy ~ 1145, cx, cy ~ 112."""
    k = torch.zeros(b, 3, 3)
    k[:, 0, 0] = 1145.0 + 4.0 * torch.randn(b, generator=g)
    k[:, 1, 1] = 1144.0 + 4.0 * torch.randn(b, generator=g)
    k[:, 0, 2] = 112.0 + 3.0 * torch.randn(b, generator=g)
    k[:, 1, 2] = 112.0 + 3.0 * torch.randn(b, generator=g)
    k[:, 2, 2] = 1.0
    if kind == "skew":
        k[:, 0, 1] = 2.5 * torch.randn(b, generator=g)
    if kind == "row3":
        k[:, 2, 0] = 0.01 * torch.randn(b, generator=g)
        k[:, 2, 1] = 0.01 * torch.randn(b, generator=g)
        k[:, 2, 2] = 1.0 + 0.02 * torch.randn(b, generator=g)
    return k


def poses(b: int, t: int, g: torch.Generator) -> torch.Tensor:
    """(B,T,17,3) camera-frame poses, metres: a root at 4-5 m depth drifting over the clip, joints within ~0.5 m of it."""
    root = torch.cat([torch.rand(b, 1, 1, 2, generator=g) - 0.5, 4.0 + torch.rand(b, 1, 1, 1, generator=g)], dim=-1)
    drift = 0.01 * torch.randn(b, t, 1, 3, generator=g).cumsum(dim=1)
    body = 0.25 * torch.randn(b, 1, 17, 3, generator=g) + 0.02 * torch.randn(b, t, 17, 3, generator=g)
    return root + drift + body


def project64(p: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    ph = torch.einsum("bij,btnj->btni", k.double(), p.double())
    return ph[..., :2] / ph[..., 2:3]


def geo_batches_for(case_seed: int, b: int, t: int):
    """Two (feats, joints3d, joints2d, K) batches of a step-level case: feats as phase 1's fixture draws them, poses at 4-5 m,
    joints2d = their projection plus one pixel of noise."""
    g = torch.Generator().manual_seed(900 + case_seed)
    out = []
    for _ in range(2):
        feats = torch.randn(b, t, 2048, generator=g).abs()
        gt = poses(b, t, g)
        k = intrinsics(b, g)
        j2d = (project64(gt, k) + torch.randn(b, t, 17, 2, generator=g).double()).float()
        out.append((feats, gt, j2d, k))
    return out


def geo_state_dict(latent: int, blocks: int, seed: int):
    """The lifting oracle's synthetic head with y0 moved to z = Y0_Z and the regressor's last layer scaled by OUT_SCALE (its
    synthetic weights move a pose by ~4 m per iteration; scaled, the head predicts within ~0.3 m of y0, in front of the camera)."""
    from oracle.lifting_oracle import synthetic_head_state_dict
    sd = synthetic_head_state_dict(latent, blocks, seed)
    y0 = sd["f_3D.y0"].clone().view(-1, 3)
    y0[:, 2] = Y0_Z
    sd["f_3D.y0"] = y0.view(sd["f_3D.y0"].shape)
    for k in ("f_3D.mlp.5.weight", "f_3D.mlp.5.bias"):
        sd[k] = sd[k] * OUT_SCALE
    return sd


def op_inputs(name: str, b: int, t: int, edges):
    g = torch.Generator().manual_seed(hash_name(name))
    gt = poses(b, t, g)
    k = intrinsics(b, g, name)
    pred = gt + 0.05 * torch.randn(b, t, 17, 3, generator=g)
    j2d = (project64(gt, k) + torch.randn(b, t, 17, 2, generator=g).double()).float()
    if name == "behind":                       # three joints behind the camera (Z = -0.2 .. -0.6), one of them in the last frame
        for (bi, ti, ji), z in zip(((0, 0, 3), (1, 2, 10), (2, t - 1, 16)), (-0.2, -0.4, -0.6)):
            pred[bi, ti, ji, 2] = z
    if name == "zero_bone":                    # joint 5 = joint 4 bit for bit in two frames: edge (4, 5) has predicted length 0
        pred[0, 1, 5] = pred[0, 1, 4]
        pred[2, 4, 5] = pred[2, 4, 4]
    # the inputs leave no element near a branch, in fp32 as in fp64
    z = torch.einsum("bij,btnj->btni", k.double(), pred.double())[..., 2]
    assert bool(((z >= 1.0) | (z <= -0.1)).all()), name
    assert bool((torch.einsum("bij,btnj->btni", k.double(), gt.double())[..., 2] >= 1.0).all()), name
    a = torch.tensor([e[0] for e in edges]); c = torch.tensor([e[1] for e in edges])
    bl = torch.norm(pred[:, :, c].double() - pred[:, :, a].double(), dim=-1)
    assert bool(((bl == 0) | (bl >= 1e-2)).all()), name
    assert int((bl == 0).sum()) == (2 if name == "zero_bone" else 0) and int((z < 1e-6).sum()) == (3 if name == "behind" else 0)
    return pred, gt, j2d, k


def hash_name(name: str) -> int:
    return 7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def lambda_sets(t: int):
    l2, lv, lb = LAMBDAS
    sets = [(l2, 0.0, 0.0), (0.0, lv, 0.0), (0.0, 0.0, lb), (l2, lv, lb)]
    if t == 1:                                 # no velocity pair
        sets = [(l2, 0.0, 0.0), (0.0, 0.0, lb), (l2, 0.0, lb)]
    return sets


def head_len(numel: int) -> int:
    return min(64, int(numel))


def _heads(tensors):
    out = torch.full((len(tensors), 64), float("nan"))
    for i, t in enumerate(tensors):
        out[i, : head_len(t.numel())] = t.reshape(-1)[:64]
    return out


def main():
    tv = types.ModuleType("torchvision"); tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"] = tv; sys.modules["torchvision.models"] = tv.models
    sys.path.insert(0, REF_SRC)
    import train as ref_train
    import model as ref_model
    edges = [tuple(int(v) for v in e) for e in ref_train.H36M_EDGES]
    out = {"edges": [list(e) for e in edges], "eps": 1e-6, "lambdas": list(LAMBDAS), "op": [], "steps": [], "joint_steps": []}

    def composite(pred, gt, j2d, k, lam):
        uv = ref_train.project_with_K_torch(pred, k)
        tm = {"l3d": (pred - gt).pow(2).mean(), "l2d": (uv - j2d).pow(2).mean(), "l_bone": ref_train.bone_length_loss(pred, gt),
              "l_vel": ((pred[:, 1:] - pred[:, :-1]) - (gt[:, 1:] - gt[:, :-1])).pow(2).mean() if pred.shape[1] > 1
              else pred.new_zeros(())}
        loss = tm["l3d"]
        for w, n in zip(lam, ("l2d", "l_vel", "l_bone")):
            if w != 0:
                loss = loss + w * tm[n]
        return loss, tm

    for name, b, t in OP_CASES:
        pred, gt, j2d, k = op_inputs(name, b, t, edges)
        case = {"name": name, "b": b, "t": t, "pred": pred, "joints3d": gt, "joints2d": j2d, "K": k, "sets": []}
        for lam in lambda_sets(t):
            leaf = pred.double().clone().requires_grad_(True)
            loss, tm = composite(leaf, gt.double(), j2d.double(), k.double(), lam)
            (grad,) = torch.autograd.grad(loss, leaf)
            assert bool(torch.isfinite(grad).all())
            case["sets"].append({"lambdas": list(lam), "loss": float(loss.detach()), "l3d": float(tm["l3d"].detach()),
                                 "l2d": float(tm["l2d"].detach()), "l_vel": float(tm["l_vel"].detach()),
                                 "l_bone": float(tm["l_bone"].detach()), "grad": grad})
        print(name, b, t, [(s["lambdas"], s["loss"]) for s in case["sets"]])
        out["op"].append(case)

    for latent, blocks, b, t, seed in STEP_CASES:
        m = ref_model.PHDFor3DJoints(latent_dim=latent, joints_num=17, number_blocks=blocks).eval()
        m.load_state_dict(geo_state_dict(latent, blocks, seed), strict=True)
        for p in m.f_AR.parameters():
            p.requires_grad = False
        names = [n for n, p in m.named_parameters() if p.requires_grad]
        params = [p for p in m.parameters() if p.requires_grad]
        optim = torch.optim.AdamW(params, lr=LR, weight_decay=1e-2)
        case = {"latent_dim": latent, "number_blocks": blocks, "seed": seed, "b": b, "t": t, "lr": LR, "lambdas": list(LAMBDAS),
                "trainable": names, "head_len": [head_len(p.numel()) for p in params], "losses": []}
        for s, (feats, gt, j2d, k) in enumerate(geo_batches_for(seed, b, t)):
            optim.zero_grad(set_to_none=True)
            _phi, _phi_hat, joints_pred, _ = m.forward(feats, predict_future=False)
            assert float(torch.einsum("bij,btnj->btni", k, joints_pred.detach())[..., 2].min()) >= 1.0
            loss, tm = composite(joints_pred, gt, j2d, k, LAMBDAS)
            loss.backward()
            if s == 0:
                case["grad_norm"] = [float(p.grad.norm()) for p in params]
                case["grad_head"] = _heads([p.grad for p in params])
            optim.step()
            case["losses"].append([float(loss.detach())] + [float(tm[n].detach()) for n in ("l3d", "l2d", "l_vel", "l_bone")])
        case["param_norm"] = [float(p.detach().norm()) for p in params]
        case["param_head"] = _heads([p.detach() for p in params])
        print(latent, blocks, b, t, "losses", case["losses"])
        out["steps"].append(case)

    for latent, blocks, b, t, seed, lam_f, lam_l in JOINT_CASES:
        m = ref_model.PHDFor3DJoints(latent_dim=latent, joints_num=17, number_blocks=blocks).eval()
        m.load_state_dict(geo_state_dict(latent, blocks, seed), strict=True)
        for p in m.parameters():
            p.requires_grad = True
        names = [n for n, _ in m.named_parameters()]
        params = list(m.parameters())
        optim = torch.optim.AdamW(params, lr=LR, weight_decay=1e-2)
        case = {"latent_dim": latent, "number_blocks": blocks, "seed": seed, "b": b, "t": t, "lr": LR, "lambdas": list(LAMBDAS),
                "lambda_future": lam_f, "lambda_latent": lam_l, "trainable": names, "head_len": [head_len(p.numel()) for p in params],
                "losses": []}
        for s, (feats, gt, j2d, k) in enumerate(geo_batches_for(seed, b, t)):
            optim.zero_grad(set_to_none=True)
            phi, phi_hat, joints_phi, joints_hat = m(feats, predict_future=True)
            for jp in (joints_phi, joints_hat[:, 1:]):
                assert float(torch.einsum("bij,btnj->btni", k, jp.detach())[..., 2].min()) >= 1.0
            c1, tm1 = composite(joints_phi, gt, j2d, k, LAMBDAS)
            c2, tm2 = composite(joints_hat[:, 1:], gt[:, 1:], j2d[:, 1:], k, LAMBDAS)
            l_lat = (phi_hat[:, 1:] - phi[:, 1:].detach()).pow(2).mean()
            loss = c1 + lam_f * c2 + lam_l * l_lat
            loss.backward()
            if s == 0:
                case["grad_norm"] = [float(p.grad.norm()) for p in params]
                case["grad_head"] = _heads([p.grad for p in params])
            optim.step()
            case["losses"].append([float(loss.detach())] + [float(tm1[n].detach()) for n in ("l3d", "l2d", "l_vel", "l_bone")] +
                                  [float(tm2[n].detach()) for n in ("l3d", "l2d", "l_vel", "l_bone")] + [float(l_lat.detach())])
        case["param_norm"] = [float(p.detach().norm()) for p in params]
        case["param_head"] = _heads([p.detach() for p in params])
        print("joint", latent, blocks, b, t, "losses", case["losses"])
        out["joint_steps"].append(case)
    torch.save(out, os.path.join(HERE, "geo_golden.pt"))


if __name__ == "__main__":
    main()
