"""The launch sequence of every head-training step kind (implementation_phd_lab_vision_amd/trainable.py and the three heads built on
it) against tests/golden/train_launch_sequences.json: the ordered ``what`` strings that one eager ``forward_backward`` passes to
``_lib.check``, for phase 1, phase 1 + geo, phase 2 teacher, phase 2 rollout, joint, joint + geo (eval mode, dropout off) and phase 1
with masks given, on PHD(64, 17, 1) heads at B 2, T 4 (rollout: I 2, k 2), fp16.  An added, dropped or reordered launch shows here;
the reference-parity tests cannot see one.  Also each head's ``_layout`` against the fixture's."""
import json

import pytest
import torch

from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = GOLDEN / "train_launch_sequences.json"
DIMS, B, T, INPUT_LEN, K_STEPS = (64, 17, 1), 2, 4, 2, 2
STEP_KINDS = ("phase1", "phase1_geo", "phase2_teacher", "phase2_rollout", "joint", "joint_geo", "phase1_masks")


def head_class(kind):
    from implementation_phd_lab_vision_amd import train, train_ar, train_joint
    return {"phase1": train.TrainableHead, "phase2": train_ar.ARTrainableHead, "joint": train_joint.JointTrainableHead}[kind]


def make_head(kind, dims=DIMS):
    from oracle import lifting_oracle as lo
    d, j, nb = dims
    h = head_class(kind)(d, j, nb, precision="fp16")
    h.load_state_dict(lo.synthetic_head_state_dict(d, nb, 3))
    return h.to(DEV)


def batch():
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(B, T, 2048, generator=g).abs()
    gt = torch.randn(B, T, 17, 3, generator=g) * 0.3
    gt[..., 2] += 5.0                                                    # in front of the camera
    k = torch.tensor([[1000.0, 0.0, 500.0], [0.0, 1000.0, 500.0], [0.0, 0.0, 1.0]])
    gt2d = torch.randn(B, T, 17, 2, generator=g) * 50.0 + 500.0
    return feats.to(DEV), gt.to(DEV), gt2d.to(DEV), k.to(DEV)


def record_step(step_kind, monkeypatch_setattr):
    """The ``what`` strings of one eager ``forward_backward`` of ``step_kind``, in launch order."""
    from implementation_phd_lab_vision_amd import _lib
    from implementation_phd_lab_vision_amd.train import GeoWeights
    head = make_head(step_kind.split("_")[0])
    head.train(False)
    feats, gt, gt2d, k = batch()
    geo = GeoWeights() if step_kind.endswith("_geo") else None
    masks = head.make_dropout_masks(B, T, generator=torch.Generator(device=DEV).manual_seed(5)) if step_kind.endswith("_masks") else None
    calls = []
    real = _lib.check

    def check(rc, handle=None, what=""):
        calls.append(what)
        return real(rc, handle, what)

    monkeypatch_setattr(_lib, "check", check)
    try:
        if step_kind == "phase2_rollout":
            head.rollout_forward_backward(feats, gt, INPUT_LEN, K_STEPS, 1024.0)
        elif step_kind == "phase2_teacher":
            head.forward_backward(feats, gt, 1024.0)
        else:
            head.forward_backward(feats, gt, 1024.0, masks, gt2d if geo else None, k if geo else None, geo)
        torch.cuda.synchronize()
    finally:
        monkeypatch_setattr(_lib, "check", real)
    return calls


@pytest.fixture(scope="module")
def fixture():
    return json.loads(FIXTURE.read_text())


@pytest.mark.parametrize("step_kind", STEP_KINDS)
def test_launch_sequence(step_kind, fixture, monkeypatch, lib_built):
    got = record_step(step_kind, monkeypatch.setattr)
    want = fixture["sequences"][step_kind]
    assert len(want) > 40
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w)


@pytest.mark.parametrize("kind", ("phase1", "phase2", "joint"))
def test_uploaded_layout(kind, fixture, lib_built):
    head = make_head(kind)
    assert [[n, o, list(s)] for n, o, s in head._layout] == fixture["layouts"][kind]["64,17,1"]
