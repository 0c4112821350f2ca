"""The geometric pose losses (2D reprojection, velocity, bone length) without a GPU: the tests' fp64
restatement (tests/geo_reference.py) against what the reference's own functions computed (tests/golden/geo_golden.pt), the package's
skeleton against the reference's, ``train_geo``'s parser per stage, and the argument refusals of ``r50_op_geo_pose_loss_grad``."""
import ctypes as C
import math

import pytest
import torch

from tests import geo_reference as gr
from tests.golden.make_golden_geo import JOINT_CASES, LAMBDAS, OP_CASES, STEP_CASES, geo_batches_for, geo_state_dict
from tests.helpers import GOLDEN

from implementation_phd_lab_vision_amd import train, train_geo, train_joint


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLDEN / "geo_golden.pt", map_location="cpu", weights_only=True)


def _edges(gold):
    return [tuple(e) for e in gold["edges"]]


def test_edge_constant_equals_reference(gold):
    assert [list(e) for e in train.H36M_EDGES] == gold["edges"]
    assert len(train.H36M_EDGES) == 16 and {j for e in train.H36M_EDGES for j in e} == set(range(17))     # a tree over the 17 joints
    assert train.GEO_EPS == gold["eps"] == 1e-6


def test_restatement_reproduces_op_fixture(gold):
    """Every op-level value of the fixture (the reference's functions, fp64) to 1e-12 relative: the terms relative to their own value,
    the gradient relative to its largest entry.  The inputs keep every element away from the clamp and from a zero-length bone (or
    exactly on it), which is asserted here from the fp64 values: the mask of elements to leave out is empty."""
    edges = _edges(gold)
    assert [(c["name"], c["b"], c["t"]) for c in gold["op"]] == list(OP_CASES)
    for c in gold["op"]:
        pred, g3d, g2d, k = c["pred"], c["joints3d"], c["joints2d"], c["K"]
        z = torch.einsum("bij,btnj->btni", k.double(), pred.double())[..., 2]
        bl = gr.bone_lengths(pred.double(), edges)
        near = ((z > -0.1) & (z < 1.0)).sum() + ((bl > 0) & (bl < 1e-2)).sum()
        assert int(near) == 0, c["name"]
        assert int((z < 1e-6).sum()) == (3 if c["name"] == "behind" else 0) and int((bl == 0).sum()) == (2 if c["name"] == "zero_bone" else 0)
        for st in c["sets"]:
            out8, grad = gr.geo_loss_grad(pred, g3d, g2d, k, edges, tuple(st["lambdas"]))
            got = dict(zip(gr.OUT8, out8.tolist()))
            for name in ("loss", "l3d", "l2d", "l_vel", "l_bone"):
                assert got[name] == pytest.approx(st[name], rel=1e-12, abs=0), (c["name"], st["lambdas"], name)
            assert bool(torch.isfinite(grad).all())
            assert float((grad - st["grad"]).abs().max()) <= 1e-12 * float(st["grad"].abs().max()), (c["name"], st["lambdas"])
            assert got["n_clamped"] == (3 if c["name"] == "behind" else 0)
    zb = next(c for c in gold["op"] if c["name"] == "zero_bone")          # the zero-length bone: gradient 0 from that bone, not NaN
    _, g_bone = gr.geo_loss_grad(zb["pred"], zb["joints3d"], zb["joints2d"], zb["K"], [(4, 5)], (0.0, 0.0, 1.0))
    _, g_none = gr.geo_loss_grad(zb["pred"], zb["joints3d"], zb["joints2d"], zb["K"], [], (0.0, 0.0, 0.0))
    assert torch.equal(g_bone[0, 1, 4:6], g_none[0, 1, 4:6]) and not torch.equal(g_bone[0, 0, 4:6], g_none[0, 0, 4:6])


def test_behind_camera_gradient_goes_through_the_numerator(gold):
    """Below the clamp the denominator is eps and carries no gradient; the numerator still does: ~cx * Z / eps pixels."""
    c = next(c for c in gold["op"] if c["name"] == "behind")
    st = c["sets"][0]
    assert st["lambdas"][1:] == [0.0, 0.0] and st["l2d"] > 1e12
    g = st["grad"][0, 0, 3]
    assert float(g.abs().max()) > 1e6 and bool(torch.isfinite(g).all())


def test_s0_leaves_frame_0_out(gold):
    """s0 = 1 is the loss over pred[:, 1:]: frame 0 gets gradient 0 and the means are those of the sliced clips."""
    edges = _edges(gold)
    c = gold["op"][0]
    out1, grad1 = gr.geo_loss_grad(c["pred"], c["joints3d"], c["joints2d"], c["K"], edges, LAMBDAS, s0=1)
    out0, grad0 = gr.geo_loss_grad(c["pred"][:, 1:], c["joints3d"][:, 1:], c["joints2d"][:, 1:], c["K"], edges, LAMBDAS)
    assert torch.equal(out1, out0) and torch.equal(grad1[:, 1:], grad0) and not bool(grad1[:, 0].any())


def _check_steps(case, losses, grads, final, sd):
    """tests/test_train_joint_cpu.py::test_restatement_reproduces_fixture's bars, on every trainable parameter."""
    for s in range(2):
        torch.testing.assert_close(torch.tensor(losses[s]), torch.tensor(case["losses"][s]), rtol=1e-5, atol=0)
    for i, n in enumerate(case["trainable"]):
        k = case["head_len"][i]
        assert float(grads[n].norm()) == pytest.approx(case["grad_norm"][i], rel=1e-4), n
        torch.testing.assert_close(grads[n].reshape(-1)[:k], case["grad_head"][i][:k], rtol=1e-3, atol=1e-4 * case["grad_norm"][i] / 64 ** 0.5)
        torch.testing.assert_close(final[n].reshape(-1)[:k], case["param_head"][i][:k], rtol=0, atol=0.02 * case["lr"])
        assert bool(case["grad_head"][i][k:].isnan().all())
    assert torch.equal(final["f_3D.y0"], sd["f_3D.y0"])


def test_restatement_reproduces_step_fixture(gold):
    edges = _edges(gold)
    assert len(gold["steps"]) == len(STEP_CASES) and len(gold["joint_steps"]) == len(JOINT_CASES)
    for c in gold["steps"]:
        assert c["trainable"] == train.trainable_names(c["number_blocks"]) and tuple(c["lambdas"]) == LAMBDAS
        sd = geo_state_dict(c["latent_dim"], c["number_blocks"], c["seed"])
        losses, grads, final = gr.geo_steps_reference(sd, c["trainable"], geo_batches_for(c["seed"], c["b"], c["t"]), edges, LAMBDAS,
                                                      lr=c["lr"])
        _check_steps(c, losses, grads, final, sd)
    for c in gold["joint_steps"]:
        assert c["trainable"] == train_joint.joint_trainable_names(c["number_blocks"])
        sd = geo_state_dict(c["latent_dim"], c["number_blocks"], c["seed"])
        losses, grads, final = gr.geo_steps_reference(sd, c["trainable"], geo_batches_for(c["seed"], c["b"], c["t"]), edges, LAMBDAS,
                                                      joint=(c["lambda_future"], c["lambda_latent"]), lr=c["lr"])
        _check_steps(c, losses, grads, final, sd)


def test_geo_weights():
    g = train.GeoWeights()
    assert g.as_tuple() == (1e-6, 1.0, 1.0)                    # the reference's --lambda-2d default and train()'s signature
    with pytest.raises(Exception):
        g.lambda_2d = 1.0                                       # frozen
    for bad in ((-1e-9, 1, 1), (0, float("nan"), 1), (0, 1, float("inf")), (0, -1, 0)):
        with pytest.raises(ValueError):
            train.GeoWeights(*bad)
    assert train.expand_intrinsics(torch.eye(3), 4).shape == (4, 3, 3)
    with pytest.raises(ValueError, match="per-frame"):
        train.expand_intrinsics(torch.zeros(4, 5, 3, 3), 4)
    with pytest.raises(ValueError):
        train.expand_intrinsics(torch.zeros(3, 3, 3), 4)


def test_parsers(tmp_path):
    p1 = vars(train.build_parser().parse_args([]))
    # train.build_parser() is unchanged: the reference's flags plus this project's four
    assert set(p1) == {"train", "val", "seq_len", "batch_size", "lr", "epochs", "num_workers", "lambda_2d", "outdir", "resume", "log_every",
                       "early_stop_patience", "early_stop_min_delta", "precision", "seed", "train_subjects", "val_subjects"}
    assert p1["lambda_2d"] == 1e-6 and p1["outdir"] == "./runs/phase1"
    new = {"stage", "lambda_vel", "lambda_bone", "warmup_2d_epochs"}
    a = vars(train_geo.parse_args([]))
    assert set(a) == set(p1) | new
    assert {k: v for k, v in a.items() if k not in new | {"outdir"}} == {k: v for k, v in p1.items() if k != "outdir"}
    assert (a["stage"], a["lambda_vel"], a["lambda_bone"], a["warmup_2d_epochs"], a["outdir"]) == ("phase1", 1.0, 1.0, 1, "./runs/geo")
    pj = vars(train_joint.parse_args(["--init", "x.pt"]))
    j = vars(train_geo.parse_args(["--stage", "joint", "--init", "x.pt"]))
    assert set(j) == set(pj) | new and j["stage"] == "joint"
    assert {k: v for k, v in j.items() if k not in new | {"outdir"}} == {k: v for k, v in pj.items() if k != "outdir"}
    got = train_geo.parse_args(["--lambda-2d", "1e-4", "--lambda-vel", "0", "--lambda-bone", "2.5", "--warmup-2d-epochs", "3", "--precision", "bf16"])
    assert (got.lambda_2d, got.lambda_vel, got.lambda_bone, got.warmup_2d_epochs, got.precision) == (1e-4, 0.0, 2.5, 3, "bf16")
    w = train_geo.geo_schedule(got)
    assert w(2) == train.GeoWeights(0.0, 0.0, 2.5) and w(3) == train.GeoWeights(1e-4, 0.0, 2.5)
    for bad in (["--lambda-2d", "-1"], ["--lambda-vel", "-1e-9"], ["--lambda-bone", "nan"], ["--lambda-2d", "nan"], ["--lambda-vel", "inf"],
                ["--warmup-2d-epochs", "-1"], ["--stage", "phase2"], ["--stage", "joint"], ["--init", "x.pt"],
                ["--stage", "joint", "--init", "x.pt", "--lambda-future", "-1"],
                ["--stage", "joint", "--resume", str(tmp_path / "missing.pt")]):
        with pytest.raises(SystemExit):
            train_geo.parse_args(bad)
    assert "no run has measured" in train_geo.build_parser().format_help() or "nobody has measured" in train_geo.build_parser().format_help()
    assert "train_geo" in train.build_parser().format_help()


def test_abi_argument_errors_need_no_gpu(lib_built):
    lib = lib_built
    p = C.c_void_p(4096)                       # never dereferenced: every call below is refused before any launch
    f = lib.r50_op_geo_pose_loss_grad
    flat = [v for e in train.H36M_EDGES for v in e]
    ok = dict(y=p, g3=p, g2=p, k=p, b=2, t=5, s0=0, j=17, edges=flat, l2=1e-6, lv=1.0, lb=1.0, eps=1e-6, dy=p, part=p, out=p)

    def call(**change):
        a = {**ok, **change}
        ed = (C.c_int * max(len(a["edges"]), 1))(*a["edges"]) if a["edges"] is not None else None
        return f(a["y"], a["g3"], a["g2"], a["k"], a["b"], a["t"], a["s0"], a["j"], ed, len(a["edges"] or ()) // 2 if "ne" not in a else a["ne"],
                 a["l2"], a["lv"], a["lb"], a["eps"], 1.0, 1.0, a["dy"], a["part"], a["out"], None)

    bad = [(dict(y=None), b"null"), (dict(g3=None), b"null"), (dict(g2=None), b"null"), (dict(k=None), b"null"), (dict(part=None), b"null"),
           (dict(out=None), b"null"), (dict(b=0), b"b >= 1"), (dict(s0=2), b"s0"), (dict(s0=-1), b"s0"), (dict(t=0), b"t - s0 >= 1"),
           (dict(t=1, s0=1), b"t - s0 >= 1"), (dict(t=1), b"t - s0 >= 2"), (dict(t=2, s0=1), b"t - s0 >= 2"), (dict(j=0), b"joints"),
           (dict(j=65), b"joints <= 64"), (dict(ne=65), b"n_edges"), (dict(ne=-1), b"n_edges"), (dict(edges=None, ne=3), b"edges_host"),
           (dict(edges=[0, 17]), b"edge index"), (dict(edges=[-1, 2]), b"edge index"), (dict(l2=-1.0), b"lambdas"),
           (dict(lv=float("nan")), b"lambdas"), (dict(lb=float("inf")), b"lambdas"), (dict(eps=0.0), b"eps > 0"),
           (dict(eps=float("nan")), b"eps > 0"), (dict(t=272), b"4608"), (dict(j=64, t=73), b"4608")]
    for change, word in bad:
        assert call(**change) == -1, change
        msg = lib.r50_last_error(None)
        assert b"r50_op_geo_pose_loss_grad" in msg and word in msg, (change, msg)
    assert math.isclose(1e-6, train.GEO_EPS)
