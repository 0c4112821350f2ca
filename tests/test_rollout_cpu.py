"""The autoregressive rollout without a GPU: the test-side restatement against the reference module's own
rollouts (tests/golden/rollout_golden.pt), the forecasting metrics' definition on hand-made tensors, and the results CLI's new
flags."""
import pytest
import torch

from implementation_phd_lab_vision_amd import forecast, results
from oracle import lifting_oracle as lo
from tests.helpers import GOLDEN
from tests.rollout_reference import case_feats, horizon_sums, rollout_reference


def test_restatement_equals_reference_module_golden():
    cases = torch.load(GOLDEN / "rollout_golden.pt", map_location="cpu", weights_only=True)
    assert [(c["latent_dim"], c["b"], c["input_len"], c["pred_len"]) for c in cases] == [(64, 3, 5, 7), (128, 2, 15, 25), (256, 4, 1, 3)]
    for c in cases:
        sd = lo.synthetic_head_state_dict(c["latent_dim"], c["number_blocks"], c["seed"])
        phi, joints = rollout_reference(sd, case_feats(c["seed"], c["b"], c["t"]), c["input_len"], c["pred_len"])
        for got, want in ((phi, c["future_phi"]), (joints, c["future_joints"])):
            assert got.shape == want.shape
            torch.testing.assert_close(got, want.double(), rtol=1e-5, atol=1e-5 * float(want.abs().max()))
        assert torch.allclose(phi.norm(dim=-1).mean(0), c["future_norms"].double(), rtol=1e-5)


def test_restatement_reads_only_the_observed_frames():
    sd = lo.synthetic_head_state_dict(64, 2, 3)
    feats = case_feats(3, 2, 9)
    want = rollout_reference(sd, feats, 4, 3)
    feats[:, 4:] = float("nan")
    got = rollout_reference(sd, feats, 4, 3)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_horizon_metrics_definition_on_hand_made_tensors():
    b, t, j, i0, p = 3, 9, 4, 2, 5
    gt = torch.randn(b, t, j, 3, generator=torch.Generator().manual_seed(0))
    off = torch.tensor([3.0, 4.0, 0.0])                         # |off| = 5
    pred = gt[:, i0:i0 + p].clone() + off * torch.arange(1, p + 1, dtype=torch.float32).view(1, p, 1, 1)
    sums = horizon_sums(pred, gt, i0)
    assert sums.shape == (2 * p + 1,) and float(sums[-1]) == b
    m = forecast.metrics_from_sums(sums.tolist(), p, j)
    k = torch.arange(1, p + 1, dtype=torch.float64)
    assert torch.allclose(torch.tensor(m["mpjpe"], dtype=torch.float64), 5.0 * k)          # mean over clips and joints of the distance
    assert torch.allclose(torch.tensor(m["l3d"], dtype=torch.float64), 25.0 * k ** 2 / 3)   # mean over clips, joints and coordinates of the squared error
    assert m["mpjpe_mean"] == pytest.approx(15.0) and m["clips"] == b
    # each clip weighs the same over a pass: batches of 1 and 2 clips add up to the whole, not to a mean of batch means
    pred[0] += 1.0
    parts = horizon_sums(pred[:1], gt[:1], i0) + horizon_sums(pred[1:], gt[1:], i0)
    torch.testing.assert_close(parts, horizon_sums(pred, gt, i0))
    whole = forecast.metrics_from_sums(parts.tolist(), p, j)["mpjpe"]
    batch_means = [(forecast.metrics_from_sums(horizon_sums(pred[s], gt[s], i0).tolist(), p, j)["mpjpe"][0]) for s in (slice(0, 1), slice(1, 3))]
    assert whole[0] != pytest.approx(sum(batch_means) / 2)
    with pytest.raises(ValueError):
        forecast.metrics_from_sums(sums.tolist()[:-1], p, j)
    with pytest.raises(ValueError):
        forecast.metrics_from_sums([0.0] * (2 * p + 1), p, j)


def test_evaluate_rollout_refuses_lengths_beyond_the_store():
    class Store:
        feats = torch.zeros(2, 8, 2048)

        def __len__(self):
            return 2
    for i_len, p_len in ((3, 6), (8, 1), (0, 2), (2, 0)):
        with pytest.raises(ValueError):
            forecast.evaluate_rollout(None, Store(), i_len, p_len)


def _args(*extra):
    return ["--features_root", "F", "--preprocessed_root", "P", "--model_path", "M", *extra]


def test_results_parser_rollout_flags():
    a = results.parse_args(_args())
    assert (a.input_len, a.pred_len) == (15, 0)
    assert results.build_parser().parse_args(_args()).pred_len == 0
    a = results.parse_args(_args("--seq-len", "8", "--input-len", "3", "--pred-len", "5"))
    assert (a.input_len, a.pred_len, a.seq_len) == (3, 5, 8)
    a = results.parse_args(_args("--input-len", "15", "--pred-len", "25"))               # the paper's split of SEQ_LEN = 40
    assert a.input_len + a.pred_len == a.seq_len == 40
    assert results.parse_args(_args("--input-len", "0")).pred_len == 0                   # off: --input-len is not used
    for bad in (("--pred-len", "-1"), ("--seq-len", "8", "--input-len", "3", "--pred-len", "6"),
                ("--input-len", "0", "--pred-len", "5"), ("--pred-len", "x")):
        with pytest.raises(SystemExit):
            results.parse_args(_args(*bad))
