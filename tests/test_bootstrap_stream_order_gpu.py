"""The rows of tests/rows/bootstrap.py late on a side stream, with the harness of tests/stream_order.py: each row
runs once plainly on the default stream and once on the side stream while its unit rows and its stratum table are still stale; snapshot
bits == final bits == plain bits, and the op does not hold the host.  Then the Python entry points: ``bootstrap_sums`` +
``statistics_device`` with late unit rows (no host synchronisation at all), and ``evaluate_bootstrap`` with a late feature store: the
default stream's numbers, and exactly the read-backs it declares -- one per head's pass (``collect_clip_scores``) and one per bootstrap
(``statistics``) --, which hold the host by design.  The store there is opened without ``test_set``: a test-set store also reads every
batch's rows back to look its metas up (``DeviceFeatureStore.get_batch``, as in every report's pass), which is the store's, not the
bootstrap's."""
import numpy as np
import pytest
import torch

from tests.rows.bootstrap import ROWS_BOOTSTRAP, unit_rows
from tests.stream_order import run_row_late, side_against_default

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("row", ROWS_BOOTSTRAP, ids=[r.id for r in ROWS_BOOTSTRAP])
def test_late_on_a_side_stream_bootstrap(row):
    run_row_late(row)


def test_the_wrapper_and_the_statistics_on_a_side_stream():
    from implementation_phd_lab_vision_amd import bootstrap as bs
    table = bs.UnitTable.from_sizes([1, 5, 70])
    table.device_starts(DEV)                                                        # the checked host table goes up once, before either run
    v = np.abs(unit_rows(76, 5, 4)) + 1.0
    v[:, -1] = np.arange(76) % 3 + 1
    point = torch.from_numpy(bs.point_sums(v, table)).to(DEV)
    torch.cuda.synchronize()

    def call(_w, d):
        sums, counts = bs.bootstrap_sums(d["v"], table, 33, 9, r0=1, window=16, counts=True)
        out = {"sums": sums, "counts": counts}
        out.update(bs.statistics_device(sums, point, 0.9, pairs=2))
        return out
    late = side_against_default("bootstrap.bootstrap_sums + statistics_device", call, {"v": torch.from_numpy(v)})
    assert not late.blocked, "bootstrap_sums or statistics_device held the host"


def test_evaluate_bootstrap_on_a_side_stream_reads_back_what_it_declares(tmp_path, monkeypatch):
    from implementation_phd_lab_vision_amd import bootstrap as bs
    from implementation_phd_lab_vision_amd import results
    from implementation_phd_lab_vision_amd.feature_store import DeviceFeatureStore
    from oracle import lifting_oracle as lo
    from tests import results_data as rd
    store = DeviceFeatureStore(str(rd.make_results_cache(tmp_path / "features")), subjects=[9], device=DEV)      # no metas: see the docstring
    head = results.build_head(lo.synthetic_head_state_dict(1024, 2, seed=2), DEV)
    other = results.build_head(lo.synthetic_head_state_dict(1024, 2, seed=3), DEV)
    feats, joints = store.feats.cpu(), store.joints3d.cpu()
    reads, kept = [], {}
    plain_cpu = torch.Tensor.cpu

    def counted(self, *args, **kwargs):
        reads.append(tuple(self.shape))
        return plain_cpu(self, *args, **kwargs)

    def call(late, d):
        store.feats, store.joints3d = d["feats"], d["joints3d"]
        monkeypatch.setattr(torch.Tensor, "cpu", counted)
        try:
            del reads[:]
            res = bs.evaluate_bootstrap(head, store, None, 48, "sequence", 3, 0.9, 4, 3, batch_size=4, compare=other)
            kept["default" if late is None else "side"] = (res, list(reads))
        finally:
            monkeypatch.setattr(torch.Tensor, "cpu", plain_cpu)
        return {name: torch.from_numpy(np.ascontiguousarray(res[name])).to(DEV) for name in ("point", "b_point", "lo", "hi", "diff_lo", "diff_hi",
                                                                                              "p_better", "unit_table")}
    late = side_against_default("bootstrap.evaluate_bootstrap", call, {"feats": feats, "joints3d": joints})
    assert late.blocked, "evaluate_bootstrap reads its passes back: it holds the host by design"
    for which in ("default", "side"):
        res, seen = kept[which]
        # two heads' passes (N clips x 6 scores each) and two bootstraps (the sequence units and the clip units of the design effect)
        assert len(seen) == 4 and seen[0] == seen[1] == (rd.N_S9, 6) and len(seen[2]) == len(seen[3]) == 1, (which, seen)
    assert kept["side"][0]["design_effect"] == kept["default"][0]["design_effect"]
