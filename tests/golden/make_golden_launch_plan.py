"""Records tests/golden/backbone_launch_plan.json on an MI355X: what the backbone launches for every option set of
tests/test_launch_plan_gpu.py, and which sets give the same feature bits.

    python tests/golden/make_golden_launch_plan.py                      # write the golden
    python tests/golden/make_golden_launch_plan.py --dump-features F    # also keep one feature tensor per group of equal bits in F
    python tests/golden/make_golden_launch_plan.py --compare-features F --no-write
                                                                        # another build: every set must give the bits kept in F

The golden pins the launch sequence of the commit it was recorded on.  Re-record it only with a change that is MEANT to launch
something else, and say so in that change.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import test_launch_plan_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump-features")
    ap.add_argument("--compare-features")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    from implementation_phd_lab_vision_amd import _lib
    _lib.build_library()
    kept = torch.load(args.compare_features) if args.compare_features else None
    golden = {"frames": T.FRAMES, "frames_streams": T.FRAMES_STREAMS, "frame_seed": T.FRAME_SEED, "plans": {}, "partitions": {}}
    dump, differ = {}, []
    for precision in T.ALL:
        plans, _rows, groups = T.measure(precision)
        golden["plans"][precision] = plans
        golden["partitions"][precision] = {v: [names for _rep, names in gs] for v, gs in groups.items()}
        dump[precision] = {v: [(rep.cpu(), names) for rep, names in gs] for v, gs in groups.items()}
        print(f"{precision}: {len(plans)} option sets, groups of equal bits per variant: "
              f"{ {v: len(gs) for v, gs in groups.items()} }", flush=True)
        if kept is not None:
            for v, gs in groups.items():
                then = {n: rep for rep, names in kept[precision][v] for n in names}
                for rep, names in gs:
                    differ += [(precision, v, n) for n in names if not torch.equal(rep.cpu(), then[n])]
    golden["taps"] = {t: fp for t, (fp, _rows) in T.measure_taps().items()}
    if kept is not None:
        n_sets = sum(len(names) for p in dump.values() for gs in p.values() for _rep, names in gs)
        print(f"features compared with {args.compare_features}: {n_sets - len(differ)} of {n_sets} (set, variant) pairs bit-identical")
        for d in differ:
            print("  DIFFERS:", d)
    if args.dump_features:
        torch.save(dump, args.dump_features)
    if not args.no_write:
        T.GOLDEN.write_text(json.dumps(golden, indent=1, sort_keys=True) + "\n")
        print(f"wrote {T.GOLDEN}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
