#!/bin/bash
# MFMA-pipe utilisation per kernel class of a bench step from PMC counters (run on the GPU box), kernel-trace only; full-batch launches only.
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
OUT="${OUT:-prof_out}"; mkdir -p "$OUT"     # every output of this script goes under $OUT
rm -rf $OUT/pmcb_MFMA
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_MFMA --output-format csv -d $OUT/pmcb_MFMA -- python3 bench.py --full --lanes 1 --steps 3 --warmup 1 --no-cpu-baseline --no-secondary --preheat 0 --no-check > $OUT/pmcb_MFMA.log 2>&1 || echo "pass failed"
python3 scripts/pmc_bench_mfma_summary.py --dir "$OUT" --forwards 7 > $OUT/pmc_mfma_util.json
