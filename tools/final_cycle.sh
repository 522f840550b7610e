#!/bin/bash
# final_cycle.sh TAG -- what a tree is measured by before its numbers go into the documents, in ONE gpurun call (one box): the GPU
# suite, the profile round (tools/profile_round.sh: rocprofv3 --kernel-trace --stats + the PMC passes) turned into the files under
# profiles/ (tools/profile_commit.sh: fresh traffic_cfg4_*.json, stamped with the kernel sources' hashes), then bench.py --full.
#   bash tools/final_cycle.sh TAG [OUTDIR]      (the suite's log, its parity table and the bench line land in OUTDIR/TAG; default out/)
TAG=$1; OUT=${2:-out}/$TAG; mkdir -p "$OUT"
BYOLO_PARITY_TABLE="$OUT/parity_table.json" timeout 1800 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu.log" 2>&1; tail -3 "$OUT/pytest_gpu.log"
bash tools/profile_round.sh $TAG > "$OUT/profile_round.log" 2>&1
bash tools/profile_commit.sh $TAG > "$OUT/profile_commit.log" 2>&1
timeout 900 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"; tail -c 300 "$OUT/bench_default.json"
