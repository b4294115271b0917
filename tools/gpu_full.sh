#!/bin/bash
# the whole GPU test tier, smoke, then the bench line with --full
# tools/gpu_full.sh [output dir, default a new temporary one]
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${1:-$(mktemp -d)}; mkdir -p "$OUT"; echo "outputs in $OUT"
python -m pytest tests/ -x -q -m gpu 2>&1 | tail -4 > "$OUT/full_tests.log"; cat "$OUT/full_tests.log"
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
python bench.py --full > "$OUT/full_bench.json" 2> "$OUT/full_bench.err"; cut -c1-6000 "$OUT/full_bench.json"
