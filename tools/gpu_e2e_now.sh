#!/bin/bash
# CLI / renderer parity tests, then the bench line's regions (--full, end to end included)
cd "$GRAFT_REPO_ROOT" || exit 1
python -m pytest tests/test_gpu_parity.py tests/test_gpu_multigpu.py -q -m gpu -x -k "cli or config2 or shard or driver or golden or demo" 2>&1 | grep -v amdgpu.ids | tail -3
python bench.py --full --no-cpu-baseline --no-gather 2>/tmp/bench_err.log | tee /tmp/bench_e2e_now.json | python -c "
import json,sys
d=json.loads(sys.stdin.readline())
print(d['value'], d['ms_per_step'])
e=d.get('end_to_end'); print(e['value'], e['median_value'], e['stage_s'], e['region_s_all_runs'])"
