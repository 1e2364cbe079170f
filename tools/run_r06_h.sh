#!/bin/bash
# the bench as the driver ran it in round 5 (20 timed calls, 5 warm-up calls): wall time of the whole command incl. the live C1 subprocess
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=${1:?usage: $0 OUTPUT_DIR}; mkdir -p "$out"
( time timeout 1500 python bench.py --full --gpus 1 --steps 20 --warmup 5 ) > $out/bench_driverlike.log 2>&1
grep '^{"metric"' $out/bench_driverlike.log > $out/r06_bench_driverlike.json
tail -4 $out/bench_driverlike.log | cut -c1-300
OUT="$out" python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "r06_bench_driverlike.json")).read()); r = d["roofline"]
print(d["value"], d["ms_per_step"], r["frac"], r["dit_frac"], r["attention"]["achieved"], r["frac_of_capped"], d["cpu_baseline"]["value"], d["cpu_baseline"]["c1"]["wall_s_incl_weights_and_warmup"])
PY
