#!/bin/bash
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$R"
OUT=${OUT:-$(mktemp -d)}
python bench.py --full --config 4 --steps 10 --warmup 3 --windows 1 --no-cpu-baseline --no-dropin --no-h2d > "$OUT/bench_c4.json" 2> "$OUT/bench_c4.err"
python - "$OUT/bench_c4.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["config"]["rois_per_step_rank0"], d["config"]["boxes_pre_area_filter_rank0"], d["config"]["roi_longer_side_px"], d["config"]["detector"])
print({k: round(v * 1000, 1) for k, v in d["roofline"]["kernels_ms"].items()})
PY
