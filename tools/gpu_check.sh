#!/bin/bash
# On the GPU box: parity tests, then the C2 bench line (no CPU baseline) -> $OUT (default out/)
OUT=${OUT:-out}; export OUT
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -m gpu -x -q > "$OUT"/gputests.log 2>&1; echo "tests rc=$?"; tail -3 "$OUT"/gputests.log
python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline "$@" > "$OUT"/bench_quick.json 2> "$OUT"/bench_quick.err; echo "bench rc=$?"
python - <<'PY'
import json, os
try:
    d=json.load(open(os.environ['OUT'] + '/bench_quick.json'))
    r=d['roofline']
    print(f"Mrays/s {d['value']:.1f}  ms/step {d['ms_per_step']:.1f} dev_ms {d['device_ms_per_step']:.1f} trace_avg_ms {r['avg_launch_ms']:.3f} launches {r['launches_per_step']} frac {r['frac']:.4f} GB/s {r['achieved']:.0f} trace_share {r['trace_share_of_device_time']:.3f} nodes/ray {r['nodes_per_ray']:.2f} tris/ray {r['tris_per_ray']:.2f}")
except Exception as e:
    print("bench parse failed", e); print(open(os.environ['OUT'] + '/bench_quick.err').read()[-2000:])
PY
