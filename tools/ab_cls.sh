#!/bin/bash
T=$(mktemp -d); export T; trap 'rm -rf "$T"' EXIT   # scratch bench line (bench.py --full)
run() {
  for wl in "$@"; do
    timeout 900 python bench.py --full --workload $wl --no-cpu-baseline --no-extra --steps 3 --warmup 1 > "$T"/bench.json 2>"$T"/bench.err || { echo "FAILED"; tail -3 "$T"/bench.err; continue; }
    python - $wl <<'PY'
import json,os,sys
d=json.load(open(os.environ['T'] + '/bench.json'))
r=d['roofline']; K=r['kernels']
print('   %s Mrays/s %.0f ms %.2f trace %.2f classify %.2f shade %.2f'%(sys.argv[1],d['value'],d['ms_per_step'],K['k_trace']['ms_per_step'],K['k_classify']['ms_per_step'],K['k_shade']['ms_per_step']))
PY
  done
}
WLS="${@:-c4 c3 c2}"
echo "default";              run $WLS
echo "RT_CLS_STREAMS=2";     RT_CLS_STREAMS=2 run $WLS
echo "RT_CLS_STREAMS=3";     RT_CLS_STREAMS=3 run $WLS
echo "default again";        run $WLS
