for t in 262144 786432 2097152 6291456; do
T=$(mktemp -d); export T; trap 'rm -rf "$T"' EXIT   # scratch bench line (bench.py --full)
  RT_TAIL_PATHS=$t timeout 900 python bench.py --full --workload c4 --no-cpu-baseline --no-extra --steps 2 --warmup 1 > "$T"/bench.json 2>"$T"/bench.err
  python - $t <<'PY'
import json,os,sys
d=json.load(open(os.environ['T'] + '/bench.json')); r=d['roofline']; k=r['kernels']['k_shade']
print('c4 tail_paths %s Mrays/s %.0f ms %.2f trace %.2f shade %.2f launches %d'%(sys.argv[1],d['value'],d['ms_per_step'],r['avg_launch_ms']*r['launches_per_step'],k['avg_launch_ms']*k['launches_per_step'],r['launches_per_step']))
PY
done
