#!/bin/bash
# Throughput vs lanes per GPU (occupancy sweep) -- measurement tool.  Logs go to $BENCH_LOGS (default bench_logs/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 2
LOGS=${BENCH_LOGS:-bench_logs}
mkdir -p "$LOGS"
for b in "$@"; do
  timeout -k 10 300 python3 bench.py --full --steps 1 --warmup 1 --no-cpu --batch $b > "$LOGS/sweep_$b.log" 2>&1
  rc=$?
  python3 - "$b" "$LOGS/sweep_$b.log" <<'PY'
import json, re, sys
b = sys.argv[1]
s = open(sys.argv[2]).read()
m = re.search(r'(\{"metric.*\})', s)
if m:
    d = json.loads(m.group(1))
    k = d.get("kernels", {})
    print(f"batch {b}: value {d['value']/1e6:.2f} M it/s  bwd {k.get('backward',{}).get('avg_ms',0):.3f} ms  trial {k.get('trial',{}).get('avg_ms',0):.3f} ms  iters {d['parity']['outer_iterations']}")
else:
    print(f"batch {b}: no result"); print(s[-2000:])
PY
  if [ $rc -ne 0 ]; then exit $rc; fi
done
