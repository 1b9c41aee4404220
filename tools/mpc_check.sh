cd $GRAFT_REPO_ROOT && mkdir -p gpurun_out && timeout -k 10 300 python -u -m pytest tests/test_tracking.py tests/test_gpu_workloads.py -m gpu -k "tracking or mpc or cfg5 or fused or p_inf" -x -v -p no:cacheprovider --tb=short --timeout 120 --timeout-method thread > gpurun_out/mpc_tests.log 2>&1; rc=$?; tail -25 gpurun_out/mpc_tests.log; [ $rc -le 1 ] || exit $rc
LOGS=${BENCH_LOGS:-bench_logs}; mkdir -p "$LOGS"
timeout -k 10 200 python -u bench.py --workload mpc --steps 20 --warmup 3 --full > "$LOGS/bench_mpc.log" 2>&1; tail -1 "$LOGS/bench_mpc.log"
