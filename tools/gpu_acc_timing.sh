# k_accumulate timing: bench HIP events vs rocprofv3 kernel trace of the same default run
set -o pipefail
export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest tests/test_msm_gpu.py -x -q -p no:cacheprovider --timeout 200 > gpurun_out/m.log 2>&1 || { echo TESTS_FAILED; tail -20 gpurun_out/m.log; exit 1; }
tail -1 gpurun_out/m.log
O=${OUT:-$(mktemp -d)}  # the trace and the bench log
rm -rf $O/pchk
timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d $O/pchk -o run -- python3 bench.py --full --no-cpu-baseline > $O/pchk.log 2>&1 || { echo PROF_FAILED; tail -20 $O/pchk.log; exit 1; }
python3 tools/acc_timing_check.py $O/pchk/run_kernel_trace.csv $O/pchk.log
