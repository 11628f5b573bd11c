#!/bin/bash
# Round artifacts: bench line (--full: with the CPU leg), rocprofv3 kernel trace stats, PMC passes -> pmc_traffic.json, f64 / sync
# microbenchmarks.  Usage: gpu_profile_round.sh r02f <output dir>     (copy <output dir>/* into profiles/ afterwards)
TAG=${1:-rXX}
OUT=$(realpath -m "${2:?usage: gpu_profile_round.sh <tag> <output dir>}")
mkdir -p $OUT
export TMPDIR=/tmp
REPO=${GRAFT_REPO_ROOT:-/root/repo}
cd $REPO
timeout 900 python bench.py --full 2>$OUT/bench.err | grep "^{" > $OUT/bench.json
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/trace -o bench -- python $REPO/bench.py --steps 10 --warmup 2 --no-cpu 2>/dev/null | grep "^{" > $OUT/bench_under_rocprof.json
for C in FETCH_SIZE WRITE_SIZE "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE" ; do
  tag=$(echo $C | tr ' ' '_' | cut -c1-24)
  timeout 300 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $OUT/pmc/$tag -o p -- python $REPO/bench.py --steps 3 --warmup 1 --no-cpu > /dev/null 2>&1
done
cd $REPO
python tools/rocpd_stats.py $OUT/trace/bench_results.db > $OUT/kernel_stats.csv
python tools/pmc_summary.py $OUT/pmc > $OUT/pmc_summary.csv
python tools/make_pmc_traffic.py $OUT/pmc_summary.csv $TAG && cp profiles/pmc_traffic.json $OUT/pmc_traffic.json
rm -rf $OUT/trace $OUT/pmc
timeout 120 tools/bin/ubench_f64 > $OUT/ubench_f64.txt 2>&1
head -10 $OUT/kernel_stats.csv; head -4 $OUT/pmc_summary.csv | cut -c1-160; cut -c1-600 $OUT/bench.json; cat $OUT/ubench_f64.txt
