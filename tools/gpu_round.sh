#!/bin/bash
# One GPU-box pass: gpu parity tests, smoke, bench, rocprof kernel stats.
# Usage (from the repo root): bash tools/gpu_round.sh TAG [tests|bench|prof ...]
# Logs and results go to $GENIE_ROUND_OUT (default round_out/).
set -o pipefail
TAG=${1:-run}; shift
STEPS=${@:-tests smoke bench prof}
OUT=${GENIE_ROUND_OUT:-round_out}
mkdir -p $OUT
export TMPDIR=/tmp
for s in $STEPS; do
  case $s in
    tests) timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1 || { tail -30 $OUT/${TAG}_tests.log; exit 1; }
           tail -3 $OUT/${TAG}_tests.log ;;
    smoke) timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { tail -30 $OUT/${TAG}_smoke.log; exit 1; }
           tail -2 $OUT/${TAG}_smoke.log ;;
    bench) timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -30 $OUT/${TAG}_bench.err; exit 1; }
           cat $OUT/${TAG}_bench.json ;;
    prof)  rm -rf $OUT/prof_${TAG}
           timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o bench -- python3 bench.py > $OUT/${TAG}_bench_under_rocprof.log 2>&1 || { tail -30 $OUT/${TAG}_bench_under_rocprof.log; exit 1; }
           python tools/prof_summary.py $OUT/prof_${TAG} > $OUT/${TAG}_kernel_stats.txt 2>&1; head -25 $OUT/${TAG}_kernel_stats.txt ;;
    batched) for w in batch64 mixed100; do
             timeout -k 10 300 python bench.py --full --workload $w --no-cpu-baseline > $OUT/${TAG}_$w.json 2> $OUT/${TAG}_$w.err || { tail -30 $OUT/${TAG}_$w.err; exit 1; }
             cat $OUT/${TAG}_$w.json
           done ;;
    mfma)  # MFMA busy cycles per kernel (SQ_VALU_MFMA_BUSY_CYCLES; GRBM_GUI_ACTIVE sums the 8 XCDs)
           for w in bench aux; do
             if [ $w = bench ]; then cmd="python3 bench.py --steps 3 --warmup 1"; else cmd="python3 tools/aux_models_bench.py"; fi
             rm -rf $OUT/pmc_${TAG}_mfma_$w
             timeout -s KILL 240 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_${TAG}_mfma_$w -o pmc -- $cmd > $OUT/${TAG}_pmc_mfma_$w.log 2>&1 || { tail -30 $OUT/${TAG}_pmc_mfma_$w.log; exit 1; }
             python tools/mfma_util.py $OUT/pmc_${TAG}_mfma_$w > $OUT/${TAG}_mfma_$w.txt 2>&1; head -30 $OUT/${TAG}_mfma_$w.txt
           done ;;
    mfmab) # the same MFMA-busy pass over one batch64 batch (k_decode_persistm, k_mrf_pair, the packed prefill)
           rm -rf $OUT/pmc_${TAG}_mfma_batch64
           timeout -s KILL 240 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_${TAG}_mfma_batch64 -o pmc -- python3 bench.py --workload batch64 --steps 1 --warmup 1 > $OUT/${TAG}_pmc_mfma_batch64.log 2>&1 || { tail -30 $OUT/${TAG}_pmc_mfma_batch64.log; exit 1; }
           python tools/mfma_util.py $OUT/pmc_${TAG}_mfma_batch64 > $OUT/${TAG}_mfma_batch64.txt 2>&1; head -30 $OUT/${TAG}_mfma_batch64.txt ;;
    pmc)   for c in FETCH_SIZE WRITE_SIZE; do
             rm -rf $OUT/pmc_${TAG}_$c
             timeout -s KILL 180 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_${TAG}_$c -o pmc -- python3 bench.py --steps 3 --warmup 1 > $OUT/${TAG}_pmc_$c.log 2>&1 || { tail -30 $OUT/${TAG}_pmc_$c.log; exit 1; }
             python tools/pmc_summary.py $OUT/pmc_${TAG}_$c --gfx950-fetch-x2 --json $OUT/${TAG}_pmc_$c.json > $OUT/${TAG}_pmc_$c.txt 2>&1; grep -i "persist\|conv1d<11" $OUT/${TAG}_pmc_$c.txt | head -5 || true
           done ;;
  esac
done
