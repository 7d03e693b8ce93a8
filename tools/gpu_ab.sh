#!/bin/bash
# A/B: the default build against every libdeme_v_*.so, interleaved rounds (box-to-box spread is ~5 %, run-to-run ~1 %)
#   AB_OUT=out ROUNDS=3 BENCH_ARGS="--steps 20 --warmup 5" TAG=driver_shape bash tools/gpu_ab.sh
#   AB_OUT: the directory the results go to (one sub-directory per TAG)
# Every bench run has its own time limit; the first one that fails ends the script.
TAG=${TAG:-ab}
out=${AB_OUT:?set AB_OUT to the directory the results go to}/$TAG; mkdir -p $out; rm -f $out/*.json $out/*.err
R=${ROUNDS:-2}
run() {  # name round [library]
  DEME_HIP_LIB=$3 timeout -k 10 ${BENCH_TIMEOUT:-300} python bench.py $BENCH_ARGS --no-cpu-baseline --state-cache /tmp/bed.npz > $out/$1_$2.json 2>$out/$1_$2.err
  rc=$?; [ $rc -eq 0 ] || { echo "$1 round $2: bench.py ended with $rc"; tail -5 $out/$1_$2.err; exit $rc; }
}
for r in $(seq 1 $R); do
  run cur $r ""
  for f in dem-engine_amd/csrc/libdeme_v_*.so; do
    n=$(basename $f .so); n=${n#libdeme_v_}
    run $n $r $PWD/$f
  done
done
python - $out <<'PY'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1]+'/*.json')):
    try:
        d=json.loads(open(f).read().strip().split('\n')[-1]); k=d['kernels_ms']
        print(f"{f:44s} step {d['ms_per_step']:.4f} force {k['calc_forces']:.4f} integ {k['integrate']:.4f} det {k['detect_update']:.3f}")
    except Exception as e: print(f,'ERR',e)
PY
