#!/bin/bash
# Alternating A/B of the headline (bench.py --steps 100 --warmup 10) between the product library and a variant build:
#   tools/ab_headline.sh <tag> <variant-lib-name> [runs a side, default 6] [extra bench.py arguments ...]
# default = visfs_amd/lib/libvisfs_ba_hip.so, variant = visfs_amd/lib/libvisfs_ba_hip_<name>.so (tools/build_variant.sh); the runs
# alternate variant / default so that drift of the box hits both sides alike.  Decision rule: the two RANGES must not overlap.
# Logs go to $AB_OUT (default ab_out/).  Every run has its own time limit and the script stops at the first run that fails.
O=${AB_OUT:-ab_out}; TAG=$1; VAR=$2; N=${3:-6}; shift; shift; shift
mkdir -p $O
LOG=$O/${TAG}_headline_ab.log
for i in $(seq 1 $N); do
  for V in $VAR default; do
    if [ $V != default ]; then export VISFS_BA_LIB=$PWD/visfs_amd/lib/libvisfs_ba_hip_$V.so; else unset VISFS_BA_LIB; fi
    echo "== $V run $i" >> $LOG
    timeout -k 10 240 python bench.py --gpus 1 --steps 100 --warmup 10 --no-cpu-baseline "$@" >> $LOG 2>&1 || { echo "run failed: $V $i (status $?)" | tee -a $LOG; exit 1; }
  done
done
unset VISFS_BA_LIB
grep -h '"value"\|^==' $LOG | python -c "
import sys, json, statistics
side, vals = None, {}
for ln in sys.stdin:
    if ln.startswith('=='): side = ln.split()[1]; continue
    vals.setdefault(side, []).append(json.loads(ln)['value'])
var = [k for k in vals if k != 'default'][0]
a, b = vals[var], vals['default']
print('bench.py --steps 100 --warmup 10 ' + ' '.join(sys.argv[1:]) + f' ({var} = the variant library, new = the product library, alternating runs, BA it/s)')
for name, v in ((var, a), ('new', b)):
    print(f'  {name:<7} runs ' + ' '.join(f'{x:.1f}' for x in v) + f' | median {statistics.median(v):.1f} | min {min(v):.1f} max {max(v):.1f}')
verdict = 'ranges do not overlap: new above ' + var if min(b) > max(a) else 'ranges do not overlap: new BELOW ' + var if max(b) < min(a) else 'ranges overlap'
print(f'  median new / {var} = {statistics.median(b) / statistics.median(a):.4f} | {verdict}')
" "$@" | tee $O/${TAG}_headline_ab.txt
