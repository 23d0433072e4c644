#!/bin/bash
# Interleaved default-bench A/B over several checkouts copied under the repo
# (each with its own built library).  usage: bash tools/ab_trees.sh ROUNDS DIR...
# ("." is this tree; "VAR=value@DIR" runs DIR with that environment
# variable set).  Prints value and phase times per run.
set -eo pipefail
R=$1; shift
OUT=${OUT:-$PWD/bench_out/abt}  # set OUT to keep the lines elsewhere
mkdir -p $OUT
for r in $(seq 1 $R); do
  for A in "$@"; do
    D=${A##*@}; E=""; [ "$D" != "$A" ] && E=${A%@*}
    n=$(echo $A | tr './=@' '____')
    (cd $D && env $E timeout -k 10 120 python bench.py --full --steps 20000 --warmup 500 --cpu-seconds 0) > $OUT/${n}_$r.json 2> $OUT/${n}_$r.err
    python -c "import json; a=json.loads(open('$OUT/${n}_$r.json').read().strip().splitlines()[-1]); print($r, '$A', a['value'], {k: round(v*1e3,2) for k,v in a['phase_ms'].items()})"
  done
done
