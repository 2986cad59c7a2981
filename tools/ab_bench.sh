#!/bin/bash
# same-box A/B of bench.py, interleaved: tools/ab_bench.sh "<cfg>" "<cfg>" ...
#   cfg = env toggles "VAR=VAL ..." and / or "tree=DIR": the bench.py of another, already built checkout (the parent
#   commit exported with `git archive` and built with make, say); an empty cfg "" is this tree as it stands.
#   ROUNDS (default 2) rounds of every cfg in turn, BLOCKS (default 3) timed blocks per run.
out=gpurun_out/ab_bench.log
mkdir -p $(dirname $out)
: > $out
for round in $(seq 1 ${ROUNDS:-2}); do
  i=0
  for cfg in "$@"; do
    i=$((i+1))
    dir=.; envs=""
    for word in $cfg; do
      case $word in tree=*) dir=${word#tree=};; *) envs="$envs $word";; esac
    done
    echo "== round $round cfg[$i]: $cfg" >> $out
    # a run that fails or overruns ends the comparison: nothing more is started on the GPU after it
    line=$(cd $dir && env $envs timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --blocks ${BLOCKS:-3} --no-cpu-baseline 2>/dev/null) \
      || { echo "bench.py failed (status $?) in round $round cfg[$i]" | tee -a $out; exit 1; }
    echo "$line" | python -c "
import sys, json
for l in sys.stdin:
    l = l.strip()
    if l.startswith('{'):
        d = json.loads(l); r = d['roofline']
        print(d['value'], 'img/s', d['ms_per_step'], 'ms', 'p10', d.get('ms_per_step_p10'), 'p90', d.get('ms_per_step_p90'),
              json.dumps(r['per_class_ms_per_step']))
" >> $out
  done
done
cat $out
