#!/bin/bash
# A/B on ONE box: depth-normal regulariser inside the SSIM gradient's launch (default) against its own launch (IGS_NO_LOSS_MIX=1);
# BASELINE configs[4] side leg of bench.py, alternating, 3 rounds
for i in 1 2 3; do
  for v in mix nomix; do
    if [ $v = nomix ]; then export IGS_NO_LOSS_MIX=1; else unset IGS_NO_LOSS_MIX; fi
    timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-dropin-leg --no-cold-leg --side-steps 200 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); s=d['side_legs']; print('[%s]' % sys.argv[1], 'cfg3', round(d['ms_per_step'],4), 'cfg4', round(s['cfg4']['ms_per_step'],4), 'cfg5', round(s['cfg5']['ms_per_step'],4))" "$v" || exit 1
  done
done
