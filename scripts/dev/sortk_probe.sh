#!/bin/bash
# r05s experiment: the same stiffness draws, assigned to the envs in drawn order against sorted order (envs of similar stiffness share a solver wavefront)
cd $GRAFT_REPO_ROOT
OUT=${OUT:-dev_out}; mkdir -p "$OUT"
for s in softbox softcylinder softball; do
  for k in "" 1; do
    SG_EXP_SORT_K=$k timeout -k 10 300 python3 bench.py --full --steps 200 --warmup 0 --no-cpu-baseline --no-fix-variant --scene $s > $OUT/r05s_sortk_${s}_$k.json 2> $OUT/r05s_sortk_${s}_$k.err || { tail -5 $OUT/r05s_sortk_${s}_$k.err; exit 1; }
    python3 -c "import json;l=json.load(open('$OUT/r05s_sortk_${s}_$k.json'));print('$s sorted=$k',round(l['value']),l['roofline']['avg_kernel_ms'],l['config']['envs_flagged_bad'], l['roofline'].get('dominant_kernel',{}).get('avg_launch_ms'))"
  done
done
