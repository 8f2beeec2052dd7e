set -e
cd $GRAFT_REPO_ROOT
OUT=${OUT:-dev_out}; mkdir -p "$OUT"
T=${1:-r04y}
timeout -k 10 900 python3 -m pytest tests/test_gpu_tree.py -m gpu -x -q > $OUT/${T}_tree_tests.log 2>&1 || { tail -40 $OUT/${T}_tree_tests.log; exit 1; }
tail -3 $OUT/${T}_tree_tests.log
for s in freeball_fix fourfinger_softball_fix fourfinger_softball freeball; do
  timeout -k 10 600 python3 bench.py --full --steps 200 --warmup 0 --no-cpu-baseline --no-fix-variant --scene $s > $OUT/${T}_bench_$s.json 2> $OUT/${T}_bench_$s.err
  python3 -c "import json;l=json.load(open('$OUT/${T}_bench_$s.json'));print('$s',l['value'],l['roofline']['avg_kernel_ms'],l['config']['envs_flagged_bad'])"
done
python3 scripts/tree_section_profile.py freeball_fix > $OUT/${T}_tree_sections_freeball.txt 2>&1
grep -A24 "squeeze peak" $OUT/${T}_tree_sections_freeball.txt
