# The fit of the mixed series (bench.py's mixed_models block) with MacaqueV gaps going to the wave encoder from
# 256 (default) / 128 / 64 / 32 values on. Usage: scripts/ab/gap_min_values.sh OUT_DIR
out=${1:?usage: scripts/ab/gap_min_values.sh OUT_DIR}
for g in 256 128 64 32; do
  MDB_FIT_GAP_MIN_VALUES=$g timeout 400 python bench.py --full --no-irregular --no-host-path --steps 2 > $out/bench_gap$g.json 2>/dev/null
  echo "gap min values $g"; python3 scripts/show_mixed_fit.py $out/bench_gap$g.json | head -2
done
