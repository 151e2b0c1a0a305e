# does the untimed profile pass right before the timed region slow the timed steps?  (default 10 steps / 3 warm-up)
OUT=${OUT:-bench_logs}; mkdir -p "$OUT"
for r in 1 2 3; do
  for f in "" "--no-prof"; do
    python bench.py --full --no-secondary --no-cpu-baseline --no-general-leg $f > "$OUT/pe.json" 2>/dev/null
    echo "flags=[$f] $(python tools/benchsum.py "$OUT/pe.json" | cut -c1-70)"
  done
done
