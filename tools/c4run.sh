OUT=${OUT:-bench_logs}; mkdir -p "$OUT"
timeout -k 10 300 python tools/bench_configs.py c4 > "$OUT/c4.log" 2>&1 || { tail -5 "$OUT/c4.log"; exit 1; }
cat "$OUT/c4.log"
