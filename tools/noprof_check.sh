OUT=${OUT:-bench_logs}; mkdir -p "$OUT"
for c in 1 256; do for p in "" "--no-prof"; do
  timeout -k 10 300 python bench.py --full --chains $c --no-secondary --no-cpu-baseline --steps 10 --warmup 3 $p > "$OUT/np.log" 2>&1 || { tail -3 "$OUT/np.log"; exit 1; }
  python - <<PY
import json
for l in open("$OUT/np.log"):
    if l.startswith("{"):
        d = json.loads(l); print("chains $c prof='$p':", round(d["value"], 1), round(d["ms_per_step"], 4))
PY
done; done
