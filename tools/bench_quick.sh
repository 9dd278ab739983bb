cd "$(dirname "$0")/.."; O=${OUT:-out}; mkdir -p $O
timeout 600 python bench.py --full --no-cpu-baseline > $O/bq.json 2> $O/bq.err; python - $O/bq.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(d["value"], "img/s", d["ms_per_step"], "ms/step  p50 b1", d.get("p50_latency_ms_batch1"))
for k, v in d["kernels"].items(): print(f"  {k:18s} {v['avg_ms']:.4f} ms x{v['launches_per_step']}  {v.get('tflops','')}")
PY
