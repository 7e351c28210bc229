cd /root/repo
export OUT=${OUT:?set OUT to the directory for the bench lines}; mkdir -p "$OUT"
export PYTHONUNBUFFERED=1
for i in 1 2; do
python bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --latency-reps 100 2>/dev/null | tail -n 1 > "$OUT"/lat_split_$i.json
python bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --latency-reps 100 --no-split 2>/dev/null | tail -n 1 > "$OUT"/lat_nosplit_$i.json
done
python - <<'PY'
import json, os
for n in ("split_1","nosplit_1","split_2","nosplit_2"):
    d=json.load(open(os.environ["OUT"] + f"/lat_{n}.json")); print(n, round(d["value"],1), round(d["ms_per_step"],2), "fwd/frame", round(d["fwd_ms_per_frame"],3), "batch1", round(d["fwd_ms_batch1"],3), d["roofline"]["frac"])
PY
