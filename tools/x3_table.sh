cd /root/repo
export OUT=${OUT:?set OUT to the directory for the bench lines}; mkdir -p "$OUT"
export PYTHONUNBUFFERED=1
DPFT_CONV_TABLE="$OUT"/table_f32.txt python bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --latency-reps 5 2>/dev/null | tail -n 1 > "$OUT"/tb_f32.json
DPFT_CONV_TABLE="$OUT"/table_x3.txt python bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --latency-reps 5 --dtype f32x3 2>/dev/null | tail -n 1 > "$OUT"/tb_x3.json

python bench.py --full --steps 40 --warmup 10 --no-cpu-baseline --latency-reps 30 --dtype f32x3 2>/dev/null | tail -n 1 > "$OUT"/step_x3_3.json
python bench.py --full --steps 40 --warmup 10 --no-cpu-baseline --latency-reps 30 2>/dev/null | tail -n 1 > "$OUT"/step_f32_3.json
python bench.py --full --steps 40 --warmup 10 --no-cpu-baseline --latency-reps 30 --dtype f32x3 2>/dev/null | tail -n 1 > "$OUT"/step_x3_4.json
python bench.py --full --steps 40 --warmup 10 --no-cpu-baseline --latency-reps 30 2>/dev/null | tail -n 1 > "$OUT"/step_f32_4.json
