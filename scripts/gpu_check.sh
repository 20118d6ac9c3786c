# one GPU call: the whole -m gpu suite, then C2 and LeGO bench lines
# (no CPU baselines) -> $OUT/<tag>_* (default bench_out/)
set -o pipefail
export TMPDIR=/tmp
out=${OUT:-bench_out}; mkdir -p $out
tag=${1:-r06a}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $out/${tag}_tests.log 2>&1 || { tail -40 $out/${tag}_tests.log; exit 3; }
tail -2 $out/${tag}_tests.log
timeout -k 10 120 ./scripts/micro/launch_cost > $out/${tag}_launch_cost.jsonl 2>&1 || exit 6
B="timeout -k 10 300 python bench.py --full --no-cpu-baseline"
$B --steps 200 --warmup 10 > $out/${tag}_bench_c2.json 2>$out/${tag}_bench_c2.err || exit 4
$B --workload lego > $out/${tag}_bench_lego.json 2>/dev/null || exit 5
timeout -k 10 300 python bench.py --full --workload s2m --steps 20 --warmup 2 > $out/${tag}_bench_s2m.json 2>$out/${tag}_bench_s2m.err || exit 7
python - <<PY
import json
for n in ("c2", "lego", "s2m"):
    d = json.load(open(f"$out/${tag}_bench_{n}.json"))
    print(n, round(d["value"]), round(d["ms_per_step"] * 1e3, 1), d["roofline"]["avg_launch_us"])
PY
