cd "$GRAFT_REPO_ROOT"
T=$(mktemp -d)
for v in 1 0 1 0; do
  LSDR_BENCH_PLACE_INPUT=$v LSDR_BENCH_MORE_ONLY=c3,anf1,c2_offset LSDR_BENCH_FULL=$T/ab_in_$v.json timeout 900 python bench.py --steps 2 --warmup 1 --full --no-cpu > /dev/null 2> $T/ab_in.err
  python - <<PY
import json
j=json.load(open("$T/ab_in_$v.json"))
m=j["more"]
print("place_input=$v", {k:(m[k].get("value"), m[k].get("pass"), m[k].get("error","")[:200]) for k in m})
PY
done
