# Usage (on an MI355X): [OUT=<dir>] bash tools/gpu_check.sh <tag>  - the whole -m gpu suite, then the full bench line (bench.py --full),
# both under $OUT (default: out/ in the repository)
TAG=${1:-chk}
cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p $OUT
timeout 1500 python -m pytest tests -x -q -m gpu > $OUT/${TAG}_gputest.txt 2>&1
tail -8 $OUT/${TAG}_gputest.txt
timeout 600 python bench.py --full > $OUT/${TAG}_bench.log 2>&1
tail -1 $OUT/${TAG}_bench.log > $OUT/${TAG}_bench.json
python - <<PY
import json
d = json.load(open("$OUT/${TAG}_bench.json"))
print({k: d[k] for k in ("value", "ms_per_step", "roofline", "ctc_loss_parity", "persistent_launches")})
print(d["kernel_ms"])
PY
