set -e
D=${1:?usage: bash tools/pw_check.sh OUTDIR}; mkdir -p $D
python -m pytest tests/test_hip_ops.py tests/test_hip_embed.py tests/test_hip_fuzz.py tests/test_hip_projection.py -x -q -m gpu > $D/tests.log 2>&1 || { tail -30 $D/tests.log; exit 1; }
tail -2 $D/tests.log
python bench.py --full --no-cpu-baseline --gradient-steps 0 --targets 0 --landmark-callback none --config4 0 --config5-targets 0 --bf16x3-leg 0 > $D/bench.json 2> $D/bench.err
python - "$D/bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print('HEADLINE', d['value'], d['ms_per_step'], 'objectives', {k:v.get('value') for k,v in d.get('objectives',{}).items()} if isinstance(d.get('objectives'),dict) else d.get('objectives'))
PY
