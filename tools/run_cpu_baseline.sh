# The full bench line's CPU baseline (bench.py --full), then the direct CPU measurement at the headline size
# (tools/cpu_c3.py) on the GPU box's host cores (via gpurun from the repo root).
set -o pipefail
cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out
timeout -k 10 600 python bench.py --full | python -c "
import json, sys; d = json.loads(sys.stdin.read().strip().splitlines()[-1])
print('bench', round(d['ms_per_step'], 1), 'ms; cpu', d['cpu_baseline'])
" || exit 1
timeout -k 10 700 python -u tools/cpu_c3.py --cap 200 > gpurun_out/cpu_c3.json 2> gpurun_out/cpu_c3.log || { tail -5 gpurun_out/cpu_c3.log; exit 1; }
cat gpurun_out/cpu_c3.json
