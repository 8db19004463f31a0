#!/usr/bin/env bash
# On a machine with an MI355X: full parity suite, smoke, the full bench line (bench.py --full: with
# the mirror check, e2e_host and cpu_baseline), N=2 rehearsal (gloo, two ranks on one GPU), the
# other configs, per-step symbol latency, rocprof kernel stats + PMC traffic (headline and
# configs[4]), the keyed decode-side kernel trace. Usage: bash tools/gpu_round.sh <tag>
# The logs and JSON lines of this script go to $SSNT_OUT (default: out/); the profile scripts it
# ends with keep their own output directories.
set -euo pipefail
TAG=${1:-r2}
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${SSNT_OUT:-out}
mkdir -p "$OUT"
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > "$OUT/pytest_gpu_${TAG}.log" 2>&1 || { tail -40 "$OUT/pytest_gpu_${TAG}.log"; exit 1; }
tail -2 "$OUT/pytest_gpu_${TAG}.log"
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke_${TAG}.log" 2>&1
tail -1 "$OUT/smoke_${TAG}.log"
timeout -k 10 300 python3 bench.py --full > "$OUT/bench_${TAG}.json" 2> "$OUT/bench_${TAG}.err"
cat "$OUT/bench_${TAG}.json"
timeout -k 10 200 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --full --gpus 2 --steps 20 --warmup 5 --dist-backend gloo > "$OUT/bench2_${TAG}.json" 2> "$OUT/bench2_${TAG}.err"
cat "$OUT/bench2_${TAG}.json"
timeout -k 10 300 python3 tools/bench_configs.py > "$OUT/configs_${TAG}.jsonl" 2> "$OUT/configs_${TAG}.err"
cat "$OUT/configs_${TAG}.jsonl"
timeout -k 10 200 python3 tools/bench_step_symbols.py > "$OUT/steps_${TAG}.json" 2> "$OUT/steps_${TAG}.err"
cat "$OUT/steps_${TAG}.json"
timeout -k 10 200 python3 tools/bench_cliff.py > "$OUT/cliff_${TAG}.jsonl" 2> "$OUT/cliff_${TAG}.err"
cat "$OUT/cliff_${TAG}.jsonl"
bash tools/profile_gpu.sh "$TAG"
bash tools/profile_long.sh "$TAG"
bash tools/profile_decode.sh "$TAG"
