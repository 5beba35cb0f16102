# Host-side profile (cProfile, backward on the calling thread) of the reference 32 x 64 schedule.
# usage: bash tools/gpu/host_prof.sh OUT_DIR
set -o pipefail
OUT=${1:?usage: host_prof.sh OUT_DIR}
mkdir -p "$OUT"
timeout -k 10 400 python tools/host_prof.py "$OUT/ref.prof" --full --steps 1 --warmup 1 --ref-steps 4 --json-out "$OUT/b.json" > "$OUT/b.log" 2>&1 || exit $?
python - "$OUT/ref.prof" <<'PY' > "$OUT/top.txt"
import pstats
import sys
p = pstats.Stats(sys.argv[1])
p.sort_stats("tottime").print_stats(70)
p.sort_stats("cumulative").print_stats(120)
PY
