# A/B of two engine libraries built from one tree (TPAMD_LIBRARY selects the .so), in turn:
# 3 x 300 pipelined steps and 2 x 300 unpipelined steps of each, then 3 x `bench.py --steps 20 --warmup 5`
# of each, after the parity tests of the sweep on both. Build the other library with
#   engine.build_library(force=True, extra_flags=[...], output=".../libtpamd_prev.so")
# (or from the parent's sources). One line per run; a run that fails or outlives its limit ends the script.
#   bash tools/ab_two_libraries.sh [new.so [prev.so]]        (names inside csrc/)
export TMPDIR=/tmp
cd "$(dirname "$0")/.." || exit 1
NEW=${1:-libtpamd.so}
PREV=${2:-libtpamd_prev.so}
LINE=$(mktemp) || exit 1
trap 'rm -f "$LINE"' EXIT
# parity first: a library that is not bit-identical to the oracle is not worth timing
for lib in $NEW $PREV; do
TPAMD_LIBRARY=$PWD/x-edr-trajectory-planning_amd/csrc/$lib timeout -k 10 300 python -m pytest tests/test_gpu_emit_pipeline.py tests/test_gpu_sweep_runahead.py -m gpu -x -q 2>&1 | tail -1
[ ${PIPESTATUS[0]} -eq 0 ] || { echo "$lib parity FAILED"; exit 1; }
done
run() { # label, library, bench arguments...
  local label=$1 lib=$2; shift 2
  TPAMD_LIBRARY=$PWD/x-edr-trajectory-planning_amd/csrc/$lib timeout -k 10 300 python bench.py "$@" 2>/dev/null > "$LINE"
  local rc=$?
  [ $rc -eq 0 ] || { echo "$lib $label FAILED rc=$rc"; exit $rc; }
  python -c "
import sys,json; d=json.loads(open('$LINE').read().strip().splitlines()[-1]); r=d.get('roofline') or {}
print('$lib $label', d['value'], d['ms_per_step'], {k:v['ms'] for k,v in (r.get('kernels') or {}).items()})"
}
for rep in 1 2 3; do for lib in $NEW $PREV; do
run piped300 $lib --steps 300 --warmup 5 --no-cpu-baseline
done; done
for rep in 1 2; do for lib in $NEW $PREV; do
run unpiped300 $lib --steps 300 --warmup 5 --no-cpu-baseline --no-pipeline
done; done
for rep in 1 2 3; do for lib in $NEW $PREV; do
run bench20 $lib --steps 20 --warmup 5
done; done
