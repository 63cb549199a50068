#!/bin/bash
# A/B of two builds on the C3 bench (+ the GPU parity tests on the B build).
#   ALT_LIB=galah_amd/lib_alt/libgalahgpu.so OUT=ab_logs bash scripts/ab.sh [pytest -k expr]
# Logs go to $OUT (default: build/ab).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 2
export TMPDIR=/tmp
out="${OUT:-build/ab}"
mkdir -p "$out"
ALT=${ALT_LIB:-galah_amd/lib_alt/libgalahgpu.so}
echo "== tests (B)"
GALAHGPU_LIB=$ALT timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread ${1:+-k "$1"} > "$out/ab_tests.log" 2>&1 || { tail -30 "$out/ab_tests.log"; exit 1; }
tail -2 "$out/ab_tests.log"
show() {  # log: ms per step, phases, K1 / finalize / K2 device ms per step
  python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['ms_per_step'], d['phase_ms'], d['kernel_ms_per_step'])" "$1"
}
for r in 1 2; do
  echo "== bench A"
  timeout -k 10 300 python -u bench.py --steps 3 --warmup 1 > "$out/ab_a$r.log" 2>&1 || exit 1
  show "$out/ab_a$r.log"
  echo "== bench B"
  GALAHGPU_LIB=$ALT timeout -k 10 300 python -u bench.py --steps 3 --warmup 1 > "$out/ab_b$r.log" 2>&1 || exit 1
  show "$out/ab_b$r.log"
done
