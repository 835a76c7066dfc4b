#!/bin/bash
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
OUT=${SVAE_OUT:-bench_out}  # where the logs and profiles go
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -m gpu -q -x > "$OUT"/tests.log 2>&1
rc=$?; echo tests_rc=$rc >> "$OUT"/tests.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke.log 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT"/prof_bf16 -o run -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > "$OUT"/prof.log 2>&1 || exit 1
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > "$OUT"/bench.log 2>&1 || exit 1
if [ "$1" != "pmc" ]; then exit 0; fi
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT"/pmc_fetch -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT"/pmc_fetch.log 2>&1 || exit 1
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT"/pmc_write -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT"/pmc_write.log 2>&1 || exit 1
