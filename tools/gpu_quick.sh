#!/bin/bash
# one GPU call: the GPU test suite + one bench line (no CPU baseline)
set -o pipefail
O=${SMG_OUT:-bench_out}
mkdir -p $O
TAG=${1:-q}
timeout -k 10 600 python -u -m pytest tests -q -m gpu -x --timeout 120 --timeout-method thread > $O/${TAG}_pytest.log 2>&1 || { tail -30 $O/${TAG}_pytest.log; exit 1; }
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err || { tail $O/${TAG}_bench.err; exit 1; }
