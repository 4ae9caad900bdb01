#!/bin/bash
# one GPU call: the GPU test suite, then one bench line per workload named in
# $2.. (default gp), no CPU baseline.  Each step time-limited; first failure ends it.
set -o pipefail
O=${SMG_OUT:-bench_out}
mkdir -p $O
TAG=${1:-t}
shift
WLS=${@:-gp}
timeout -k 10 800 python -u -m pytest tests -q -m gpu -x --timeout 200 --timeout-method thread > $O/${TAG}_pytest.log 2>&1 || { tail -40 $O/${TAG}_pytest.log; exit 1; }
tail -3 $O/${TAG}_pytest.log
for w in $WLS; do
  timeout -k 10 300 python bench.py --workload $w --full --no-cpu-baseline > $O/${TAG}_bench_$w.json 2> $O/${TAG}_bench_$w.err || { tail $O/${TAG}_bench_$w.err; exit 1; }
  python -c "import json;d=json.load(open('$O/${TAG}_bench_$w.json'));print('$w', d['value'], d['ms_per_step'], d['roofline']['frac'])"
done
