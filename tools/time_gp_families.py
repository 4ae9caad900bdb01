"""Timing of the GP covariance families at N = 4096, D = 1, aligned operands:
the C entries smg_gp_cov_fwd / _rev / _inverse_adjoint of the exponential and
Matern 3/2, 5/2 families next to the squared-exponential entries
(smg_gp_exp_quad_cov_nd_fwd / _nd_rev, smg_gp_inverse_adjoint: the yardstick),
by the context's HIP-event regions (one region per call), 5 repeats after a
warm-up: median and min-max.  Then the GP-marginal gradient through the tape
(tests/cpp/_bin/test_gp_families, mode "time") for exp_quad and matern52 over
20 steps.  DESIGN.md "Covariance families" holds the table this printed.

    python3 tools/time_gp_families.py [N]
"""
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402
from _util import ROOT, prebuilt  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = 5
SIG, ELL, NOISE = 1.3, 0.7, 0.5
rng = np.random.default_rng(N)
x = rng.uniform(-10, 10, N)
y = rng.standard_normal(N)


def timed(ctx, call):
    """ms of the GP-family regions of REPS calls after one warm-up call."""
    call()
    out = []
    for _ in range(REPS):
        ctx.profile(True)
        call()
        ms, cnt, _ = ctx.profile_read("gp")
        assert cnt == 1, cnt
        out.append(ms)
    ctx.profile(False)
    return out


def line(what, ms):
    print(f"{what:44s} median {statistics.median(ms):8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}  "
          f"raw {' '.join(f'{v:.4f}' for v in ms)}", flush=True)


with hip.Context(0, 2 << 30) as ctx:
    M = rng.uniform(-1, 1, (N, N))
    dx = ctx.put(x)
    dK, dA, dC = ctx.zeros(N * N), ctx.put(M.ravel()), ctx.put((M + M.T).ravel())
    ds, dd, o2 = ctx.put(rng.uniform(-1, 1, 2 * N)), ctx.zeros(1), ctx.zeros(2)
    for name, fam in (("exp_quad (yardstick)", 0), ("exponential", 1), ("matern32", 2), ("matern52", 3)):
        if fam == 0:
            f = lambda: ctx.call("smg_gp_exp_quad_cov_nd_fwd", dx, 1, N, SIG, ELL, dK, N)  # noqa: E731
            r = lambda: ctx.call("smg_gp_exp_quad_cov_nd_rev", dx, 1, N, SIG, ELL, dA, N, o2)  # noqa: E731
            i = lambda: ctx.call("smg_gp_inverse_adjoint", dC, N, N, ds, 1, 2 * N, 0.8, dK, N, dx, 1, SIG, ELL, dd,  # noqa: E731
                                 o2)
        else:
            f = lambda: ctx.call("smg_gp_cov_fwd", fam, dx, 1, N, SIG, ELL, dK, N)  # noqa: E731
            r = lambda: ctx.call("smg_gp_cov_rev", fam, dx, 1, N, SIG, ELL, dA, N, o2)  # noqa: E731
            i = lambda: ctx.call("smg_gp_cov_inverse_adjoint", fam, dC, N, N, ds, 1, 2 * N, 0.8, dK, N, dx, 1, SIG,  # noqa: E731
                                 ELL, dd, o2)
        line(f"N={N} {name} fwd", timed(ctx, f))
        line(f"N={N} {name} rev", timed(ctx, r))
        line(f"N={N} {name} inverse_adjoint", timed(ctx, i))

# the GP-marginal gradient through the tape, one fresh process per family
exe = prebuilt(os.path.join(ROOT, "tests", "cpp", "_bin", "test_gp_families"))
for family in ("exp_quad", "matern52"):
    stdin = f"time {family} 20 {N} {SIG} {ELL} {NOISE}\n" + " ".join(map(repr, x.tolist())) + "\n" + \
        " ".join(map(repr, y.tolist())) + "\n"
    p = subprocess.run([exe], input=stdin, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        sys.exit(f"{family}: exit {p.returncode}: {p.stderr[-1000:]}")
    rows = [l.split() for l in p.stdout.strip().splitlines()]
    line(f"N={N} {family} GP-marginal gradient step", [float(r[2]) for r in rows])
    print(f"    last: {' '.join(rows[-1][4:])}", flush=True)
