"""Timing of the per-dimension length-scale (ARD) entries at N = 4096, D = 4,
aligned operands: smg_gp_ard_scale, smg_gp_ard_cov_rev and
smg_gp_ard_cov_inverse_adjoint of the four families next to their yardsticks
on the same points, smg_gp_cov_rev and smg_gp_cov_inverse_adjoint_x with D = 4
and one scalar length scale, by the context's HIP-event regions (one region
per call), 5 repeats after a warm-up: median and min-max.  Then the GP-marginal
gradient step through the tape (tests/cpp/_bin/test_gp_ard, mode "time") with
the ARD overload and with the scalar-length-scale overload on the same points,
5 steps after the program's three warm-up evaluations.  DESIGN.md "ARD length
scales" holds the table this printed (profiles/gp_ard_n4096.txt the raw lines).

    python3 tools/time_gp_ard.py [N [D]]
"""
import ctypes
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
D = int(sys.argv[2]) if len(sys.argv) > 2 else 4
REPS = 5
SIG, NOISE = 1.3, 0.5
ELLS = np.linspace(0.7, 2.1, D)
ELL = float(ELLS[0])  # the yardsticks' scalar length scale
rng = np.random.default_rng(N + D)
x = rng.uniform(-10, 10, (N, D))
y = rng.standard_normal(N)
FAMILIES = (("exp_quad", 0), ("exponential", 1), ("matern32", 2), ("matern52", 3))


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
    print(f"{what:52s} median {statistics.median(ms):8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}  "
          f"raw {' '.join(f'{v:.4f}' for v in ms)}", flush=True)
    return statistics.median(ms)


def entries(ctx):
    """The three ARD entries and their yardsticks; {name: median ms}."""
    lp = ctypes.c_void_p(ELLS.ctypes.data)
    M = rng.uniform(-1, 1, (N, N))
    dx, dz, dzt = ctx.put(x.ravel()), ctx.zeros(N * D), ctx.zeros(N * D)
    dA, dC = ctx.put(M.ravel()), ctx.put((M + M.T).ravel())
    ds, dd, o, o2 = ctx.put(rng.uniform(-1, 1, 2 * N)), ctx.zeros(1), ctx.zeros(1 + D), ctx.zeros(2)
    med = {}
    med["scale"] = line(f"N={N} D={D} ard_scale",
                        timed(ctx, lambda: ctx.call("smg_gp_ard_scale", dx, D, N, lp, dz, dzt)))
    for name, fam in FAMILIES:
        med[name, "rev"] = line(f"N={N} D={D} {name} ard_cov_rev", timed(
            ctx, lambda: ctx.call("smg_gp_ard_cov_rev", fam, dzt, D, N, SIG, lp, dA, N, o)))
        med[name, "rev0"] = line(f"N={N} D={D} {name} cov_rev (yardstick)", timed(
            ctx, lambda: ctx.call("smg_gp_cov_rev", fam, dx, D, N, SIG, ELL, dA, N, o2)))
        med[name, "inv"] = line(f"N={N} D={D} {name} ard_cov_inverse_adjoint", timed(
            ctx, lambda: ctx.call("smg_gp_ard_cov_inverse_adjoint", fam, dC, N, N, ds, 1, 2 * N, 0.8, dzt, D, SIG, lp,
                                  dd, o)))
        med[name, "inv0"] = line(f"N={N} D={D} {name} cov_inverse_adjoint_x (yardstick)", timed(
            ctx, lambda: ctx.call("smg_gp_cov_inverse_adjoint_x", fam, dC, N, N, ds, 1, 2 * N, 0.8, dx, D, SIG, ELL,
                                  dd, o2)))
    return med


def tape():
    """The GP-marginal gradient step, one fresh process per family and overload."""
    exe = prebuilt(os.path.join(ROOT, "tests", "cpp", "_bin", "test_gp_ard"))
    nums = lambda a: " ".join(map(repr, np.asarray(a).ravel().tolist()))  # noqa: E731
    for family in ("exp_quad", "matern52"):
        for ard in (1, 0):
            stdin = f"time {family} {ard} {REPS} {D} {N} {SIG} {nums(ELLS)} {NOISE}\n{nums(x)}\n{nums(y)}\n"
            p = subprocess.run([exe], input=stdin, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{family}: exit {p.returncode}: {p.stderr[-1000:]}")
            rows = [l.split() for l in p.stdout.strip().splitlines()]
            what = "ARD" if ard else "scalar l (yardstick)"
            line(f"N={N} D={D} {family} GP-marginal gradient step, {what}", [float(r[2]) for r in rows])
            print(f"    last: {' '.join(rows[-1][4:])}", flush=True)


if __name__ == "__main__":
    with hip.Context(0, 2 << 30) as c:
        m = entries(c)
    for name, _ in FAMILIES:
        print(f"ratio {name}: ard_cov_rev / cov_rev {m[name, 'rev'] / m[name, 'rev0']:.3f}   "
              f"ard_cov_inverse_adjoint / cov_inverse_adjoint_x {m[name, 'inv'] / m[name, 'inv0']:.3f}", flush=True)
    tape()
