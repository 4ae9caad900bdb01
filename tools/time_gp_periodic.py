"""Timing of the periodic and dot-product covariance entries at n1 = n2 = 4096,
D = 1, aligned operands: smg_gp_periodic_cov_fwd / _rev and
smg_gp_dot_prod_cov_fwd / _rev next to smg_gp_cross_cov_fwd / _rev with
SMG_GP_EXP_QUAD on the same points and adjoint (all of them move the same
bytes: one write of K, one read of Kadj), by the context's HIP-event regions
(one region per call), 21 repeats after three warm-up calls: median and
min-max, the GB/s against those bytes, and each entry's ratio to the exp_quad
line.  DESIGN.md "Periodic and dot-product covariances" holds the table this
printed.

    python3 tools/time_gp_periodic.py [N]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS, WARM = 21, 3
SIG, ELL, PER = 1.3, 0.9, 1.7


def timed(ctx, call):
    """ms of the GP-family region of each of REPS calls after WARM warm-up calls."""
    for _ in range(WARM):
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


def line(what, ms, nbytes, base=None):
    med = statistics.median(ms)
    ratio = "" if base is None else f"  x{med / base:5.2f} of exp_quad"
    print(f"{what:36s} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}  "
          f"{nbytes / med / 1e6:8.1f} GB/s{ratio}", flush=True)
    return med


def main():
    rng = np.random.default_rng(N)
    x = rng.uniform(-10, 10, N)
    xs = rng.uniform(-10, 10, N)
    nbytes = 8.0 * N * N
    with hip.Context(0, 2 << 30) as c:
        dx, dxs = c.put(x), c.put(xs)
        dK, dA, o = c.zeros(N * N), c.put(rng.uniform(-1, 1, N * N)), c.zeros(3)
        f0 = line(f"N={N} exp_quad cross_cov_fwd", timed(
            c, lambda: c.call("smg_gp_cross_cov_fwd", 0, dxs, N, dx, N, 1, SIG, ELL, dK, N)), nbytes)
        line(f"N={N} periodic_cov_fwd", timed(
            c, lambda: c.call("smg_gp_periodic_cov_fwd", dxs, N, dx, N, 1, SIG, ELL, PER, dK, N)), nbytes, f0)
        line(f"N={N} dot_prod_cov_fwd", timed(
            c, lambda: c.call("smg_gp_dot_prod_cov_fwd", dxs, N, dx, N, 1, SIG, dK, N)), nbytes, f0)
        r0 = line(f"N={N} exp_quad cross_cov_rev", timed(
            c, lambda: c.call("smg_gp_cross_cov_rev", 0, dxs, N, dx, N, 1, SIG, ELL, dA, N, o)), nbytes)
        line(f"N={N} periodic_cov_rev", timed(
            c, lambda: c.call("smg_gp_periodic_cov_rev", dxs, N, dx, N, 1, SIG, ELL, PER, dA, N, o)), nbytes, r0)
        line(f"N={N} dot_prod_cov_rev", timed(
            c, lambda: c.call("smg_gp_dot_prod_cov_rev", N, N, SIG, dA, N, o)), nbytes, r0)


if __name__ == "__main__":
    main()
