"""Timing of the cross-covariance entries at n1 = n2 = 4096, D = 1, aligned
operands: smg_gp_cross_cov_fwd and smg_gp_cross_cov_rev of the four families
next to the symmetric entries smg_gp_cov_fwd and smg_gp_cov_rev on the same
points and adjoint (both pairs move the same bytes: one write of K, one read of
Kadj), by the context's HIP-event regions (one region per call), 21 repeats
after three warm-up calls: median and min-max, and the reverse's GB/s against
its one read of Kadj; then exp_quad's cross entries on the same bytes as a tall
K with 64 columns.  DESIGN.md "GP cross-covariance" holds the table this
printed.

    python3 tools/time_gp_cross.py [N]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS, WARM = 21, 3
SIG, ELL = 1.3, 0.9
FAMILIES = (("exp_quad", 0), ("exponential", 1), ("matern32", 2), ("matern52", 3))


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


def line(what, ms, nbytes):
    med = statistics.median(ms)
    print(f"{what:44s} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}  "
          f"{nbytes / med / 1e6:8.1f} GB/s", flush=True)
    return med


def main():
    rng = np.random.default_rng(N)
    x = rng.uniform(-10, 10, N)
    xs = rng.uniform(-10, 10, N)
    nbytes = 8.0 * N * N
    with hip.Context(0, 2 << 30) as c:
        dx, dxs = c.put(x), c.put(xs)
        dK, dA, o = c.zeros(N * N), c.put(rng.uniform(-1, 1, N * N)), c.zeros(2)
        for name, fam in FAMILIES:
            f0 = line(f"N={N} {name} cov_fwd (yardstick)", timed(
                c, lambda: c.call("smg_gp_cov_fwd", fam, dx, 1, N, SIG, ELL, dK, N)), nbytes)
            f1 = line(f"N={N} {name} cross_cov_fwd", timed(
                c, lambda: c.call("smg_gp_cross_cov_fwd", fam, dxs, N, dx, N, 1, SIG, ELL, dK, N)), nbytes)
            r0 = line(f"N={N} {name} cov_rev (yardstick)", timed(
                c, lambda: c.call("smg_gp_cov_rev", fam, dx, 1, N, SIG, ELL, dA, N, o)), nbytes)
            r1 = line(f"N={N} {name} cross_cov_rev", timed(
                c, lambda: c.call("smg_gp_cross_cov_rev", fam, dxs, N, dx, N, 1, SIG, ELL, dA, N, o)), nbytes)
            print(f"ratio {name}: cross / symmetric  fwd {f1 / f0:.3f}  rev {r1 / r0:.3f}", flush=True)
        # the same bytes as a tall K: N * N / 64 rows, 64 columns (the rows split over the grid)
        n1, n2 = N * N // 64, 64
        dt = c.put(rng.uniform(-10, 10, n1))
        line(f"{n1} x {n2} exp_quad cross_cov_fwd", timed(
            c, lambda: c.call("smg_gp_cross_cov_fwd", 0, dt, n1, dx, n2, 1, SIG, ELL, dK, n1)), nbytes)
        line(f"{n1} x {n2} exp_quad cross_cov_rev", timed(
            c, lambda: c.call("smg_gp_cross_cov_rev", 0, dt, n1, dx, n2, 1, SIG, ELL, dA, n1, o)), nbytes)


if __name__ == "__main__":
    main()
