"""Timing of smg_neg_binomial_2_log_glm next to smg_poisson_log_glm (unchanged
code: the yardstick) on the same x and y, at R = 1e6 x M = 256 and R = 1e6 x
M = 8, by the context's HIP-event regions (one region per call of the C
entry), in one process: three warm-up calls of each, then 21 rounds that
alternate the two entries.  Prints median (min-max), the TB/s of x (8 R M bytes
per call) and the ratio of the medians.  DESIGN.md "Negative-binomial GLM"
holds the lines this printed.

    python3 tools/time_glm_neg_binomial.py [R]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402

R = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1000000
REPS, WARM = 21, 3
ALPHA, PHI = 0.1, 2.5


def region_ms(ctx, call):
    ctx.profile(True)
    call()
    ms, cnt, _ = ctx.profile_read("glm")
    assert cnt == 1, cnt
    return ms


def line(what, ms, nbytes):
    med = statistics.median(ms)
    print(f"{what:40s} median {med:8.4f} ms  (min {min(ms):8.4f} - max {max(ms):8.4f})  "
          f"{nbytes / med / 1e9:6.3f} TB/s of x", flush=True)
    return med


def main():
    with hip.Context(0, 4 << 30) as c:
        for M in (256, 8):
            m0 = c.mark()
            rng = np.random.default_rng(M)
            x = c.alloc(8 * R * M)
            c.call("smg_fill_unif", x, R * M, 20260101 + M, -1.0, 1.0, float(np.sqrt(3.0)))
            y = c.put(np.floor(rng.uniform(0.0, 6.0, R)).astype(np.int32))
            beta = rng.uniform(-1.0, 1.0, M) * np.sqrt(3.0 / M)
            ab = c.put(np.concatenate([[ALPHA], beta]))
            abp = c.put(np.concatenate([[ALPHA], beta, [PHI]]))
            ws = c.zeros(int(max(c.lib.smg_glm_ws_doubles(R, M), c.lib.smg_neg_binomial_2_log_glm_ws_doubles(R, M))))
            out = c.zeros(M + 6)
            calls = {
                "poisson_log_glm": lambda: c.call("smg_poisson_log_glm", y, x, R, M, R, ab, ws, out),
                "neg_binomial_2_log_glm": lambda: c.call("smg_neg_binomial_2_log_glm", y, x, R, M, R, abp, ws, out),
            }
            for f in calls.values():
                for _ in range(WARM):
                    f()
            ms = {k: [] for k in calls}
            for _ in range(REPS):
                for k, f in calls.items():
                    ms[k].append(region_ms(c, f))
            c.profile(False)
            assert np.all(np.isfinite(c.get(out, M + 6)))
            med = {k: line(f"R={R} M={M} {k}", v, 8.0 * R * M) for k, v in ms.items()}
            print(f"R={R} M={M} neg_binomial / poisson = {med['neg_binomial_2_log_glm'] / med['poisson_log_glm']:.3f}",
                  flush=True)
            c.rewind(m0)


if __name__ == "__main__":
    main()
