"""Timing of smg_ordered_logistic_glm next to smg_poisson_log_glm (unchanged
code: the yardstick) on the same x, at R = 1e6 x M = 256 and R = 1e6 x M = 8,
for C = 5 and C = 16 classes, by the context's HIP-event regions (one region
per call of the C entry), in one process: three warm-up calls of each, then
21 rounds that alternate the entries.  Prints median (min-max), the TB/s of x
(8 R M bytes per call) and the ratio of the medians.  DESIGN.md "Ordered
logistic GLM" holds the lines this printed.

    python3 tools/time_glm_ordered.py [R]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402

R = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1000000
REPS, WARM = 21, 3
CS = (5, 16)


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
            yp = c.put(np.floor(rng.uniform(0.0, 6.0, R)).astype(np.int32))
            beta = rng.uniform(-1.0, 1.0, M) * np.sqrt(3.0 / M)
            ab = c.put(np.concatenate([[0.1], beta]))
            ws = c.zeros(int(max(c.lib.smg_glm_ws_doubles(R, M),
                                 max(c.lib.smg_ordered_logistic_glm_ws_doubles(R, M, C) for C in CS))))
            out = c.zeros(M + max(CS) + 3)
            calls = {"poisson_log_glm": lambda: c.call("smg_poisson_log_glm", yp, x, R, M, R, ab, ws, out)}
            for C in CS:
                yo = c.put((1 + np.floor(rng.uniform(0.0, C, R))).astype(np.int32))
                bc = c.put(np.concatenate([beta, np.linspace(-2.0, 2.0, C - 1)]))
                calls[f"ordered_logistic_glm C={C}"] = (
                    lambda yo=yo, bc=bc, C=C: c.call("smg_ordered_logistic_glm", yo, x, R, M, R, C, bc, ws, out))
            for f in calls.values():
                for _ in range(WARM):
                    f()
            ms = {k: [] for k in calls}
            for _ in range(REPS):
                for k, f in calls.items():
                    ms[k].append(region_ms(c, f))
            c.profile(False)
            assert np.all(np.isfinite(c.get(out, M + max(CS))))
            med = {k: line(f"R={R} M={M} {k}", v, 8.0 * R * M) for k, v in ms.items()}
            for C in CS:
                print(f"R={R} M={M} C={C} ordered_logistic / poisson = "
                      f"{med[f'ordered_logistic_glm C={C}'] / med['poisson_log_glm']:.3f}", flush=True)
            c.rewind(m0)


if __name__ == "__main__":
    main()
