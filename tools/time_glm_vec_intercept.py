"""Timing of smg_glm_vec_intercept next to each kind's scalar entry (unchanged
code: the yardstick) on the same x and y, at R = 1e6 x M = 256 and R = 1e6 x
M = 8, for kinds 0 bernoulli_logit (against _checked), 1 normal_id, 2
poisson_log and 3 neg_binomial_2_log, by the context's HIP-event regions (one
region per call of the C entry), in one process: three warm-up calls of each,
then 21 rounds that alternate the three forms -- scalar, vector with theta_adj
null, vector with theta_adj stored.  Prints median (min-max), the TB/s of x
(8 R M bytes per call), the ratio of each vector form's median to the scalar
one's and the byte ratio it is held against, (8 M + 4 + 8 k) / (8 M + 4) per row
(kind 1: 8 M + 8), k = 1 for the load, k = 2 with the store.  DESIGN.md "One
intercept per row" holds the lines this printed.

    python3 tools/time_glm_vec_intercept.py [R]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402

R = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1000000
REPS, WARM = 21, 3
NAMES = ("bernoulli_logit", "normal_id", "poisson_log", "neg_binomial_2_log")
SCALAR = ("smg_bernoulli_logit_glm_checked", "smg_normal_id_glm", "smg_poisson_log_glm",
          "smg_neg_binomial_2_log_glm")


def region_ms(ctx, call):
    ctx.profile(True)
    call()
    ms, cnt, _ = ctx.profile_read("glm")
    assert cnt == 1, cnt
    return ms


def line(what, ms, nbytes):
    med = statistics.median(ms)
    print(f"{what:52s} median {med:8.4f} ms  (min {min(ms):8.4f} - max {max(ms):8.4f})  "
          f"{nbytes / med / 1e9:6.3f} TB/s of x", flush=True)
    return med


def main():
    with hip.Context(0, 4 << 30) as c:
        for M in (256, 8):
            m0 = c.mark()
            rng = np.random.default_rng(M)
            x = c.alloc(8 * R * M)
            c.call("smg_fill_unif", x, R * M, 20260101 + M, -1.0, 1.0, float(np.sqrt(3.0)))
            beta = rng.uniform(-1.0, 1.0, M) * np.sqrt(3.0 / M)
            av = c.put(rng.uniform(-0.5, 0.5, R))
            th = c.zeros(R)
            ys = (c.put((rng.uniform(0.0, 1.0, R) < 0.5).astype(np.int32)), c.put(rng.uniform(-2.0, 2.0, R)),
                  c.put(np.floor(rng.uniform(0.0, 6.0, R)).astype(np.int32)))
            ws = c.zeros(int(max(c.lib.smg_glm_ws_doubles(R, M), c.lib.smg_neg_binomial_2_log_glm_ws_doubles(R, M))))
            out = c.zeros(M + 6)
            for kind in range(4):
                y = ys[min(kind, 2)]
                ab = c.put(np.concatenate([[0.1], beta, [1.3]]))
                calls = {
                    "scalar": lambda y=y, ab=ab, kind=kind: c.call(SCALAR[kind], y, x, R, M, R, ab, ws, out),
                    "vector": lambda y=y, ab=ab, kind=kind: c.call("smg_glm_vec_intercept", kind, y, x, R, M, R, av,
                                                                   ab, ws, out, None),
                    "vector + theta_adj": lambda y=y, ab=ab, kind=kind: c.call("smg_glm_vec_intercept", kind, y, x, R,
                                                                               M, R, av, ab, ws, out, th),
                }
                for f in calls.values():
                    for _ in range(WARM):
                        f()
                ms = {k: [] for k in calls}
                for _ in range(REPS):
                    for k, f in calls.items():
                        ms[k].append(region_ms(c, f))
                c.profile(False)
                assert np.all(np.isfinite(c.get(out, M + 2)))
                med = {k: line(f"R={R} M={M} {NAMES[kind]} {k}", v, 8.0 * R * M) for k, v in ms.items()}
                row = 8.0 * M + (8 if kind == 1 else 4)
                for k, extra in (("vector", 8.0), ("vector + theta_adj", 16.0)):
                    print(f"R={R} M={M} {NAMES[kind]} {k} / scalar = {med[k] / med['scalar']:.3f}  "
                          f"(bytes {(row + extra) / row:.3f})", flush=True)
            c.rewind(m0)


if __name__ == "__main__":
    main()
