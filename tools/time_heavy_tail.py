"""Timing of smg_cauchy_lpdf_fused and smg_student_t_lpdf_fused next to
smg_normal_lpdf_fused (unchanged code: the yardstick) on the same y, mu, sigma
device buffers and the same set of partials (y', mu' written, the scalar
sigma's reduced; a scalar nu's reduced too), at n = 2^24, by the context's
HIP-event regions of the elementwise family (one region per call of the C
entry), in one process: three warm-up calls of each form, then 21 rounds that
alternate the forms.  Prints the median (min-max), the bytes moved per element
and the TB/s, and each form's median over the yardstick's next to its byte
ratio.  DESIGN.md "Heavy-tailed densities" holds the lines this printed.

    python3 tools/time_heavy_tail.py [n]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1 << 24
REPS, WARM = 21, 3


def region_ms(ctx, call):
    ctx.profile(True)
    call()
    ms, cnt, _ = ctx.profile_read("elementwise")
    assert cnt == 1, cnt
    return ms


def main():
    with hip.Context(0, 4 << 30) as c:
        rng = np.random.default_rng(24)
        mu_h = rng.uniform(-2.0, 2.0, N)
        y = c.put(mu_h + 1.3 * rng.standard_t(2.0, N))
        mu = c.put(mu_h)
        nu = c.put(0.5 * 400.0 ** rng.uniform(0.0, 1.0, N))
        del mu_h
        gy, gmu, gnu = c.alloc(8 * N), c.alloc(8 * N), c.alloc(8 * N)
        res = c.zeros(9)
        s0, nu0 = 1.3, 4.5
        # (name, bytes per element, call): y, mu read and y', mu' written = 32 B
        forms = [
            ("normal (yardstick)", 32, lambda: c.call("smg_normal_lpdf_fused", y, mu, None, 0.0, 0.0, s0, N, 7, res, gy,
                                                      gmu, res)),
            ("cauchy", 32, lambda: c.call("smg_cauchy_lpdf_fused", y, mu, None, 0.0, 0.0, s0, N, 7, res, gy, gmu, res)),
            ("student_t scalar nu", 32, lambda: c.call("smg_student_t_lpdf_fused", y, None, mu, None, 0.0, nu0, 0.0, s0, N,
                                                       15, res, gy, res, gmu, res)),
            ("student_t vector nu", 40, lambda: c.call("smg_student_t_lpdf_fused", y, nu, mu, None, 0.0, 0.0, 0.0, s0, N,
                                                       15, res, gy, None, gmu, res)),
            ("student_t vector nu + nu'", 48, lambda: c.call("smg_student_t_lpdf_fused", y, nu, mu, None, 0.0, 0.0, 0.0, s0,
                                                             N, 15, res, gy, gnu, gmu, res)),
        ]
        for _, _, f in forms:
            for _ in range(WARM):
                f()
        ms = {name: [] for name, _, _ in forms}
        for _ in range(REPS):
            for name, _, f in forms:
                ms[name].append(region_ms(c, f))
        c.profile(False)
        assert np.all(np.isfinite(c.get(res, 9)))
        med = {}
        for name, nbytes, _ in forms:
            v = ms[name]
            med[name] = statistics.median(v)
            print(f"n={N} {name:28s} median {med[name]:8.4f} ms  (min {min(v):8.4f} - max {max(v):8.4f})  "
                  f"{nbytes} B/element  {nbytes * N / med[name] / 1e9:6.3f} TB/s", flush=True)
        base = forms[0][0]
        for name, nbytes, _ in forms[1:]:
            print(f"n={N} {name} / normal = {med[name] / med[base]:.3f}  (bytes {nbytes / forms[0][1]:.3f})", flush=True)


if __name__ == "__main__":
    main()
