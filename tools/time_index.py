"""Timing of smg_gather and smg_segment_sum next to smg_axpy (unchanged code:
the yardstick, 16 B read and 8 B written per element) at R = 2^24 rows, between
HIP events recorded on the context's stream around one call (smg_segment_sum's
two launches are inside one pair), in one process: three warm-up calls of each
form, then 21 rounds that alternate all forms.  Groupings: J in {16, 2^10,
2^20} with g sorted and shuffled, and the skewed one (J = 2^10, destination 1
holding half the rows, shuffled).  Prints the median (min-max) of each form,
its ratio to the yardstick, and per kernel the largest ratio between two
groupings at equal R, and between the three sorted shapes of the balance claim
(one destination, R singletons, half the rows in one among singletons: the
same streaming reads, so only the shape differs).  Then what the plain
launches cost, at sizes where the kernels' own work is small (`launches`).

Then the hierarchical Poisson GLM end to end (tests/cpp/_bin/test_index_ops,
mode bench: R = 10^6, M = 8, J = 1000): gradient evaluations per second of the
device form (gather) and of the host-vari form (alpha a std::vector<var>),
alternating in one process, medians and ranges.  DESIGN.md "Indexing by
group" holds the lines this printed.

    python3 tools/time_index.py [R] [bench reps] [kernels | launches | model ...]
"""
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402

R = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1 << 24
BENCH_REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
PARTS = sys.argv[3:] or ["kernels", "launches", "model"]
REPS, WARM = 21, 3
BALANCE = ("one destination, sorted", "R singletons, sorted", "half the rows in one among singletons, sorted")


class Events:
    """A pair of HIP events on the context's stream."""

    def __init__(self, ctx):
        self.rt = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.stream = ctypes.c_void_p(ctx.lib.smg_ctx_stream(ctx.ptr))
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            assert self.rt.hipEventCreate(ctypes.byref(e)) == 0

    def ms(self, call):
        assert self.rt.hipEventRecord(self.a, self.stream) == 0
        call()
        assert self.rt.hipEventRecord(self.b, self.stream) == 0
        assert self.rt.hipEventSynchronize(self.b) == 0
        t = ctypes.c_float()
        assert self.rt.hipEventElapsedTime(ctypes.byref(t), self.a, self.b) == 0
        return float(t.value)


def groupings(rng):
    """[(name, g, J)]"""
    out = []
    for J in (16, 1 << 10, 1 << 20):
        g = np.sort(rng.integers(1, J + 1, R, dtype=np.int32))
        out.append((f"J={J} sorted", g, J))
        out.append((f"J={J} shuffled", rng.permutation(g), J))
    J = 1 << 10
    g = rng.integers(2, J + 1, R, dtype=np.int32)
    g[rng.permutation(R)[:R // 2]] = 1
    out.append((f"J={J} skewed, half the rows in one", g, J))
    # the three shapes of the balance claim, all in sorted order (the same streaming reads)
    out.append((BALANCE[0], np.ones(R, dtype=np.int32), 1))
    out.append((BALANCE[1], np.arange(1, R + 1, dtype=np.int32), R))
    half = R // 2
    out.append((BALANCE[2], np.concatenate([np.ones(half, dtype=np.int32), np.arange(2, R - half + 2, dtype=np.int32)]),
                R - half + 1))
    return out


def kernels():
    with hip.Context(0, 8 << 30) as c:
        rng = np.random.default_rng(24)
        ev = Events(c)
        x = c.put(rng.uniform(-1.0, 1.0, R))
        y = c.zeros(R)
        forms = [("axpy (yardstick)", "axpy", lambda: c.call("smg_axpy", R, 1e-3, x, 1, y, 1))]
        for name, g, J in groupings(rng):
            perm = np.argsort(g, kind="stable").astype(np.int32)
            offs = np.concatenate([[0], np.cumsum(np.bincount(g - 1, minlength=J))]).astype(np.int64)
            gd, pd, od = c.put(g), c.put(perm), c.put(offs)
            u, out = c.put(rng.uniform(-1.0, 1.0, J)), c.zeros(J)
            ws = c.zeros(int(c.lib.smg_segment_sum_ws_doubles(R, J)))
            forms += [
                (f"gather {name}", "gather", lambda u=u, gd=gd: c.call("smg_gather", u, gd, R, 0, y)),
                (f"gather accumulating {name}", "gather accumulating",
                 lambda u=u, gd=gd: c.call("smg_gather", u, gd, R, 1, y)),
                (f"segment_sum accumulating {name}", "segment_sum accumulating",
                 lambda pd=pd, od=od, J=J, ws=ws, out=out: c.call("smg_segment_sum", x, pd, od, R, J, 1, ws, out)),
                (f"segment_sum {name}", "segment_sum",
                 lambda pd=pd, od=od, J=J, ws=ws, out=out: c.call("smg_segment_sum", x, pd, od, R, J, 0, ws, out)),
            ]
        for _, _, f in forms:
            for _ in range(WARM):
                ev.ms(f)
        ms = {name: [] for name, _, _ in forms}
        for _ in range(REPS):
            for name, _, f in forms:
                ms[name].append(ev.ms(f))
        assert np.all(np.isfinite(c.get(y, 1024)))
        med = {}
        for name, _, _ in forms:
            v = ms[name]
            med[name] = statistics.median(v)
            print(f"R={R} {name:62s} median {med[name]:8.4f} ms  (min {min(v):8.4f} - max {max(v):8.4f})", flush=True)
        base = med[forms[0][0]]
        for name, _, _ in forms[1:]:
            print(f"R={R} {name} / axpy = {med[name] / base:.3f}", flush=True)
        for kind in ("gather", "gather accumulating", "segment_sum accumulating", "segment_sum"):
            m = {name: med[name] for name, k, _ in forms if k == kind}
            lo, hi = min(m, key=m.get), max(m, key=m.get)
            print(f"R={R} {kind}: slowest / fastest grouping = {m[hi] / m[lo]:.3f}  ({hi} / {lo})", flush=True)
            m = {b: med[f"{kind} {b}"] for b in BALANCE}
            lo, hi = min(m, key=m.get), max(m, key=m.get)
            print(f"R={R} {kind}: slowest / fastest of the three sorted shapes = {m[hi] / m[lo]:.3f}  ({hi} / {lo})",
                  flush=True)


def launches():
    """What the plain launches cost: at sizes where the kernels' own work is
    small, smg_gather (one launch) next to smg_segment_sum with one tile (two
    launches: the tiles' first destinations, the tile kernel) and with four
    tiles (three: the combine step too), J = 7, 201 rounds alternating."""
    with hip.Context(0, 1 << 28) as c:
        T = (ctypes.c_int * 5)()
        assert c.lib.smg_index_launch_shape(c.ptr, T) == 0
        T = T[1]
        rng = np.random.default_rng(7)
        ev = Events(c)
        forms = []
        for n, what in ((T, "one tile: two launches"), (3 * T + 5, "four tiles: three launches")):
            g = rng.integers(1, 8, n, dtype=np.int32)
            perm = np.argsort(g, kind="stable").astype(np.int32)
            offs = np.concatenate([[0], np.cumsum(np.bincount(g - 1, minlength=7))]).astype(np.int64)
            gd, pd, od = c.put(g), c.put(perm), c.put(offs)
            x, y, u, out = c.put(rng.uniform(-1.0, 1.0, n)), c.zeros(n), c.put(rng.uniform(-1.0, 1.0, 7)), c.zeros(7)
            ws = c.zeros(int(c.lib.smg_segment_sum_ws_doubles(n, 7)))
            forms += [
                (f"R={n} gather accumulating (one launch)", lambda u=u, gd=gd, n=n, y=y: c.call("smg_gather", u, gd, n, 1, y)),
                (f"R={n} segment_sum accumulating ({what})",
                 lambda x=x, pd=pd, od=od, n=n, ws=ws, out=out: c.call("smg_segment_sum", x, pd, od, n, 7, 1, ws, out)),
            ]
        for _, f in forms:
            for _ in range(WARM):
                ev.ms(f)
        ms = {name: [] for name, _ in forms}
        for _ in range(201):
            for name, f in forms:
                ms[name].append(ev.ms(f))
        for name, _ in forms:
            v = ms[name]
            print(f"{name:62s} median {1e3 * statistics.median(v):8.2f} us  (min {1e3 * min(v):8.2f} - max "
                  f"{1e3 * max(v):8.2f})", flush=True)


def model():
    from math_amd import srchash
    binary = os.path.join(ROOT, "tests", "cpp", "_bin", "test_index_ops")
    srchash.check(binary, "cpp:test_index_ops")
    Rm, J, M = 1000000, 1000, 8
    p = subprocess.run([binary], input=f"bench {Rm} {J} {M} {BENCH_REPS}\n", capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    res = {}
    for ln in p.stdout.strip().splitlines():
        tag, _, vals = ln.partition(" ")
        res[tag] = [float(v) for v in vals.split()]
    for tag, what in (("ms_dev", "device form (gather)"), ("ms_host", "host-vari form (std::vector<var> alpha)")):
        v = res[tag]
        m = statistics.median(v)
        print(f"hierarchical poisson_log GLM R={Rm} M={M} J={J} {what:42s} median {m:9.3f} ms  (min {min(v):9.3f} - max "
              f"{max(v):9.3f})  {1e3 / m:8.2f} evals/s  ({1e3 / max(v):.2f} - {1e3 / min(v):.2f})", flush=True)
    print(f"hierarchical poisson_log GLM host / device = "
          f"{statistics.median(res['ms_host']) / statistics.median(res['ms_dev']):.2f}; largest gradient difference / "
          f"largest entry = {res['gradient_diff'][0]:.3e}", flush=True)


if __name__ == "__main__":
    for part in PARTS:
        {"kernels": kernels, "launches": launches, "model": model}[part]()
