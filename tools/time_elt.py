"""Timing of the element-wise maps (smg_elt_unary_* / smg_elt_binary_*) next to
smg_axpy (unchanged code: the yardstick, 16 B read and 8 B written per element)
on the same device buffers at n = 2^24, each form in its 8-byte and in its
16-byte access width (smg_elt_set_width), between HIP events recorded on the
context's stream around one call, in one process: three warm-up calls of each
form, then 21 rounds that alternate the forms and the widths.  Prints the
median (min-max), the bytes moved per element and the TB/s, and each form's
median over the yardstick's next to its byte ratio.  DESIGN.md "Element-wise
device nodes" holds the lines this printed.

    python3 tools/time_elt.py [n]
"""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from math_amd import hip  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1 << 24
REPS, WARM = 21, 3
EXP, INV_LOGIT = 0, 5
ADD, SUBTRACT, MULTIPLY = 0, 1, 2


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


def main():
    with hip.Context(0, 4 << 30) as c:
        rng = np.random.default_rng(24)
        x = c.put(rng.uniform(-6.0, 6.0, N))
        b = c.put(rng.uniform(0.5, 2.0, N))
        cadj = c.put(rng.uniform(-1e-3, 1e-3, N))
        out, aadj, badj = c.zeros(N), c.zeros(N), c.zeros(N)
        red = c.zeros(2)
        ev = Events(c)
        # (name, bytes per element, uses the width, call)
        forms = [
            ("axpy (yardstick)", 24, False, lambda: c.call("smg_axpy", N, 1e-3, x, 1, aadj, 1)),
            ("add fwd", 24, True, lambda: c.call("smg_elt_binary_fwd", ADD, x, b, 0.0, 0.0, N, out)),
            ("add rev, two adjoints", 40, True,
             lambda: c.call("smg_elt_binary_rev", ADD, x, b, 0.0, 0.0, N, cadj, aadj, badj, 0, None)),
            ("exp fwd", 16, True, lambda: c.call("smg_elt_unary_fwd", EXP, x, N, out)),
            ("inv_logit fwd", 16, True, lambda: c.call("smg_elt_unary_fwd", INV_LOGIT, x, N, out)),
            ("inv_logit rev", 32, True, lambda: c.call("smg_elt_unary_rev", INV_LOGIT, x, out, N, cadj, aadj)),
            ("elt_multiply rev", 56, True,
             lambda: c.call("smg_elt_binary_rev", MULTIPLY, x, b, 0.0, 0.0, N, cadj, aadj, badj, 0, None)),
            ("subtract(A, c) rev + scalar sum", 24, True,
             lambda: c.call("smg_elt_binary_rev", SUBTRACT, x, None, 0.0, 1.5, N, cadj, aadj, None, 2, red)),
        ]
        cases = [(name, nb, w, f) for name, nb, wide, f in forms for w in ((1, 2) if wide else (0,))]
        prev = c.lib.smg_elt_set_width(c.ptr, -1)

        def timed(w, f):
            if w:
                c.lib.smg_elt_set_width(c.ptr, w)
            return ev.ms(f)
        for _, _, w, f in cases:
            for _ in range(WARM):
                timed(w, f)
        ms = {(name, w): [] for name, _, w, _ in cases}
        for _ in range(REPS):
            for name, _, w, f in cases:
                ms[(name, w)].append(timed(w, f))
        c.lib.smg_elt_set_width(c.ptr, prev)
        assert np.all(np.isfinite(c.get(red, 2))) and np.all(np.isfinite(c.get(aadj, 1024)))
        med = {}
        label = {0: "", 1: " [8 B]", 2: " [16 B]"}
        for name, nbytes, w, _ in cases:
            v = ms[(name, w)]
            med[(name, w)] = statistics.median(v)
            print(f"n={N} {name + label[w]:40s} median {med[(name, w)]:8.4f} ms  (min {min(v):8.4f} - max {max(v):8.4f})  "
                  f"{nbytes} B/element  {nbytes * N / med[(name, w)] / 1e9:6.3f} TB/s", flush=True)
        base = med[(forms[0][0], 0)]
        for name, nbytes, w, _ in cases[1:]:
            print(f"n={N} {name + label[w]} / axpy = {med[(name, w)] / base:.3f}  (bytes {nbytes / forms[0][1]:.3f})",
                  flush=True)
        for name, _, wide, _ in forms:
            if wide:
                print(f"n={N} {name}: 16 B / 8 B = {med[(name, 2)] / med[(name, 1)]:.3f}", flush=True)


if __name__ == "__main__":
    main()
