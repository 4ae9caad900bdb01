"""Raw outputs of the rectangular GP entries, for a bit-for-bit comparison of
two builds of the library: smg_gp_cross_cov_fwd / _rev (the four families),
smg_gp_periodic_cov_fwd / _rev and smg_gp_dot_prod_cov_fwd / _rev at the
shapes of SCALAR and POINTS in tests/test_gp_cross.py and
tests/test_gp_periodic.py, plus (300, 257, 70) for the dot product.  K is
written into a NaN-filled buffer of leading dimension ldk and dumped whole;
the adjoint's padding rows are NaN; the reverse's output is pre-loaded.

    python3 tools/gp_rect_bits.py dump OUT.npz [ROOT]   # ROOT: the tree whose math_amd is loaded (default: this one)
    python3 tools/gp_rect_bits.py compare A.npz B.npz   # one line per entry and shape; exit status 1 on a difference
"""
import os
import sys

import numpy as np

# (n1, n2, D, ld)
CROSS = [(1, 1, 1, 1), (1, 7, 1, 1), (7, 1, 1, 7), (33, 20, 1, 33), (33, 20, 1, 36), (300, 257, 1, 300),
         (300, 257, 1, 303), (5, 2050, 1, 5), (2050, 5, 1, 2050), (2050, 5, 1, 2053),
         (1, 3, 3, 1), (33, 20, 3, 33), (33, 20, 3, 36), (300, 7, 5, 300), (7, 2051, 3, 7), (64, 9, 200, 64)]
PERIODIC = [(33, 20, 1, 33), (300, 257, 1, 300), (300, 257, 1, 301), (299, 20, 1, 299), (5000, 3, 1, 5000),
            (3, 2100, 1, 3), (33, 20, 3, 33), (300, 257, 5, 300)]
DOT = PERIODIC + [(300, 257, 70, 300)]
SIG, ELL, PER = 1.3, 0.9, 1.7
PRE = np.array([0.25, -0.5, 0.75])


def dump(path, root):
    sys.path.insert(0, root)
    from math_amd import hip
    out = {}
    with hip.Context(0, 1 << 30) as c:
        def run(tag, shape, fwd, rev, nout):
            n1, n2, D, ld = shape
            rng = np.random.default_rng(1000003 * n1 + 1009 * n2 + 17 * D + ld)
            half = 4.4 / np.sqrt(D)
            x1, x2 = rng.uniform(-half, half, n1 * D), rng.uniform(-half, half, n2 * D)
            A = np.full((n2, ld), np.nan)
            A[:, :n1] = rng.uniform(-1, 1, (n2, n1))
            m = c.mark()
            d1, d2 = c.put(x1), c.put(x2)
            dK, dA, do = c.put(np.full(ld * n2, np.nan)), c.put(A.ravel()), c.put(PRE[:nout])
            assert fwd(d1, n1, d2, n2, D, dK, ld) == 0
            assert rev(d1, n1, d2, n2, D, dA, ld, do) == 0
            key = f"{tag} n1={n1} n2={n2} D={D} ld={ld}"
            out[key + " fwd"] = c.get(dK, ld * n2)
            out[key + " rev"] = c.get(do, nout)
            assert c.status() == 0
            c.rewind(m)

        L, P = c.lib, c.ptr
        for fam in range(4):
            for s in CROSS:
                run(f"cross family {fam}", s,
                    lambda a, n1, b, n2, D, K, ld: L.smg_gp_cross_cov_fwd(P, fam, a, n1, b, n2, D, SIG, ELL, K, ld),
                    lambda a, n1, b, n2, D, A, ld, o: L.smg_gp_cross_cov_rev(P, fam, a, n1, b, n2, D, SIG, ELL, A, ld, o),
                    2)
        for s in PERIODIC:
            run("periodic", s,
                lambda a, n1, b, n2, D, K, ld: L.smg_gp_periodic_cov_fwd(P, a, n1, b, n2, D, SIG, ELL, PER, K, ld),
                lambda a, n1, b, n2, D, A, ld, o: L.smg_gp_periodic_cov_rev(P, a, n1, b, n2, D, SIG, ELL, PER, A, ld, o),
                3)
        for s in DOT:
            run("dot product", s,
                lambda a, n1, b, n2, D, K, ld: L.smg_gp_dot_prod_cov_fwd(P, a, n1, b, n2, D, SIG, K, ld),
                lambda a, n1, b, n2, D, A, ld, o: L.smg_gp_dot_prod_cov_rev(P, n1, n2, SIG, A, ld, o), 1)
    np.savez(path, **out)
    print(f"{len(out)} outputs of {hip.LIB_PATH} -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files)
    bad = 0
    for k in a.files:
        same = a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))
        bad += not same
        print(f"{k:52s} {a[k].size:8d} doubles  {'bit-equal' if same else 'DIFFERENT'}")
    print(f"{len(a.files)} outputs compared (raw bits, NaN padding included), {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
        dump(sys.argv[2], os.path.abspath(sys.argv[3] if len(sys.argv) > 3 else here))
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
