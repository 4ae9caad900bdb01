"""Large device adjoints are zeroed when their first dense user appears.

The tape registers an adjoint buffer of 2^17 elements or more unzeroed
(rev/core/grad.hpp) and zeroes it when a node that adds into it densely is
constructed, when expand_adjoint() or a host read needs it, or in
set_zero_all_adjoints.  Under the closed-form reverse of the GP marginal the
N^2 adjoints of K, K + dI and L are neither written nor read, so they are never
zeroed; wherever they are used, the results are those of the build that zeroed
every buffer at registration (tests/golden/lazy_adjoint_clear_parent.json,
written by that build from tests/cpp/test_lazy_adjoint_clear.cpp's commands).

Tolerances: the gradient against the reference's at the suite's 1e-10.  Against
the parent build's dump 1e-12 relative with a 1e-12 * max-norm floor: the same
kernels add the same terms into buffers that hold the same zeros, so only the
order of floating-point atomics inside a reduction can differ between runs.
"""
import os
import subprocess

import numpy as np
import pytest

from _util import ROOT, golden, near_rel, prebuilt

BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_lazy_adjoint_clear")
RTOL = 1e-10
SAME = 1e-12


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = {}
    for line in p.stdout.strip().splitlines():
        tag, *vals = line.split()
        res[tag] = np.array([float(v) for v in vals])
    return res


def _num(vals):
    return " ".join(repr(float(v)) for v in np.ravel(vals))


def _same_as_parent(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.all(np.isfinite(got)), what
    near_rel(got, want, SAME, atol=SAME * float(np.abs(want).max()), what=what)


def _stats_same(got, want, what):
    """[head, sum, abs_sum, l2, samples...]: the sums against the magnitude sum."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.all(np.isfinite(got)), what
    near_rel(got[0], want[0], SAME, what=what + " value")
    near_rel(got[1], want[1], SAME, atol=SAME * float(want[2]), what=what + " sum")
    near_rel(got[2:4], want[2:4], SAME, what=what + " abs sum, l2")
    near_rel(got[4:], want[4:], SAME, atol=SAME * float(np.abs(want[4:]).max()), what=what + " samples")


@pytest.mark.gpu
def test_unread_adjoints_are_never_cleared():
    """The GP closed-form gradient at N = 1024, twice (the second evaluation on
    the predicted closed form), each from an arena filled with NaN: the bytes
    zeroed per evaluation stay below one N^2 buffer, so none of the adjoints of
    K, K + dI and L was cleared -- and none was read, or the NaN would show."""
    N = 1024
    d = golden(f"gp_N{N}")
    res = _run(f"unread {N} 2 {_num(d['x'])} {_num(d['y'])} {_num(d['theta'])}\n")
    for r in range(2):
        got = res[f"unread_{r}"]
        print(f"evaluation {r}: {int(got[4])} bytes zeroed (one N^2 adjoint: {N * N * 8})")
        near_rel(got[0], d["fx"], 1e-12, what=f"fx {r}")
        near_rel(got[1:4], d["grad"], RTOL, what=f"grad {r}")
        assert got[4] < N * N * 8, (r, got[4])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_read_adjoints_are_cleared(variant):
    """The same model with K's, K + dI's and L's adjoints read after the sweep
    (variant 0: expand_adjoint writes the deposits densely) and with sum(L) as
    a second writer of L's adjoint (variant 1: the dense reverse), from a
    NaN-filled arena: all three buffers are zeroed, and the hyperparameter
    gradient and the three adjoints are the parent build's."""
    N = 1024
    d, want = golden(f"gp_N{N}"), golden("lazy_adjoint_clear_parent")
    res = _run(f"read {N} {variant} {_num(d['x'])} {_num(d['y'])} {_num(d['theta'])}\n")
    print(f"variant {variant}: {int(res['zeroed'][0])} bytes zeroed")
    assert res["zeroed"][0] >= 3 * N * N * 8
    if variant == 0:
        near_rel(res["theta"][0], d["fx"], 1e-12, what="lp vs reference")
        near_rel(res["theta"][1:], d["grad"], RTOL, what="grad theta vs reference")
    _same_as_parent(res["theta"], want[f"read_v{variant}_theta"], "lp, grad theta")
    for name in ("K", "Kd", "L"):
        _stats_same(res[name], want[f"read_v{variant}_{name}"], name + " adjoint")


@pytest.mark.gpu
def test_sum_cholesky_clears_and_matches_parent():
    """sum(cholesky_decompose(A)) at N = 512 (262144 elements: above the
    threshold), twice: the first evaluation zeroes A's and L's adjoints in the
    sweep, the second -- the dense reverse now on record for that tape position
    -- when the factorisation is constructed; both give the parent's gradient."""
    N = 512
    want = golden("lazy_adjoint_clear_parent")
    res = _run(f"mulchol {N} 2\n")
    for r in range(2):
        print(f"evaluation {r}: {int(res[f'zeroed_{r}'][0])} bytes zeroed")
        assert res[f"zeroed_{r}"][0] >= 2 * N * N * 8
        _stats_same(res[f"mulchol_{r}"], want["mulchol"], f"gradient {r}")


@pytest.mark.gpu
def test_set_zero_all_adjoints_then_second_grad():
    """grad(), set_zero_all_adjoints(), grad() on one tape of the GP at
    N = 1024: the same gradient twice, the reference's."""
    N = 1024
    d = golden(f"gp_N{N}")
    res = _run(f"setzero {N} {_num(d['x'])} {_num(d['y'])} {_num(d['theta'])}\n")
    for tag in ("first", "second"):
        near_rel(res[tag][0], d["fx"], 1e-12, what=tag + " lp")
        near_rel(res[tag][1:], d["grad"], RTOL, what=tag + " grad")
    near_rel(res["second"], res["first"], SAME, what="second vs first")
