"""What the six GLM log-density headers share (rev/fun/glm_common.hpp), seen
from outside: the whole what() string of every shared check at 4 rows and 2
columns, and one value and gradient per likelihood at R = 33, M = 3 (one full
32-row tile and a one-row tail) with every operand a var
(tests/cpp/test_glm_messages.cpp).

The strings below are the ones the headers threw before the shared layer was
split out; they are compared whole, with the exception type.

Values: each likelihood's logp and gradient against a float64 restatement whose
sums are taken with math.fsum (_glm_vec_intercept.vec_ref with a constant
intercept vector, _ordered.ol_ref, cat_ref below), every output within 1e-12 of
the sum of its terms' absolute values -- the bound of the other GLM tests; at
33 rows a float64 sum in any order rounds within 33 x 2^-53 = 4e-15 of that
scale and the terms themselves within a few 2^-53 of their size, so the bound
is not tight here.  The binary prints %a, so a build can also be compared with
another bit for bit.
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest
from scipy.special import gammaln

import gen
from _glm_vec_intercept import F, inputs as vec_inputs, vec_ref
from _ordered import inputs as ol_inputs, ol_ref
from _reducers import fsum_abs
from _util import ROOT, check_sums, prebuilt

gpu = pytest.mark.gpu

BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_glm_messages")
R, M, C = 33, 3, 4
ALPHA, SIGMA, PHI = 0.1, 1.3, 0.7
SIZES = ("; a function was called with arguments of different scalar, array, vector, or matrix types, and they "
         "were not consistently sized;  all arguments must be scalars or multidimensional values of the same shape.")
FNS = {"bernoulli": "bernoulli_logit_glm_lpmf", "poisson": "poisson_log_glm_lpmf", "normal": "normal_id_glm_lpdf"}


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


# ------------------------------------------------------------ 1. messages
@functools.lru_cache(maxsize=None)
def errors():
    got = {}
    for line in _run("errors\n").strip().splitlines():
        print(line)
        case, kind, msg = line.split("|", 2)
        got[case] = (kind, msg)
    return got


@gpu
@pytest.mark.parametrize("k", sorted(FNS))
def test_scalar_intercept_messages(k):
    """The y / x and beta size checks, the non-finite cascade (the intercept,
    then x) and the host-vector form's size check, whole strings."""
    e, fn = errors(), FNS[k]
    assert e[k + "_ok"][0] == "value" and math.isfinite(float(e[k + "_ok"][1]))
    assert e[k + "_y_size"] == ("invalid_argument",
                                f"{fn}: Vector of dependent variables has dimension = 3, expecting dimension = 4" + SIZES)
    assert e[k + "_beta_size"] == ("invalid_argument",
                                   f"{fn}: Weight vector has dimension = 3, expecting dimension = 2" + SIZES)
    assert e[k + "_alpha_inf"] == ("domain_error", f"{fn}: Intercept is inf, but must be finite!")
    if k == "normal":  # the sum of squares itself, under the name of x
        assert e[k + "_x_inf"] == ("domain_error", f"{fn}: Matrix of independent variables is inf, but must be finite!")
    else:
        assert e[k + "_x_inf"] == ("domain_error",
                                   f"{fn}: Matrix of independent variables is not finite, but must be finite!")
    assert e[k + "_host_x_size"] == ("invalid_argument", f"{fn}: x must hold y.size() * M values")


@gpu
def test_scale_and_remaining_messages():
    """normal_id's scale (checked before the sizes); the host-vector size check
    of the other two likelihoods; ordered has no intercept, and a non-finite x
    with finite beta goes straight to x's message."""
    e = errors()
    fn = FNS["normal"]
    assert e["normal_sigma_inf"] == ("domain_error", f"{fn}: Scale vector is inf, but must be finite!")
    assert e["normal_sigma_nan"] == ("domain_error", f"{fn}: Scale vector is nan, but must be > 0!")
    assert e["normal_sigma_before_y_size"] == e["normal_sigma_inf"]
    assert e["neg_binomial_host_x_size"] == ("invalid_argument",
                                             "neg_binomial_2_log_glm_lpmf: x must hold y.size() * M values")
    assert e["ordered_host_x_size"] == ("invalid_argument",
                                        "ordered_logistic_glm_lpmf: x must hold y.size() * M values")
    assert e["ordered_x_inf"] == ("domain_error", "ordered_logistic_glm_lpmf: Matrix of independent variables is "
                                                  "not finite, but must be finite!")
    assert e["stack"] == ("0", "0")


# ------------------------------------------------------------ 2. values
def cat_ref(y, x, alpha, beta):
    """categorical_logit: {name: (value, sum of the terms' absolute values)};
    the terms of logp are lin(i, y_i) - max and -log sum exp(lin - max) per row."""
    lin = x @ beta + alpha[None, :]
    mx = lin.max(axis=1)
    ex = np.exp(lin - mx[:, None])
    se = ex.sum(axis=1)
    hot = np.arange(beta.shape[1])[None, :] == (y - 1)[:, None]
    th = hot - ex / se[:, None]
    cols = [fsum_abs(th[:, c]) for c in range(th.shape[1])]
    bt = [fsum_abs(x[:, m] * th[:, c]) for c in range(th.shape[1]) for m in range(x.shape[1])]
    return {"logp": fsum_abs(np.concatenate([lin[hot] - mx, -np.log(se)])),
            "alpha'": (np.array([v[0] for v in cols]), np.array([v[1] for v in cols])),
            "beta'": (np.array([v[0] for v in bt]), np.array([v[1] for v in bt]))}


@functools.lru_cache(maxsize=None)
def values():
    """One run of the binary's "values" mode: ({likelihood: [fx, grad...]}, the inputs)."""
    x, y01, beta, _ = vec_inputs(0, R, M)
    yreal, ycount = vec_inputs(1, R, M)[1], vec_inputs(2, R, M)[1]
    _, yclass, _, cuts = ol_inputs(R, M, C)
    alphaC = gen.unif(gen.SEED + 401, C, -0.5, 0.5)
    betaC = gen.unif(gen.SEED + 402, M * C, -1.0, 1.0).reshape(C, M).T.copy()
    nums = np.concatenate([F(x), beta, [ALPHA, SIGMA, PHI], y01, yreal, ycount, yclass, alphaC, F(betaC), cuts])
    out = _run(f"values {R} {M} {C}\n" + " ".join(repr(float(v)) for v in nums) + "\n")
    res = {}
    for line in out.strip().splitlines():
        print(line)
        tag, *vals = line.split()
        res[tag] = np.array([float.fromhex(v) for v in vals])
    return res, dict(x=x, y01=y01, yreal=yreal, ycount=ycount, yclass=yclass, beta=beta, alphaC=alphaC, betaC=betaC,
                     cuts=cuts)


def _check_logp(what, fx, terms):
    """fx against the sum of (value, abs) terms, on the scale of their absolute sum."""
    want, scale = sum(t[0] for t in terms), sum(t[1] for t in terms)
    print(f"{what} logp: |diff| / abs-term sum = {abs(fx - want) / scale:.3e}")
    assert abs(fx - want) <= 1e-12 * scale, (what, fx, want)


@gpu
@pytest.mark.parametrize("kind,name", [(0, "bernoulli_logit"), (1, "normal_id"), (2, "poisson_log"),
                                       (3, "neg_binomial_2_log")])
def test_row_wise_values(kind, name):
    """[alpha', beta'(M), sigma' | phi'] and logp composed from the pass's sums."""
    r, d = values()
    y = d[{0: "y01", 1: "yreal", 2: "ycount", 3: "ycount"}[kind]]
    extra = {1: SIGMA, 3: PHI}.get(kind)
    ref, _, _ = vec_ref(kind, y, d["x"], np.full(R, ALPHA), d["beta"], extra)
    o = r[name]
    assert len(o) == 1 + 1 + M + (extra is not None)
    check_sums({"alpha'": o[1], "beta'": o[2:M + 2]}, ref, name, b_rel=None)
    neg = lambda t: (-t[0], t[1])  # noqa: E731
    if kind == 0:
        _check_logp(name, o[0], [ref["value"]])
    elif kind == 2:
        _check_logp(name, o[0], [ref["value"], neg(ref["lgamma"])])
    elif kind == 1:
        sq, sq_abs = ref["value"]
        norm = -0.5 * math.log(2 * math.pi) * R - R * math.log(SIGMA)
        _check_logp(name, o[0], [(norm, abs(norm)), (-0.5 * sq, 0.5 * sq_abs)])
        assert abs(o[M + 2] - (sq - R) / SIGMA) <= 1e-12 * (sq_abs + R) / SIGMA
    else:
        norm = R * (PHI * math.log(PHI) - gammaln(PHI))
        _check_logp(name, o[0], [neg(ref["C"]), (norm, abs(norm)), ref["D"], ref["B"], neg(ref["A"])])
        check_sums({"phi'": o[M + 2]}, ref, name)


@gpu
def test_categorical_and_ordered_values():
    r, d = values()
    o = r["categorical_logit"]
    assert len(o) == 1 + C + M * C
    check_sums({"logp": o[0], "alpha'": o[1:C + 1], "beta'": o[C + 1:]},
               cat_ref(d["yclass"], d["x"], d["alphaC"], d["betaC"]), "categorical_logit", b_rel=None)
    o = r["ordered_logistic"]
    assert len(o) == 1 + M + (C - 1)
    check_sums({"logp": o[0], "beta'": o[1:M + 1], "cuts'": o[M + 1:]},
               ol_ref(d["yclass"], d["x"], d["beta"], d["cuts"]), "ordered_logistic", b_rel=None)
    assert list(r["stack"]) == [0.0, 0.0]
