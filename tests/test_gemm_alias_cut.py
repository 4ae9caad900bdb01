"""The GEMM's general aliasing path with an offset K cut (smg_gemm_cut with C
aliasing an operand and n > 64): the product goes out of place through a
workspace, and that product must keep the cut of the call.  Inputs, bound and
helpers are test_gemm_kcut's.

Kernel reached: (192, 192, 192) NN full with C = A -- the product into the
workspace on 32 x 32 tiles, 8 waves, split over K in three, in both stage
modes (a product into the workspace never takes the DMA kernel).
"""
import numpy as np
import pytest

from test_gemm_dma_stage import View, backing, gamma
from test_gemm_kcut import _rewind, ctx, declared, reference, run, with_nan  # noqa: F401 (fixtures)


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [1, 2])
def test_aliased_product_keeps_cut(ctx, stage):  # noqa: F811
    """C aliases A in an NN full product with n > 64, cut_b = 64, NaN in the
    declared-zero 64-block of B: the result is finite, inside the gamma_K
    bound of numpy, and bit-equal to the same product run out of place (C
    there holding a copy of A) through the register-staged kernels.  The
    out-of-place product of stage mode 2 is the DMA kernel's, another
    summation order (28163 of the 36864 elements differ from it in their last
    bits), which is why the reference product runs in stage mode 1."""
    m = n = k = 192
    cut = 64
    rng = np.random.default_rng(192064)
    A = View(backing(rng, m + 128, k + 64), 64, 64, m, k)
    B = View(backing(rng, k + 64, n + 64), 64, 0, k, n)
    zero, blocks = declared(n, k, cut)
    B.a[zero.T] = 0.0
    assert blocks.sum() == 64 * 64
    Bn = with_nan(B, blocks.T)
    for alpha, beta in ((1.5, 0.0), (-1.0, 1.0), (1.5, -0.5)):
        got = run(ctx, stage, "NN-full", m, n, k, alpha, A, Bn, beta, A, cut_b=cut)
        assert np.isfinite(got).all()
        blk = got[A.r0:A.r0 + m, A.c0:A.c0 + n]
        bound = 2.0 * gamma(k) * (abs(alpha) * (np.abs(A.a) @ np.abs(B.a)) + abs(beta) * np.abs(A.a))
        err = np.abs(blk - reference(A.a, B.a, A.a, alpha, beta, 0))
        assert np.all(err <= bound), float((err / bound).max())
        mask = np.ones(A.back.shape, bool)
        mask[A.r0:A.r0 + m, A.c0:A.c0 + n] = False
        assert np.array_equal(got[mask], A.back[mask])
        out = run(ctx, 1, "NN-full", m, n, k, alpha, A, Bn, beta, View(A.back.copy(), A.r0, A.c0, m, n), cut_b=cut)
        assert np.array_equal(got, out), int((got != out).sum())
