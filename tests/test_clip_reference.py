"""tests/clip_reference.py -- the numpy statement the GPU tests hold the library to -- against exact arithmetic (CPU only)."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as AR          # noqa: E402
import clip_reference as CR          # noqa: E402

L = CR.L


@pytest.mark.parametrize("n", [1, L - 1, L, L + 1, 5 * L + 3])
def test_clip_sum_is_the_sum_of_the_exact_squares(n):
    g = AR.test_gradients(np.random.RandomState(n % 1000), n)
    exact = math.fsum(float(x) * float(x) for x in g)          # (a float32 squared is exact in double; fsum rounds once)
    s = CR.clip_sum(g)
    assert exact > 0
    assert abs(s - exact) <= exact * 2.0 ** -40, (s, exact)


def test_the_order_is_lanes_then_neighbours():
    """lane 0 holds entries 0 and L, lane 1 entry 1: S = ((g[0]^2 + g[L]^2) + g[1]^2), not g[0]^2 + (g[L]^2 + g[1]^2)"""
    g = np.zeros(L + 2, np.float32)
    g[0] = 1.0
    g[1] = g[L] = np.float32(2.0 ** -26.5)
    q = float(g[1]) ** 2                        # just above 2^-53: 1 + q rounds up to 1 + 2^-52, and so does the next add
    assert (1.0 + q) + q != 1.0 + (q + q)
    assert CR.clip_sum(g) == (1.0 + q) + q


def test_scaled_gradient_has_norm_at_most_the_bound():
    rng = np.random.RandomState(3)
    for n, share in ((8, 0.5), (L + 1, 1e-3), (5 * L + 3, 0.97)):
        g = AR.test_gradients(rng, n)
        bound = np.float32(share) * CR.clip_factor(g, 0.0)[0]
        gc, norm, scale, skip = CR.clipped(g, bound)
        assert not skip and scale is not None and norm > np.float32(bound)
        exact = math.sqrt(math.fsum(float(x) * float(x) for x in gc))
        assert exact <= float(np.float32(bound)) * (1.0 + 2.0 ** -20), (exact, bound)


def test_a_bound_above_the_norm_means_no_multiplication():
    g = AR.test_gradients(np.random.RandomState(4), 1000)
    norm, scale, skip = CR.clip_factor(g, 1e9)
    assert scale is None and not skip
    norm2, scale2, _ = CR.clip_factor(g, norm)                  # at the bound exactly: still none
    assert scale2 is None and norm2 == norm
    gc, _, _, _ = CR.clipped(g, 1e9)
    assert gc.tobytes() == g.tobytes()
    w = np.linspace(-1, 1, 1000).astype(np.float32)
    d = np.zeros(1000, np.float32)
    a = CR.clip_sgd_step(w, g, d, 1e-2, 0.9, 1e9)
    b = CR.sgd_step(w, g, d, 1e-2, 0.9)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_entries_skip_the_step(bad):
    g = AR.test_gradients(np.random.RandomState(5), L + 7)
    g[L + 3] = bad
    norm, scale, skip = CR.clip_factor(g, 1.0)
    assert skip and scale is None
    w = np.ones(g.size, np.float32)
    z = np.zeros(g.size, np.float32)
    w2, d2, _, _, sk = CR.clip_sgd_step(w, g, z, 0.1, 0.9, 1.0)
    assert sk and w2.tobytes() == w.tobytes() and d2.tobytes() == z.tobytes()
    w3, m3, v3, _, _, sk = CR.clip_adam_step(w, g, z, z, [(0, g.size, 1e-3)], 1.0)
    assert sk and w3.tobytes() == w.tobytes() and m3.tobytes() == z.tobytes() and v3.tobytes() == z.tobytes()


def test_squares_that_overflow_fp32_do_not_skip():
    """3e19^2 = 9e38 is beyond fp32 (3.4e38) and far inside double: the reason the sum is formed in double"""
    g = np.full(8, 3e19, np.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(g[0] * g[0])
    gc, norm, scale, skip = CR.clipped(g, 1.0)
    assert not skip and scale is not None and np.isfinite(norm)
    exact = Fraction(float(g[0])) ** 2 * 8
    assert abs(Fraction(float(norm)) ** 2 / exact - 1) < Fraction(1, 2 ** 22)
    assert np.all(np.isfinite(gc))
    assert abs(math.sqrt(math.fsum(float(x) ** 2 for x in gc)) - 1.0) <= 2.0 ** -20
