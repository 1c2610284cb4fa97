"""The Adam step of include/currennt_hip.h (cn_adam_update) restated in numpy, operation by operation.

With dtype float32 every numpy operation below is one IEEE operation rounded to nearest, which is what the device code is held
to (no contraction, correctly rounded square root and division, denormals kept), so the library's weights and moments must
EQUAL these bit for bit.  With dtype float64 the same statement is compared against torch.optim.Adam
(tests/test_adam_reference.py)."""
import math

import numpy as np


def adam_scalars(lr, beta1, beta2, eps, step, dtype=np.float32):
    """omb1, omb2, alpha_t, eps_t: formed in double from the arguments as `dtype` holds them, rounded once to `dtype`."""
    lr, b1, b2, eps = (float(dtype(x)) for x in (lr, beta1, beta2, eps))
    c2 = math.sqrt(1.0 - math.pow(b2, float(step)))
    c1 = 1.0 - math.pow(b1, float(step))
    return {"b1": dtype(b1), "b2": dtype(b2), "omb1": dtype(1.0 - b1), "omb2": dtype(1.0 - b2),
            "alpha_t": dtype(lr * c2 / c1), "eps_t": dtype(eps * c2)}


def adam_step(w, g, m, v, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, dtype=np.float32):
    """One update; returns the new (w, m, v).  step counts from 1."""
    s = adam_scalars(lr, beta1, beta2, eps, step, dtype)
    w, g, m, v = (np.asarray(a, dtype) for a in (w, g, m, v))
    m = s["b1"] * m + s["omb1"] * g
    v = s["b2"] * v + s["omb2"] * (g * g)
    w = w - (s["alpha_t"] * m) / (np.sqrt(v) + s["eps_t"])
    assert w.dtype == dtype and m.dtype == dtype and v.dtype == dtype
    return w, m, v


def test_gradients(rng, n, zeros=0.1):
    """Gradients of magnitude 1e-6 ... 1 with both signs and a share of exact zeros (no fp32 denormal arises from them)."""
    g = (10.0 ** rng.uniform(-6.0, 0.0, n)) * rng.choice([-1.0, 1.0], n)
    g[rng.rand(n) < zeros] = 0.0
    g = g.astype(np.float32)
    assert np.all((g == 0) | (np.abs(g) >= np.float32(1e-6)))
    return g


test_gradients.__test__ = False          # (a helper, not a test)
