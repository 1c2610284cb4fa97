"""NumPy model of the CTC post output layer (csrc/cn_ctc.hip), in the rescaled form the kernels use, runnable in float64 and
float32.

One sequence: y [len][C] posteriors, labels l[0..U) in [0, C-2], blank = C-1, extended sequence l' = (b, l0, b, ..., b),
S = 2U + 1.  A probability of the sweeps is a pair (m, k) = m * 2^k, m in [0.5, 1) of the working precision, k an integer per
state; zero is (0, KMIN).  A sum of pairs aligns to the largest exponent K, (ldexp(m0, k0-K) + ldexp(m1, k1-K)) + ldexp(m2, k2-K);
norm(x, K) = (frexp mantissa, K + frexp exponent).
    a_t(s) = norm(y_t(l'_s) * sum, K)  of a_{t-1}(s), a_{t-1}(s-1), [skip] a_{t-1}(s-2)
    (m, K) = a_{len-1}(S-1) + a_{len-1}(S-2);   -log p = -(K ln 2 + log m)
    b_t(s) = norm(sum, K)  of q_{t+1}(s), q_{t+1}(s+1), [skip] q_{t+1}(s+2);   q_t(s) = norm(m_b y_t(l'_s), k_b)
    gamma_t(s) = a_t(s) b_t(s) / sum_s a_t(s) b_t(s)          dL/dy_k(t) = -(sum_{s: l'_s = k} gamma_t(s)) / y_k(t)
A sequence is infeasible when len = 0 or U + (adjacent repeats) > len: loss 0, zero gradient, flag False.  So is one whose p
is 0.
"""
import numpy as np

KMIN = -(1 << 28)


def _norm(x, K):
    m, e = np.frexp(x)
    return m, np.where(x > 0, K + e, KMIN).astype(np.int64)


def _ldexp(m, shift):
    """m * 2^shift in m's precision (shifts far below the format's range give 0)."""
    return np.ldexp(m, np.maximum(shift, -100000)).astype(m.dtype)


def _sum3(p0, p1, p2, third):
    """Pairs (m, k) of arrays; `third`: bool array, where p2 takes part.  Returns (sum, K)."""
    K = np.maximum(p0[1], p1[1])
    K = np.where(third, np.maximum(K, p2[1]), K)
    with np.errstate(under="ignore", over="ignore"):          # (over: a third pair that does not take part, dropped below)
        v = _ldexp(p0[0], p0[1] - K) + _ldexp(p1[0], p1[1] - K)
        v = np.where(third, v + _ldexp(p2[0], p2[1] - K), v)
    return v, K


def ctc_sequence(y, labels, dtype=np.float64):
    """y: [len][C]; labels: ints.  Returns (loss, dL/dy [len][C], feasible) computed in `dtype`."""
    y = np.asarray(y, dtype)
    T, C = y.shape
    labels = [int(k) for k in labels]
    U = len(labels)
    S = 2 * U + 1
    grad = np.zeros((T, C), dtype)
    repeats = sum(1 for u in range(1, U) if labels[u] == labels[u - 1])
    if T == 0 or U + repeats > T:
        return dtype(0), grad, False
    ext = np.full(S, C - 1, np.int64)
    ext[1::2] = labels
    skip_a = np.zeros(S, bool)                      # s-2 -> s allowed
    skip_a[3::2] = ext[3::2] != ext[1:-2:2]
    skip_b = np.zeros(S, bool)                      # s -> s+2 allowed, seen from s
    skip_b[:-2] = skip_a[2:]
    zm, zk = np.zeros(2, dtype), np.full(2, KMIN, np.int64)

    am, ak = np.zeros((T, S), dtype), np.full((T, S), KMIN, np.int64)
    am[0, :2], ak[0, :2] = _norm(y[0, ext[:2]], 0)
    for t in range(1, T):
        m, k = np.concatenate([zm, am[t - 1]]), np.concatenate([zk, ak[t - 1]])
        sm, K = _sum3((m[2:], k[2:]), (m[1:-1], k[1:-1]), (m[:-2], k[:-2]), skip_a)
        am[t], ak[t] = _norm(y[t, ext] * sm, K)
    last = (am[T - 1, S - 1:], ak[T - 1, S - 1:])
    prev = (am[T - 1, S - 2:S - 1], ak[T - 1, S - 2:S - 1]) if S > 1 else (zm[:1], zk[:1])
    fin, K = _sum3(last, prev, prev, np.zeros(1, bool))
    if not fin[0] > 0:
        return dtype(0), grad, False
    loss = -(dtype(K[0]) * dtype(np.log(2.0)) + np.log(fin[0]))

    bm, bk = np.zeros((T, S), dtype), np.full((T, S), KMIN, np.int64)
    bm[T - 1, max(S - 2, 0):], bk[T - 1, max(S - 2, 0):] = 0.5, 1
    for t in range(T - 2, -1, -1):
        qm, qk = _norm(bm[t + 1] * y[t + 1, ext], bk[t + 1])
        m, k = np.concatenate([qm, zm]), np.concatenate([qk, zk])
        sm, K = _sum3((m[:-2], k[:-2]), (m[1:-1], k[1:-1]), (m[2:], k[2:]), skip_b)
        bm[t], bk[t] = _norm(sm, K)

    pk = ak + bk
    with np.errstate(under="ignore"):
        prod = _ldexp(am * bm, pk - pk.max(axis=1, keepdims=True))
    tot = prod.sum(axis=1, dtype=dtype)
    for t in range(T):
        g = np.zeros(C, dtype)
        np.add.at(g, ext, prod[t])
        nz = g > 0
        grad[t, nz] = -(g[nz] / tot[t]) / y[t, nz]
    return dtype(loss), grad, True


def ctc_fraction(y, pat, labels, dtype=np.float64):
    """y [T][PS][C], pat [T][PS], labels: one list per slot.  Returns (loss [PS], dL/dy [T][PS][C], feasible [PS])."""
    y = np.asarray(y)
    T, PS, C = y.shape
    pat = np.asarray(pat).reshape(T, PS)
    loss = np.zeros(PS, dtype)
    grad = np.zeros((T, PS, C), dtype)
    ok = np.zeros(PS, bool)
    for s in range(PS):
        n = int((pat[:, s] != 0).sum())
        loss[s], grad[:n, s], ok[s] = ctc_sequence(y[:n, s], labels[s], dtype)
    return loss, grad, ok


def softmax_jacobian(y, dldy):
    """dL/dz for z the logits of y = softmax(z): y * (dL/dy - sum_j y_j dL/dy_j), row by row."""
    y = np.asarray(y, np.float64)
    d = np.asarray(dldy, np.float64)
    return y * (d - (y * d).sum(axis=-1, keepdims=True))
