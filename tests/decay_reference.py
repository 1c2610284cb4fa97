"""Decoupled weight decay as include/currennt_hip.h states it (section Weight decay), restated in numpy.

ld = (float)((double) lr * (double) decay), then w0 = w - ld * w -- one multiplication and one subtraction, each rounded to
nearest -- on the entries that decay, and the family's step from w0.  With dtype float32 every numpy operation below is one
IEEE operation, so the library's weights and optimizer state must EQUAL what this module computes, bit for bit.  With dtype
float64 the same code is compared against torch.optim.AdamW and torch.optim.SGD (tests/test_decay_reference.py)."""
import numpy as np

import adam_reference as AR
import clip_reference as CR


def decayed_ranges(kind, L, P):
    """The runs [start, stop) of a layer's flat weight vector that decay: kind as in the network file, L units, P inputs.
    lstm / blstm: the input weights [0, 4LP) and the recurrent weights behind the 4L bias weights; the bias weights and the
    trailing 3L peephole weights do not.  feedforward_* / softmax: the input weights [0, LP), not the L bias weights."""
    if kind in ("lstm", "blstm"):
        H = L // (2 if kind == "blstm" else 1)
        return [(0, 4 * L * P), (4 * L * (P + 1), 4 * L * (P + 1) + 4 * L * H)]
    if kind.startswith("feedforward_") or kind == "softmax":
        return [(0, L * P)]
    raise ValueError(kind)


def weight_count(kind, L, P):
    if kind in ("lstm", "blstm"):
        return L * (4 * (P + 1) + (2 if kind == "blstm" else 4) * L + 3)
    return L * (P + 1)


def decay_mask(n, ranges, offset=0):
    """bool[n]: True where an entry decays; `ranges` are relative to `offset`.  Entries outside every range (bias, peephole and
    pad entries) are False."""
    m = np.zeros(n, bool)
    for a, b in ranges:
        m[offset + a:offset + b] = True
    return m


def decay_ld(lr, decay, dtype=np.float32):
    """formed in double from the two numbers as `dtype` holds them, rounded once"""
    return dtype(float(dtype(lr)) * float(dtype(decay)))


def decay_weights(w, mask, lr, decay, dtype=np.float32):
    """w0: w - ld * w where mask is set, w itself (no operation) elsewhere.  lr: a scalar or one rate per entry."""
    w = np.asarray(w, dtype)
    lr = np.broadcast_to(np.asarray(lr, dtype), w.shape)
    ld = (lr.astype(np.float64) * float(dtype(decay))).astype(dtype)
    w0 = w.copy()
    w0[mask] = w[mask] - ld[mask] * w[mask]
    assert w0.dtype == dtype
    return w0


def sgd_step(w, g, d, lr, momentum, dtype=np.float32):
    """clip_reference.sgd_step in `dtype`"""
    w, g, d = (np.asarray(a, dtype) for a in (w, g, d))
    d = dtype(momentum) * d - np.asarray(lr, dtype) * g
    w = w + d
    assert w.dtype == dtype and d.dtype == dtype
    return w, d


def decay_sgd_step(w, g, d, lr, momentum, decay, mask, dtype=np.float32):
    """One momentum step with decay; returns (w, d).  lr: a scalar or one rate per entry."""
    if float(decay) == 0.0:
        return sgd_step(w, g, d, lr, momentum, dtype)
    return sgd_step(decay_weights(w, mask, lr, decay, dtype), g, d, lr, momentum, dtype)


def decay_adam_step(w, g, m, v, segments, decay, mask, beta1=0.9, beta2=0.999, eps=1e-8, step=1, dtype=np.float32):
    """One Adam step with decay over an arena; segments: (start, stop, lr) per layer.  ld uses lr, not alpha_t.
    Returns (w, m, v); entries outside every segment (pad entries) are untouched."""
    w, m, v = (np.array(a, dtype) for a in (w, m, v))
    g = np.asarray(g, dtype)
    for a, b, lr in segments:
        w0 = w[a:b] if float(decay) == 0.0 else decay_weights(w[a:b], mask[a:b], lr, decay, dtype)
        w[a:b], m[a:b], v[a:b] = AR.adam_step(w0, g[a:b], m[a:b], v[a:b], lr, beta1, beta2, eps, step, dtype)
    return w, m, v


def clip_decay_sgd_step(w, g, d, lr, momentum, decay, mask, max_norm):
    """The clipped form (float32): the factor scales g only, a skipped step decays nothing.
    Returns (w, d, norm, scale, skip)."""
    gc, norm, scale, skip = CR.clipped(g, max_norm)
    if skip:
        return np.asarray(w, np.float32), np.asarray(d, np.float32), norm, scale, skip
    w, d = decay_sgd_step(w, gc, d, lr, momentum, decay, mask)
    return w, d, norm, scale, skip


def clip_decay_adam_step(w, g, m, v, segments, decay, mask, max_norm, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """Returns (w, m, v, norm, scale, skip)."""
    gc, norm, scale, skip = CR.clipped(g, max_norm)
    if skip:
        return tuple(np.array(a, np.float32) for a in (w, m, v)) + (norm, scale, skip)
    w, m, v = decay_adam_step(w, gc, m, v, segments, decay, mask, beta1, beta2, eps, step)
    return w, m, v, norm, scale, skip
