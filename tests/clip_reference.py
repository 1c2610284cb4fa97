"""Gradient clipping by the global L2 norm as include/currennt_hip.h states it (section Gradient clipping), restated in numpy.

The sum of squares is formed in float64 in the header's order, the norm is one double square root rounded once to float32, the
factor one float32 division and the scaled gradient one float32 multiplication per entry -- so the library's norm, factor, weights
and optimizer state must EQUAL what this module computes, bit for bit."""
import numpy as np

import adam_reference as AR

L = 16384          # lanes of the sum (CLIP_LANES)


def clip_sum(g):
    """S = sum g[i]^2 in double: lane k adds g[k]^2, g[k + L]^2, ... in ascending order (entries behind the end count as +0),
    then neighbouring lanes are added pairwise, level by level."""
    g = np.asarray(g, np.float32).reshape(-1)
    rows = -(-max(g.size, 1) // L)
    p = np.zeros(rows * L, np.float32)
    p[:g.size] = g
    acc = np.zeros(L, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in p.reshape(rows, L):
            d = r.astype(np.float64)
            acc = acc + d * d                   # (d * d is exact: 48 significant bits)
        while acc.size > 1:
            acc = acc[0::2] + acc[1::2]
    return np.float64(acc[0])


def clip_factor(g, max_norm):
    """(norm, scale, skip): norm float32; scale float32, or None when no multiplication happens; skip: S is not finite."""
    s = clip_sum(g)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.float32(np.sqrt(s))
    if not np.isfinite(s):
        return norm, None, True
    max_norm = np.float32(max_norm)
    if norm > max_norm:
        return norm, np.float32(max_norm / norm), False
    return norm, None, False


def clipped(g, max_norm):
    """(g' or None on a skipped step, norm, scale, skip): the gradient the update rule reads."""
    g = np.asarray(g, np.float32)
    norm, scale, skip = clip_factor(g, max_norm)
    if skip:
        return None, norm, scale, skip
    if scale is not None:
        with np.errstate(over="ignore"):
            g = scale * g
        assert g.dtype == np.float32
    return g, norm, scale, skip


def sgd_step(w, g, d, lr, momentum):
    """UpdateWeightFn in float32: delta = momentum * delta - lr * g; w += delta.  lr: a scalar or one rate per entry."""
    w, g, d = (np.asarray(a, np.float32) for a in (w, g, d))
    lr = np.asarray(lr, np.float32)
    d = np.float32(momentum) * d - lr * g
    w = w + d
    assert w.dtype == np.float32 and d.dtype == np.float32
    return w, d


def clip_sgd_step(w, g, d, lr, momentum, max_norm):
    """One clipped momentum step over the whole arena; returns (w, d, norm, scale, skip)."""
    gc, norm, scale, skip = clipped(g, max_norm)
    if skip:
        return np.asarray(w, np.float32), np.asarray(d, np.float32), norm, scale, skip
    w, d = sgd_step(w, gc, d, lr, momentum)
    return w, d, norm, scale, skip


def clip_adam_step(w, g, m, v, segments, max_norm, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """One clipped Adam step over the whole arena.  segments: (start, stop, lr) per layer -- the rates are per layer, the factor
    is global.  Returns (w, m, v, norm, scale, skip)."""
    w, m, v = (np.array(a, np.float32) for a in (w, m, v))
    gc, norm, scale, skip = clipped(g, max_norm)
    if skip:
        return w, m, v, norm, scale, skip
    for a, b, lr in segments:
        w[a:b], m[a:b], v[a:b] = AR.adam_step(w[a:b], gc[a:b], m[a:b], v[a:b], lr, beta1, beta2, eps, step)
    return w, m, v, norm, scale, skip
