"""LAMB as include/currennt_hip.h states it (section LAMB), restated in numpy, operation by operation.

Every float32 numpy operation below is one IEEE operation rounded to nearest; the two sums per layer are clip_reference.clip_sum
(float64, the header's order) applied to the layer's padded range, the norms one double square root rounded once to float32.  So
the library's w, m, v, ratio and norms must EQUAL what this module computes, bit for bit."""
import math

import numpy as np

import clip_reference as CR
import decay_reference as DR


def lamb_scalars(beta1, beta2, eps, step):
    """omb1, omb2, c_t, eps_t: formed in double from the arguments as float32 holds them, rounded once to float32.  lr is no part
    of c_t: the trust ratio multiplies it."""
    b1, b2, eps = (float(np.float32(x)) for x in (beta1, beta2, eps))
    c2 = math.sqrt(1.0 - math.pow(b2, float(step)))
    c1 = 1.0 - math.pow(b1, float(step))
    return {"b1": np.float32(b1), "b2": np.float32(b2), "omb1": np.float32(1.0 - b1), "omb2": np.float32(1.0 - b2),
            "c_t": np.float32(c2 / c1), "eps_t": np.float32(eps * c2)}


def padded(n):
    """a layer's padded count: its weight count rounded up to a multiple of four"""
    return (n + 3) // 4 * 4


def lamb_direction(w, g, m, v, mask, decay, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """Pass 1 over one layer's padded range; mask: the entries that decay.  Returns (m, v, u)."""
    s = lamb_scalars(beta1, beta2, eps, step)
    w, g, m, v = (np.asarray(a, np.float32) for a in (w, g, m, v))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = s["b1"] * m + s["omb1"] * g
        v = s["b2"] * v + s["omb2"] * (g * g)
        r = (s["c_t"] * m) / (np.sqrt(v) + s["eps_t"])
        u = r.copy()
        if float(decay) != 0.0:
            u[mask] = r[mask] + np.float32(decay) * w[mask]
    assert m.dtype == np.float32 and v.dtype == np.float32 and u.dtype == np.float32
    return m, v, u


def trust_ratio(w, u, min_ratio=0.0, max_ratio=0.0):
    """(ratio, nw, nu), all float32, from the layer's weights before the step and its direction."""
    sw, su = CR.clip_sum(w), CR.clip_sum(u)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        nw, nu = np.float32(np.sqrt(sw)), np.float32(np.sqrt(su))
        if nw == 0 or nu == 0 or not np.isfinite(sw) or not np.isfinite(su):
            return np.float32(1.0), nw, nu
        ratio = np.float32(nw / nu)
    assert ratio.dtype == np.float32
    lo, hi = np.float32(min_ratio), np.float32(max_ratio)
    if ratio < lo:
        ratio = lo
    if hi != 0 and ratio > hi:
        ratio = hi
    return ratio, nw, nu


def lamb_layer_step(w, g, m, v, mask, lr, decay=0.0, bounds=(0.0, 0.0), beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """One layer's step over its padded range.  Returns (w, m, v, (ratio, nw, nu))."""
    w = np.asarray(w, np.float32)
    m, v, u = lamb_direction(w, g, m, v, mask, decay, beta1, beta2, eps, step)
    rec = trust_ratio(w, u, *bounds)
    with np.errstate(over="ignore", invalid="ignore"):
        st = np.float32(lr) * rec[0]
        wn = w - st * u
    assert wn.dtype == np.float32
    return wn, m, v, rec


def lamb_step(w, g, m, v, segments, mask, decay=0.0, bounds=(0.0, 0.0), max_norm=0.0, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """One step over an arena.  segments: (start, stop, lr) per layer, stop - start the layer's PADDED count; mask: bool per arena
    entry (decay_reference.decay_mask).  max_norm != 0: the clipping record in front (the norm over the whole arena's gradient).
    Returns (w, m, v, records): records is one (ratio, nw, nu) per segment, or None on a skipped step -- which changes nothing."""
    w, m, v = (np.array(a, np.float32) for a in (w, m, v))
    g = np.asarray(g, np.float32)
    if float(max_norm) != 0.0:
        g, _, _, skip = CR.clipped(g, max_norm)
        if skip:
            return w, m, v, None
    recs = []
    for a, b, lr in segments:
        w[a:b], m[a:b], v[a:b], rec = lamb_layer_step(w[a:b], g[a:b], m[a:b], v[a:b], mask[a:b], lr, decay, bounds, beta1, beta2, eps, step)
        recs.append(rec)
    return w, m, v, recs


def arena_layout(layers):
    """layers: (kind, L, P) per trainable layer in creation order.  Returns (segments without rates [(start, stop, count)], mask,
    total): each layer's range starts on a multiple of four and is padded to one."""
    segs, ranges, off = [], [], 0
    for kind, L, P in layers:
        n = DR.weight_count(kind, L, P)
        segs.append((off, off + padded(n), n))
        ranges.append((off, DR.decayed_ranges(kind, L, P)))
        off += padded(n)
    mask = np.zeros(off, bool)
    for o, rg in ranges:
        mask |= DR.decay_mask(off, rg, o)
    return segs, mask, off
