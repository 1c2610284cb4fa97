"""Float64 statement of the post output layers and of the output layer's backward pass, with fp32 error bounds.

Plain numpy, no GPU, no oracle.  Transcribed from the header comments of the kernels (csrc/cn_elementwise.hip: "post output
layers", "feed-forward delta and bias gradient", softmax_bwd_kernel) and from oracle/currennt_oracle.c (orc_post_error,
orc_post_backward, orc_mcc_*, orc_binary_correct, orc_ff_backward, orc_softmax_backward); tests/test_post_reference.py holds it
to the double oracle at 1e-12 and shows that the fp32 oracle's arithmetic lies inside every bound below.

Layout.  `y` [N][L]: the output layer's activations, one row per pattern.  `targets`: [N][L] values (sse, ce, rmse), [N][2L]
interleaved (target, weight) pairs (weightedsse) or (target, filter input) pairs (wf), or [N] classes (binary_classification:
0 / 1; multiclass_classification: 0 .. L-1, -1 on a dummy frame).  `pat` [N]: pattern types, 0 = dummy frame.  A pattern is
real where pat != 0 (multiclass: where its class is not -1, MulticlassClassificationLayer.cu:61-62); every quantity of a row
that is not real is 0.  All inputs are fp32 VALUES held in float64, so the float64 arithmetic below is exact to 1e-16.

    term(kind, ...)    -> (t, b)   summands of the error: t[N][L] (rmse: t[N], one per row), error = SCALE[kind] * sum(t)
    inject(kind, ...)  -> (e, b)   what computeBackwardPass of the post layer writes into the output layer's outputErrors
    correct(kind, ...) -> int      countCorrectClassifications (binary, multiclass)
    delta(act, y, e)   -> (d, b)   act'(y) * e, FeedForwardLayer.cu:74-78
    softmax_jacobian(y, e, pat) -> (d, b)   y * (e - sum_j y_j e_j) on real rows, SoftmaxLayer.cu:171-218

BOUNDS.  b is an absolute bound, element by element, of an fp32 evaluation against the float64 value, with u = 2^-24 (fp32
round to nearest).  The rules, from the number format alone (nothing is tuned on a kernel's output; a kernel change that needs
more changes the rule here, by hand and on purpose):
  * every fp32 rounding adds u * |result|; an exact operation (1.0f * e, a negation, a clamp, * 0.5f) adds nothing;
  * where the compiler may contract a * b + c into one fma both forms are allowed: the bound is that of the unfused form,
    which has one rounding more (a contracted accumulation `a += x * x` only loses the product's rounding);
  * logf, sqrtf and a division get 4 u of their result (v_log_f32 / v_rcp_f32 / v_sqrt_f32 based expansions; libm and IEEE
    division are within 1 u);
  * the rounding of a logarithm's ARGUMENT is an absolute error of the logarithm (a relative bound is meaningless where log
    crosses 0): ce's quotient (a division, 4 u relative) gives t * 4 u on the term t * log(q); binary's 1 - act (one rounding)
    is given the same 4 u;
  * a sum formed by a tree of depth d gets d * u * sum |x_i| on top of the bounds of its summands;
  * products of two first-order terms are covered by the factor SECOND = 1 + 2^-12 on every bound (each bound has fewer than
    2^6 first-order terms of at most 2^6 u = 2^-18 each).
Depth of the error sum (loss_depth): ceil(L/64) + 6 + ceil(N/4096) + 2 + 6 + 16 -- a lane adds its ceil(L/64) columns in a
chain, six xor shuffles fold the wave, then rowstat_reduce adds a virtual thread's ceil(N/4096) rows per slot in a chain, its
four slots in two levels, six shuffles per virtual wave and the sixteen wave sums in a chain.
Depth of the bias sum (bias_depth): ceil(N/(8 * blocks)) + 8 + blocks, blocks = min(512, ceil(N/64)) -- a thread of
colsum_kernel adds its rows in a chain, the workgroup its eight row lanes in a chain, and the workgroups' partial sums are added
in a chain: by fold_kernel in workgroup order (deterministic) or by one atomic per workgroup in arrival order, the same count.
A serial sum (the CPU oracle) has the depth of its length; tests pass `depth` for it.
"""
import numpy as np

U = 2.0 ** -24
FLT_MIN = float(np.float32(1.1754944e-38))          # helpers/NumericLimits.cuh: min(), the literal of the oracle's NL_MIN
SECOND = 1.0 + 2.0 ** -12
FN = 4.0                                            # logf, sqrtf, division: FN * u of the result

SUM_KINDS = ("sse", "weightedsse", "wf", "ce", "rmse", "binary_classification")
KINDS = SUM_KINDS + ("multiclass_classification",)
SCALE = {"sse": 0.5, "weightedsse": 0.5, "wf": 0.5, "ce": 1.0, "rmse": 1.0, "binary_classification": 1.0,
         "multiclass_classification": -1.0}


def target_width(kind, L):
    """Columns of the targets of a post layer behind an output layer of size L (0: classes)."""
    if kind in ("weightedsse", "wf"):
        return 2 * L
    return 0 if kind in ("binary_classification", "multiclass_classification") else L


def _f64(a):
    return np.asarray(a, np.float64)


def real_rows(kind, targets, pat):
    if kind == "multiclass_classification":
        return np.asarray(targets).reshape(-1) != -1
    return np.asarray(pat).reshape(-1) != 0


def _pairs(targets, L):
    tg = _f64(targets).reshape(-1, L, 2)
    return tg[:, :, 0], tg[:, :, 1]


def _diff(kind, y, targets):
    """df of sse / weightedsse / wf / rmse and its bound."""
    L = y.shape[1]
    if kind == "sse":
        df = _f64(targets).reshape(-1, L) - y
        return df, U * np.abs(df), None
    if kind == "rmse":
        df = y - _f64(targets).reshape(-1, L)
        return df, U * np.abs(df), None
    t, w = _pairs(targets, L)
    if kind == "weightedsse":                       # (y - t) * w: two roundings
        df = (y - t) * w
        return df, 2 * U * np.abs(df), w
    df = y * w - t                                  # wf: fl(fl(y f) - t), or one fma
    return df, U * np.abs(y * w) + U * np.abs(df), w


def loss_depth(L, N):
    return -(-L // 64) + 6 + -(-N // 4096) + 2 + 6 + 16


def bias_depth(N):
    blocks = min(512, -(-N // 64))
    return -(-N // (8 * blocks)) + 8 + blocks


def _rmse_rows(y, targets, real, col_depth):
    """Per-row sqrt(sum_j (y - t)^2 / L) and its RELATIVE bound."""
    L = y.shape[1]
    df, bdf, _ = _diff("rmse", y, targets)
    sq = df * df
    bsq = 2 * np.abs(df) * bdf + U * sq
    S = sq.sum(1)
    bS = bsq.sum(1) + col_depth * U * (sq + bsq).sum(1)
    rel_S = np.where(S > 0, bS / np.where(S > 0, S, 1.0), 0.0)
    r = np.where(real, np.sqrt(S / L), 0.0)
    rel = 0.5 * (rel_S + FN * U) + FN * U          # sqrt halves what its argument carries: the sum's bound and the division's
    return r, np.where(real, rel, 0.0)


def term(kind, y, targets, pat, col_depth=None):
    """Summands of the error and their bounds.  rmse: one per row (col_depth: depth of the row's column sum, default the
    kernels' ceil(L/64) + 6); else one per (row, column); multiclass: log max(FLT_MIN, y[target]) in column `target`."""
    y = _f64(y)
    N, L = y.shape
    real = real_rows(kind, targets, pat)
    if kind == "rmse":
        r, rel = _rmse_rows(y, targets, real, -(-L // 64) + 6 if col_depth is None else col_depth)
        return r, SECOND * rel * r
    if kind in ("sse", "weightedsse", "wf"):
        df, bdf, _ = _diff(kind, y, targets)
        t = df * df
        b = 2 * np.abs(df) * bdf + bdf * bdf + U * t
    elif kind == "ce":
        tg = _f64(targets).reshape(N, L)
        t = tg * np.log(np.maximum(FLT_MIN, tg) / np.maximum(FLT_MIN, y))
        b = FN * U * np.abs(tg) + (FN + 1) * U * np.abs(t)
    elif kind == "binary_classification":
        tg = _f64(targets).reshape(N, 1)
        act = np.maximum(y, FLT_MIN)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -np.log(np.where(tg > 0, act, 1.0 - act))
        b = np.where(tg > 0, 0.0, FN * U) + FN * U * np.abs(t)
    else:
        tc = np.asarray(targets).reshape(-1)
        t = np.zeros((N, L))
        rows = np.nonzero(real)[0]
        t[rows, tc[rows]] = np.log(np.maximum(FLT_MIN, y[rows, tc[rows]]))
        b = FN * U * np.abs(t)
    t = np.where(real[:, None], t, 0.0)
    return t, SECOND * np.where(real[:, None], b, 0.0)


def error(kind, y, targets, pat, depth=None, col_depth=None):
    """calculateError in float64 and the bound of an fp32 evaluation whose sum is a tree of `depth` (default loss_depth; rmse:
    `col_depth` of it, default ceil(L/64) + 6, lies inside the row terms and the rest sums the rows)."""
    y = _f64(y)
    N, L = y.shape
    t, b = term(kind, y, targets, pat, col_depth)
    d = loss_depth(L, N) if depth is None else depth
    if kind == "rmse":
        d -= -(-L // 64) + 6 if col_depth is None else col_depth
    s = SCALE[kind]
    return s * t.sum(), abs(s) * SECOND * (b.sum() + d * U * (np.abs(t) + b).sum())


def inject(kind, y, targets, pat, col_depth=None):
    """The errors the post layer injects into the output layer and their bounds."""
    y = _f64(y)
    N, L = y.shape
    real = real_rows(kind, targets, pat)
    if kind in ("sse", "weightedsse", "wf"):
        df, bdf, w = _diff(kind, y, targets)
        if kind == "sse":
            e, b = -df, bdf
        elif kind == "weightedsse":
            e, b = df, bdf
        else:
            e = df * w
            b = bdf * np.abs(w) + U * np.abs(e)
    elif kind == "rmse":
        r, rel = _rmse_rows(y, targets, real, -(-L // 64) + 6 if col_depth is None else col_depth)
        df, bdf, _ = _diff(kind, y, targets)
        e = r[:, None] * df
        b = np.abs(e) * (rel[:, None] + 2 * U)
    elif kind == "ce":
        tg = _f64(targets).reshape(N, L)
        q = -tg / np.maximum(FLT_MIN, y)
        e = np.clip(q, -100.0, 100.0)
        b = np.where(np.abs(q) > 100.0 * (1 + 2 * FN * U), 0.0, FN * U * np.abs(q))      # far beyond the clip: exactly +-100
    elif kind == "binary_classification":
        tg = _f64(targets).reshape(N, 1)
        act = np.maximum(y, FLT_MIN)
        with np.errstate(divide="ignore"):
            e = np.where(tg > 0, -1.0 / act, 1.0 / (1.0 - act))
        b = np.where(tg > 0, FN * U, (FN + 1) * U) * np.abs(e)
    else:
        tc = np.asarray(targets).reshape(-1)
        e = np.zeros((N, L))
        rows = np.nonzero(real)[0]
        e[rows, tc[rows]] = -1.0 / np.maximum(FLT_MIN, y[rows, tc[rows]])
        b = FN * U * np.abs(e)
    return np.where(real[:, None], e, 0.0), SECOND * np.where(real[:, None], b, 0.0)


def estimated_classes(y):
    """CountCorrectClassificationsFn (MulticlassClassificationLayer.cu:89-99): start at (0, class 0), a strictly greater value wins."""
    y = _f64(y)
    first_max = y.argmax(1)                         # numpy: the first of equal maxima = the first strictly greater one
    return np.where(y.max(1) > 0.0, first_max, 0)


def correct(kind, y, targets, pat):
    y = _f64(y)
    real = real_rows(kind, targets, pat)
    tc = np.asarray(targets).reshape(-1)
    if kind == "binary_classification":             # BinaryClassificationLayer.cu:69-85
        return int(np.sum(real & ((tc > 0.5) == (y[:, 0] > 0.5))))
    if kind == "multiclass_classification":
        return int(np.sum(real & (estimated_classes(y) == tc)))
    return -1


def delta(act, y, e):
    """ComputeDeltaFn: act'(y) * e for "tanh" (1 - y^2), "logistic" (y (1 - y)) and "identity" (1)."""
    y, e = _f64(y), _f64(e)
    if act == "identity":
        return e.copy(), np.zeros_like(e)
    if act == "tanh":                               # fl(1 - fl(y y)) or one fma, then * e
        dv = 1.0 - y * y
        bdv = U * y * y + U * np.abs(dv)
    elif act == "logistic":                         # fl(y * fl(1 - y)), then * e
        dv = y * (1.0 - y)
        bdv = 2 * U * np.abs(dv)
    else:
        raise ValueError(act)
    d = dv * e
    return d, SECOND * (bdv * np.abs(e) + U * np.abs(d))


def softmax_jacobian(y, e, pat, depth=None):
    """y_j * (e_j - sum_k y_k e_k) on real rows; the other rows keep e (SoftmaxLayer.cu:175-176 skips them).  depth: of the row's
    sum, default the kernel's ceil(L/64) + 6."""
    y, e = _f64(y), _f64(e)
    L = y.shape[1]
    d = -(-L // 64) + 6 if depth is None else depth
    real = (np.asarray(pat).reshape(-1) != 0)[:, None]
    ye = y * e
    off = ye.sum(1, keepdims=True)
    boff = (d + 1) * U * np.abs(ye).sum(1, keepdims=True)
    inner = e - off
    binner = boff + U * np.abs(inner)
    out = y * inner
    b = np.abs(y) * binner + U * np.abs(out)
    return np.where(real, out, e), SECOND * np.where(real, b, 0.0)


def bias_gradient(deltas, bias, device_rows=None, depth=None):
    """ComputeBiasWeightUpdateFn (FeedForwardLayer.cu:90-101): bias * sum_n deltas[n][j], and the bound of an fp32 sum of depth
    `depth` (default bias_depth(device_rows)) of the given deltas followed by one product."""
    dl = _f64(deltas)
    d = bias_depth(device_rows if device_rows is not None else dl.shape[0]) if depth is None else depth
    s = dl.sum(0)
    return bias * s, SECOND * abs(bias) * (d * U * np.abs(dl).sum(0) + U * np.abs(s))


ACT_OF = {"feedforward_tanh": "tanh", "feedforward_logistic": "logistic", "feedforward_identity": "identity", "softmax": "softmax"}

# (post layer, output layer): the pairs of tests/test_post_reference.py and tests/test_gpu_post_outputs.py
PAIRS = [("sse", "feedforward_identity"), ("weightedsse", "feedforward_identity"), ("wf", "feedforward_tanh"), ("ce", "softmax"),
         ("rmse", "feedforward_identity"), ("binary_classification", "feedforward_logistic"),
         ("multiclass_classification", "feedforward_logistic"), ("multiclass_classification", "feedforward_tanh")]
SHORT, LONG = [11, 7, 9, 4, 1], [600, 599, 431, 200, 7]
P_IN, HIDDEN, PS = 5, 12, 6


def layers_of(post, out_type, L):
    return [{"name": "input", "type": "input", "size": P_IN},
            {"name": "lstm_0", "type": "blstm", "size": HIDDEN, "bias": 1.0},
            {"name": "output", "type": out_type, "size": L, "bias": 1.0},
            {"name": "postoutput", "type": post, "size": target_width(post, L) or L}]


def random_targets(rng, post, L, lengths):
    """Per-sequence targets of a random case: classes, a distribution with an exact zero per row (ce), or values uniform in [-1, 1)."""
    if post == "binary_classification":
        return [rng.randint(0, 2, n).astype(np.int32) for n in lengths]
    if post == "multiclass_classification":
        return [rng.randint(0, L, n).astype(np.int32) for n in lengths]
    if post == "ce":
        ts = []
        for n in lengths:
            t = rng.rand(n, L).astype(np.float32)
            t[:, 0] = 0
            ts.append((t / t.sum(1, keepdims=True)).astype(np.float32))
        return ts
    ts = [rng.uniform(-1, 1, (n, target_width(post, L))).astype(np.float32) for n in lengths]
    if post in ("weightedsse", "wf"):               # weights / filter inputs in [0.5, 1.5): no heavy tail in the squared terms
        for t in ts:
            t[:, 1::2] += 1.5
    return ts


def random_case(make_fraction, random_weights, post, out_type, L, lengths, seed=31):
    """5 inputs -> blstm 12 -> `out_type` L -> `post` on one fraction of PS = 6 with the five sequences `lengths`."""
    rng = np.random.RandomState(seed + L)
    layers = layers_of(post, out_type, L)
    weights = random_weights(layers, rng, 0.5)
    xs = [rng.randn(n, P_IN).astype(np.float32) for n in lengths]
    ts = random_targets(rng, post, L, lengths)
    frac = make_fraction(xs, ts, PS, classification=target_width(post, L) == 0)
    return layers, weights, frac


def targets_of(post, frac):
    return frac["targetClasses"] if target_width(post, 1) == 0 else frac["targets"]
