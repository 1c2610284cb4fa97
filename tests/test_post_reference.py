"""tests/post_reference.py (the float64 statement of the post output layers and of the output layer's backward pass that
tests/test_gpu_post_outputs.py holds the kernels to) against the CPU oracle, no GPU:
  * the double oracle (oracle.real64()) and post_reference agree to 1e-12 on the error, the class count and the output layer's
    outputErrors after the whole backward pass;
  * the fp32 oracle's per-element quantities, recomputed from its own fp32 outputs, lie INSIDE post_reference's per-element
    bounds, and its serially summed error inside the sum bound with d = L + N: the bounds admit honest fp32 arithmetic;
  * the input conditions the GPU module relies on hold in the random cases."""
import numpy as np
import pytest

import post_reference as pr
from helpers import random_weights

WIDTHS = (33, 65, 200)
CASES = [(post, out, 1) for post, out in pr.PAIRS if post == "binary_classification"] + \
        [(post, out, L) for post, out in pr.PAIRS if post != "binary_classification" for L in WIDTHS]
IDS = ["%s-%s-%d" % (p, o.replace("feedforward_", ""), L) for p, o, L in CASES]


def run_oracle(ons, layers, weights, frac):
    """Forward pass, error, class count, injected errors (the post layer's backward pass alone) and the whole backward pass of one
    oracle namespace, as float64."""
    post = layers[-1]["type"]
    ref = ons.OracleNetwork(layers, weights, pr.PS, frac["T"])
    ref.load_sequences(frac); ref.compute_forward_pass()
    out = ref.layers[-2]
    L, N = out.size, ref.N
    res = {"y": out.outputs[:N * L].reshape(N, L).astype(np.float64), "error": ref.calculate_error(), "correct": -1}
    if post in ("binary_classification", "multiclass_classification"):
        res["correct"] = ref.count_correct_classifications()
    inj = np.zeros(N * L, ons.REAL)
    if post == "multiclass_classification":
        ons.lib().orc_mcc_backward(L, N, ref.targetClasses, out.outputs, inj)
    else:
        ons.lib().orc_post_backward(ons.POST[post], L, N, ref.patTypes, ref.targets, out.outputs, inj)
    res["inject"] = inj.reshape(N, L).astype(np.float64)
    with np.errstate(all="ignore"):
        ref.compute_backward_pass()
    res["deltas"] = out.outputErrors[:N * L].reshape(N, L).astype(np.float64)
    res["grad_finite"] = all(bool(np.all(np.isfinite(l.weightUpdates))) for l in ref.trainable_layers())
    return res


def reference(post, out_type, y, frac, e=None, **depths):
    """post_reference's quantities for the outputs `y`; the deltas from the injected errors `e` (default: its own)."""
    tg, pat = pr.targets_of(post, frac), frac["patTypes"]
    L, N = y.shape[1], y.shape[0]
    r = {"error": pr.error(post, y, tg, pat, **depths), "correct": pr.correct(post, y, tg, pat),
         "term": pr.term(post, y, tg, pat, depths.get("col_depth")), "inject": pr.inject(post, y, tg, pat, depths.get("col_depth"))}
    e = r["inject"][0] if e is None else e
    if out_type == "softmax":
        r["deltas"] = pr.softmax_jacobian(y, e, pat, depths.get("col_depth"))
    else:
        r["deltas"] = pr.delta(pr.ACT_OF[out_type], y, e)
    return r


@pytest.mark.parametrize("post,out_type,L", CASES, ids=IDS)
def test_post_reference_against_the_oracles(pkg, orc, post, out_type, L):
    layers, weights, frac = pr.random_case(pkg.make_fraction, random_weights, post, out_type, L, pr.SHORT)
    N = frac["T"] * pr.PS
    real = pr.real_rows(post, pr.targets_of(post, frac), frac["patTypes"])
    assert real.sum() == sum(pr.SHORT) and N - real.sum() >= frac["T"]          # ragged, one unused slot

    # 1. the double oracle: same rule, same numbers
    o64 = run_oracle(orc.real64(), layers, weights, frac)
    r = reference(post, out_type, o64["y"], frac)
    assert np.all(np.isfinite(r["error"])) and all(np.all(np.isfinite(r[k][0])) and np.all(np.isfinite(r[k][1])) for k in ("term", "inject", "deltas"))
    assert abs(r["error"][0] - o64["error"]) <= 1e-12 * abs(o64["error"]), (r["error"][0], o64["error"])
    assert r["correct"] == o64["correct"]
    for k in ("inject", "deltas"):
        assert np.abs(r[k][0] - o64[k]).max() <= 1e-12 * np.abs(o64[k]).max(), k
    assert np.all(o64["inject"][~real] == 0) and np.all(o64["deltas"][~real] == 0)

    # 2. the fp32 oracle inside the bounds, from its own fp32 outputs (serial sums: depth L for a row, L + N for the error)
    o32 = run_oracle(orc, layers, weights, frac)
    y32 = o32["y"]
    q = reference(post, out_type, y32, frac, e=o32["inject"], depth=L + N, col_depth=L)
    err, berr = q["error"]
    print("\n[%s %s L=%d] error %.9g, fp32 oracle off by %.3g of its bound %.3g (relative %.3g); kernel-depth bound relative %.3g"
          % (post, out_type, L, err, abs(o32["error"] - err) / berr, berr, berr / abs(err),
             pr.error(post, y32, pr.targets_of(post, frac), frac["patTypes"])[1] / abs(err)))
    assert abs(o32["error"] - err) <= berr, (o32["error"], err, berr)
    assert q["correct"] == o32["correct"]
    for k in ("inject", "deltas"):
        v, b = q[k]
        worst = float((np.abs(o32[k] - v) / np.where(b > 0, b, 1.0)).max())
        print("[%s %s L=%d] %s: fp32 oracle at most %.3g of the per-element bound" % (post, out_type, L, k, worst))
        assert np.all(np.abs(o32[k] - v) <= b), (k, worst)
    # behind tanh a negative target output injects -1 / FLT_MIN = -8.5e37: deltas a factor 4 below FLT_MAX, which the sums of
    # the long fraction overflow (test_multiclass_behind_tanh_overflows_the_fp32_reference)
    if (post, out_type) == ("multiclass_classification", "feedforward_tanh"):
        assert np.abs(o32["deltas"]).max() > 1e37
    else:
        assert o32["grad_finite"]

    # 3. the input conditions the GPU module relies on
    t = np.abs(r["term"][0])
    t = t[real].max(1) if post == "multiclass_classification" else t[real].reshape(-1)      # (multiclass: one term per row)
    assert t.max() / t.mean() < 50, (t.max(), t.mean())
    if post == "ce":
        assert y32[real].min() > 1e-6
    # the kernels' depth at this shape and at the long fraction, and the relative bound it gives
    for rows in (88, 4800):
        assert pr.loss_depth(L, rows) <= 64
    assert pr.error(post, y32, pr.targets_of(post, frac), frac["patTypes"])[1] < 1e-5 * abs(err)


def test_multiclass_behind_tanh_overflows_the_fp32_reference(pkg, orc):
    """Why tests/test_gpu_post_outputs.py holds multiclass_classification behind feedforward_tanh forward only: on the long
    fraction the fp32 oracle's own weight gradient is not finite (sums of deltas of 8.5e37), so there is nothing to hold a
    backward pass to; the forward quantities are finite and inside the bounds."""
    layers, weights, frac = pr.random_case(pkg.make_fraction, random_weights, "multiclass_classification", "feedforward_tanh", 200, pr.LONG)
    o32 = run_oracle(orc, layers, weights, frac)
    assert not o32["grad_finite"]
    err, berr = pr.error("multiclass_classification", o32["y"], frac["targetClasses"], frac["patTypes"], depth=200 + frac["T"] * pr.PS)
    assert np.isfinite(o32["error"]) and abs(o32["error"] - err) <= berr
    assert o32["correct"] == pr.correct("multiclass_classification", o32["y"], frac["targetClasses"], frac["patTypes"])


def test_rules_on_hand_made_rows():
    """The clamps and the class rule, on values chosen by hand."""
    pat = np.array([1, 1, 0], np.int8)
    # multiclass: start (0, class 0), strictly greater wins
    y = np.array([[0.25, 0.25, 0.25], [-0.5, -0.25, -0.125], [0.0, 0.0, 0.9]])
    assert list(pr.estimated_classes(y)) == [0, 0, 2]
    assert list(pr.estimated_classes(np.array([[0.0, 0.0, 0.0], [0.1, 0.3, 0.3]]))) == [0, 1]
    tc = np.array([0, 1, -1], np.int32)
    assert pr.correct("multiclass_classification", y, tc, pat) == 1
    t, _ = pr.term("multiclass_classification", y, tc, pat)
    assert t[1, 1] == np.log(pr.FLT_MIN) and t[0, 0] == np.log(0.25) and np.count_nonzero(t) == 2
    e, _ = pr.inject("multiclass_classification", y, tc, pat)
    assert e[1, 1] == -1.0 / pr.FLT_MIN and e[0, 0] == -4.0 and np.count_nonzero(e) == 2
    # ce: clipped at +-100, max(FLT_MIN, 0) keeps it finite, a zero target gives an exact zero
    yc = np.array([[0.0, 1e-26, 0.5, 0.5], [0.25, 0.25, 0.25, 0.25], [0.5, 0.5, 0.0, 0.0]])
    tg = np.array([[0.5, 0.5, 0.0, 0.0], [0.0, 0.0, 0.5, 0.5], [1.0, 0.0, 0.0, 0.0]])
    e, b = pr.inject("ce", yc, tg, pat)
    assert list(e[0]) == [-100.0, -100.0, 0.0, 0.0] and np.all(b[0] == 0) and list(e[1]) == [0.0, 0.0, -2.0, -2.0] and np.all(e[2] == 0)
    t, b = pr.term("ce", yc, tg, pat)
    assert np.all(t[0, 2:] == 0) and np.all(b[0, 2:] == 0) and np.all(np.isfinite(t)) and np.all(t[2] == 0)
    # binary: y == 0.5 is class 0; term log 2 either way
    yb = np.array([[0.5], [0.5], [0.9]])
    assert pr.correct("binary_classification", yb, np.array([0, 1, 1], np.int32), pat) == 1
    t, _ = pr.term("binary_classification", yb, np.array([0, 1, 1], np.int32), pat)
    assert t[0, 0] == np.log(2.0) and t[1, 0] == np.log(2.0) and t[2, 0] == 0
    e, _ = pr.inject("binary_classification", np.array([[0.0], [0.25], [0.3]]), np.array([1, 0, 0], np.int32), pat)
    assert e[0, 0] == -1.0 / pr.FLT_MIN and e[1, 0] == 1.0 / 0.75 and e[2, 0] == 0
    # the depths named in the module's docstring
    assert pr.loss_depth(200, 4800) == 4 + 6 + 2 + 2 + 6 + 16 and pr.loss_depth(33, 88) == 1 + 6 + 1 + 2 + 6 + 16
    assert pr.bias_depth(4800) == 8 + 8 + 75 and pr.bias_depth(88) == 6 + 8 + 2
