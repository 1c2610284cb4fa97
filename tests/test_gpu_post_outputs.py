"""-m gpu: the regression and post-output kernels against tests/post_reference.py (float64), at real widths.

Kernels held: post_rows_kernel / post_backward_kernel (sse, weightedsse, wf, ce, rmse, binary_classification), mcc_rows_kernel,
mcc_backward_kernel, softmax_bwd_kernel, ff_delta_kernel, colsum_kernel (+ its fold / its atomics), rowstat_reduce_kernel, and
the target branch of fraction_load_kernel.  Network: 5 inputs -> blstm 12 -> output layer of size L -> post layer, one fraction
of PS = 6 (8 slots on the device) with five sequences: SHORT [11, 7, 9, 4, 1] (88 device rows) or LONG [600, 599, 431, 200, 7]
(4800 device rows; with L = 200, Lp = 224: 4800 x 224 = 1 075 200 elements > the 4096 x 256 of ff_delta_kernel's and
mcc_backward_kernel's grids, 4800 > the 4096 rows of mcc_rows_kernel's grid and of one pass of rowstat_reduce).

Everything is computed from the GPU's own y = net.outputs(): the error and the class count after the forward pass, the injected
errors after the post layer's backward pass alone, the deltas (softmax: the Jacobian) and the bias gradient after the output
layer's backward pass, each inside the bound post_reference derives from the operation count (u = 2^-24; nothing is tuned on
the kernels).  The activations and products are not the subject: outputs and weight gradients stay held to the fp32 oracle at
the suite's tolerances of the mode (1e-4 / 2e-4; bf16: 3e-2 / 6e-2).  multiclass_classification behind feedforward_tanh is held
forward only: -1 / FLT_MIN behind tanh overflows fp32 in the reference too (tests/test_post_reference.py).

The derived sum bound cannot prove that none of 10^5 terms was skipped, so test_every_row_and_column_counts_once makes every
term exactly 0 but spikes at columns {0, 63, 64, L - 1} of chosen rows and asks for their sum to 16 u.  The rows: the first
real row, the last real row, the last real row at each of the four wave positions of a workgroup (row % 4), and in the long
fraction the first real row >= 4096.  (The last workgroup of four device rows of these fractions holds no real frame -- slots
4 .. 7 have ended, are unused or are pad slots at t = T - 1 --, so "a row in the last block" is the last block with a real row.)

MEASURED on one MI355X, largest distance / bound over all cases of the kind (f32, bf16x3, bf16, deterministic 0; short and long):

  kind                       error    injected  deltas    bias gradient
  sse                        0.034    1.00      0 (exact) 0.098
  weightedsse                0.023    0.98      0 (exact) 0.13
  wf                         0.025    0.94      0.74     0.12
  ce                         0.025    0.25      0.36     0.11
  rmse                       0.044    0.23      0 (exact) 0.12
  binary_classification      0.026    0.30      0.76     0.016
  multiclass (logistic)      0.056    0.18      0.73     0.063
  multiclass (tanh)          0.048    (forward only)
  coverage: largest |error - spike sum| / |spike sum| = 1.3 u (bound 16 u)

(sse / weightedsse / wf inject one or two roundings of a difference: half an ulp reaches u * |result| just above a power of two, so
1.00 is the bound met, not missed; an identity output layer hands the errors on untouched.)

The module takes 3.3 s on the GPU machine (83 tests); the slowest test, the first, 1.7 s with the library's start, every other at most 0.15 s."""
import numpy as np
import pytest

import post_reference as pr
from helpers import random_weights
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu

TOL = {"f32": (1e-4, 2e-4), "bf16x3": (1e-4, 2e-4), "bf16": (3e-2, 6e-2)}          # outputs, weight gradients: test_config*
TANH_MCC = ("multiclass_classification", "feedforward_tanh")


def precision_of(pkg, mode):
    return {"f32": pkg.PREC_F32, "bf16x3": pkg.PREC_BF16X3, "bf16": pkg.PREC_BF16}[mode]


def widths_of(post):
    return (1,) if post == "binary_classification" else (33, 64, 65, 200)


# (post, output layer, L, fraction, mode, deterministic): every width on the short fraction and the widest on the long one in
# f32; the widest on the short one also in bf16x3, bf16 and f32 with the atomic sums
CASES = []
for _post, _out in pr.PAIRS:
    for _L in widths_of(_post):
        CASES.append((_post, _out, _L, "short", "f32", None))
    _W = widths_of(_post)[-1]
    CASES.append((_post, _out, _W, "long", "f32", None))
    CASES += [(_post, _out, _W, "short", "bf16x3", None), (_post, _out, _W, "short", "bf16", None), (_post, _out, _W, "short", "f32", 0)]


def case_id(c):
    return "%s-%s-%d-%s-%s%s" % (c[0], c[1].replace("feedforward_", ""), c[2], c[3], c[4], "" if c[5] is None else "-det%d" % c[5])


def inside(tag, got, want, bound):
    """got within `bound` of `want`, element by element; prints and returns the largest distance / bound."""
    dist = np.abs(np.asarray(got, np.float64) - want)
    ratio = float((dist / np.where(bound > 0, bound, 1.0)).max())
    print("[post-outputs] %s %.3g" % (tag, ratio))
    assert np.all(dist <= bound), (tag, ratio, float(dist.max()))             # (a bound of 0 asks for the exact value)
    return ratio


def oracle_pass(orc, layers, weights, frac, backward=True):
    ref = orc.OracleNetwork(layers, weights, pr.PS, frac["T"])
    ref.load_sequences(frac); ref.compute_forward_pass()
    e = ref.calculate_error()
    if backward:
        with np.errstate(all="ignore"):
            ref.compute_backward_pass()
    return ref, e


def check_forward(net, tag, post, L, frac, rows):
    """Step 1: error and class count from the GPU's own outputs.  -> y [T * PS][L]"""
    tg, pat = pr.targets_of(post, frac), frac["patTypes"]
    y = net.outputs().reshape(-1, L)
    assert np.all(np.isfinite(y))
    e, c = net.error_and_correct()
    want, bound = pr.error(post, y, tg, pat, depth=pr.loss_depth(L, rows))
    assert pr.loss_depth(L, rows) <= 64 and bound < 1e-5 * abs(want), (pr.loss_depth(L, rows), bound, want)
    inside(tag + " error", e, want, bound)
    assert c == pr.correct(post, y, tg, pat), (c, pr.correct(post, y, tg, pat))
    return y


def check_injected(net, tag, post, L, frac, y):
    """Step 2: the post layer's backward pass alone.  -> the injected errors as read"""
    tg, pat = pr.targets_of(post, frac), frac["patTypes"]
    net.post_output_layer().backward()
    inj = net.output_layer().output_errors().reshape(-1, L)
    want, bound = pr.inject(post, y, tg, pat)
    inside(tag + " injected", inj, want, bound)
    assert np.all(inj[np.asarray(pat) == 0] == 0)                # every row of a dummy frame and of the unused slot: exactly 0
    return inj


def check_output_backward(net, tag, out_type, L, frac, y, inj, rows):
    """Step 3: deltas (softmax: the Jacobian) of the values read in step 2, and the bias gradient of the deltas read here."""
    out = net.output_layer()
    out.backward()
    dl = out.output_errors().reshape(-1, L)
    if out_type == "softmax":
        want, bound = pr.softmax_jacobian(y, inj, frac["patTypes"])
    else:
        want, bound = pr.delta(pr.ACT_OF[out_type], y, inj)
    inside(tag + " deltas", dl, want, bound)
    gb = out.weight_updates()[L * pr.HIDDEN:L * pr.HIDDEN + L]
    want, bound = pr.bias_gradient(dl, out.bias, device_rows=rows)
    inside(tag + " bias", gb, want, bound)
    return dl


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_post_output_path_against_fp64(pkg, orc, case):
    post, out_type, L, which, mode, det = case
    lengths = pr.SHORT if which == "short" else pr.LONG
    layers, weights, frac = pr.random_case(pkg.make_fraction, random_weights, post, out_type, L, lengths)
    real = np.asarray(frac["patTypes"]) != 0
    held_backward = (post, out_type) != TANH_MCC
    ref, e_ref = oracle_pass(orc, layers, weights, frac)
    tag = "%s/%s %s" % (post, out_type, case_id(case))
    tol, gtol = TOL[mode]
    with pkg.NeuralNetwork(layers, weights, pr.PS, frac["T"], precision=precision_of(pkg, mode),
                           deterministic=None if det is None else bool(det)) as net:
        net.load_sequences(frac); net.compute_forward_pass()
        rows = net.row_map_counts()[2]
        assert rows == frac["T"] * 8 and (mode == "bf16" or net.get_option("deterministic") == (0 if det == 0 else 1))
        y = check_forward(net, tag, post, L, frac, rows)
        assert np.abs(y - ref.outputs().reshape(-1, L))[real].max() < tol
        # the input conditions of tests/test_post_reference.py, at this case's own outputs
        t = np.abs(pr.term(post, y, pr.targets_of(post, frac), frac["patTypes"])[0])
        t = t[real].max(1) if post == "multiclass_classification" else t[real].reshape(-1)
        assert t.max() / t.mean() < 50
        if post == "ce":
            assert y[real].min() > 1e-6
        if not held_backward:
            if which == "long":                     # nothing to hold a backward pass to: the reference's own gradient overflows
                assert not all(np.all(np.isfinite(l.weightUpdates)) for l in ref.trainable_layers())
            return
        inj = check_injected(net, tag, post, L, frac, y)
        dl = check_output_backward(net, tag, out_type, L, frac, y, inj, rows)
        for lay in reversed(net.layers[:-2]):
            lay.backward()
        for lay in net.trainable_layers():
            assert rel_err(lay.weight_updates(), ref.layer(lay.name).weightUpdates) < gtol, lay.name
        # the whole backward pass in one go (multiclass: mcc_backward_kernel launched by the output layer's pass, not by a read)
        net.compute_backward_pass()
        assert np.array_equal(net.output_layer().output_errors().reshape(-1, L), dl)


# ---- 4. coverage of the column and row loops -------------------------------------------------------------------------------

def spike_rows(frac, psp):
    """(t, slot) of the rows that get spikes, and their device rows."""
    pat = np.asarray(frac["patTypes"]).reshape(frac["T"], pr.PS)
    ts, slots = np.nonzero(pat)
    dev = ts * psp + slots
    chosen = {int(dev.min()), int(dev.max())}
    for wave in range(4):
        chosen.add(int(dev[dev % 4 == wave].max()))
    if dev.max() >= 4096:
        chosen.add(int(dev[dev >= 4096].min()))
    return sorted(chosen), [(d // psp, d % psp) for d in sorted(chosen)]


@pytest.mark.parametrize("which", ["short", "long"])
@pytest.mark.parametrize("post,out_type", [p for p in pr.PAIRS if p[0] in ("sse", "weightedsse", "wf", "ce", "rmse")])
def test_every_row_and_column_counts_once(pkg, post, out_type, which):
    L, psp = 200, 8
    lengths = pr.SHORT if which == "short" else pr.LONG
    layers, weights, frac = pr.random_case(pkg.make_fraction, random_weights, post, out_type, L, lengths)
    T = frac["T"]
    dev, where = spike_rows(frac, psp)
    assert dev[0] == 0 and dev[-1] == (T - 1) * psp and (which == "short" or 4096 in dev) and len({d % 4 for d in dev}) == 4
    cols = [0, 63, 64, L - 1]
    spikes = np.zeros((T, pr.PS, L), bool)
    for t, s in where:
        spikes[t, s, cols] = True
    spikes = spikes.reshape(-1, L)
    with pkg.NeuralNetwork(layers, weights, pr.PS, T, precision=pkg.PREC_F32) as net:
        net.load_sequences(frac); net.compute_forward_pass()
        assert net.row_map_counts()[2] == T * psp
        y = net.outputs().reshape(-1, L)
        tg = np.zeros_like(frac["targets"])         # weightedsse: weight 0; wf: mask 0 and target 0; ce: target 0
        if post in ("weightedsse", "wf"):
            tg[:, 0::2][spikes] = 0.375
            tg[:, 1::2][spikes] = 1.25
        elif post == "ce":
            tg[spikes] = 0.25
        else:                                       # sse / rmse: targets equal to y bit for bit, but at the spikes
            tg = y.copy()
            tg[spikes] = y[spikes] + np.float32(0.75)
        frac2 = dict(frac, targets=tg)
        net.load_sequences(frac2); net.compute_forward_pass()
        assert np.array_equal(net.outputs().reshape(-1, L), y)
        e, _ = net.error_and_correct()
        t, _ = pr.term(post, y, tg, frac["patTypes"])
        if post == "rmse":
            assert np.count_nonzero(t) == len(dev)
        else:
            assert np.array_equal(t != 0, spikes)
        want = pr.SCALE[post] * t.sum()
        print("[post-outputs] coverage %s %s: |error - spike sum| / |spike sum| = %.3g u" % (post, which, abs(e - want) / abs(want) / pr.U))
        assert abs(e - want) <= 16 * pr.U * abs(want), (e, want)
        net.post_output_layer().backward()
        inj = net.output_layer().output_errors().reshape(-1, L)
        v, b = pr.inject(post, y, tg, frac["patTypes"])
        assert np.all(inj[~spikes] == 0) and np.all(v[~spikes] == 0)
        assert np.all(np.abs(inj - v) <= b) and np.all(inj[spikes] != 0)


# ---- 5. edges, driven through the weights -------------------------------------------------------------------------------------

PROBE = [5, 3]                                      # 8 real frames


def edge_case(pkg, post, out_type, L, bias_weights, targets):
    """The output layer's input weights 0: every frame's output is act(bias weight_j)."""
    rng = np.random.RandomState(77)
    layers = pr.layers_of(post, out_type, L)
    weights = random_weights(layers, rng, 0.5)
    weights["output"]["input"] = np.zeros(L * pr.HIDDEN, np.float32)
    weights["output"]["bias"] = np.asarray(bias_weights, np.float32)
    xs = [rng.randn(n, pr.P_IN).astype(np.float32) for n in PROBE]
    frac = pkg.make_fraction(xs, targets, pr.PS, classification=pr.target_width(post, L) == 0)
    return layers, weights, frac


def run_edge(pkg, orc, tag, post, out_type, L, bias_weights, targets, y_row=None):
    """Error, class count and injected errors of an edge case: the GPU against post_reference from its own y, and the CPU oracle
    against post_reference from the oracle's y.  -> (error, correct, y, injected) of the GPU"""
    layers, weights, frac = edge_case(pkg, post, out_type, L, bias_weights, targets)
    tg, pat = pr.targets_of(post, frac), frac["patTypes"]
    real = np.asarray(pat) != 0
    assert real.sum() == 8
    ref, e_ref = oracle_pass(orc, layers, weights, frac, backward=False)
    yr = ref.outputs().reshape(-1, L).astype(np.float64)
    N = yr.shape[0]
    want_ref, bound = pr.error(post, yr, tg, pat, depth=L * N)       # (a serial sum over all N x L terms, all alike here)
    assert abs(e_ref - want_ref) <= bound, (e_ref, want_ref, bound)
    if pr.target_width(post, L) == 0:
        assert ref.count_correct_classifications() == pr.correct(post, yr, tg, pat)
    with pkg.NeuralNetwork(layers, weights, pr.PS, frac["T"], precision=pkg.PREC_F32) as net:
        net.load_sequences(frac); net.compute_forward_pass()
        y = net.outputs().reshape(-1, L)
        if y_row is not None:                       # the outputs are what the case is about: exactly these, on every real frame
            assert np.array_equal(y[real], np.broadcast_to(np.asarray(y_row, np.float32), (8, L))), y[real][0]
        e, c = net.error_and_correct()
        want, bound = pr.error(post, y, tg, pat, depth=pr.loss_depth(L, frac["T"] * 8))
        inside(tag + " edge error", e, want, bound)
        assert abs(want - want_ref) <= 1e-5 * abs(want_ref)          # (the same outputs on both sides, to the activations' rounding)
        assert c == pr.correct(post, y, tg, pat)
        if (post, out_type) == TANH_MCC:
            return e, c, y, None
        inj = check_injected(net, tag + " edge", post, L, frac, y)
    return e, c, y, inj


def classes(value):
    return [np.full(n, value, np.int32) for n in PROBE]


@pytest.mark.parametrize("target,correct", [(0, 8), (64, 0)])
def test_edge_all_outputs_equal_and_positive(pkg, orc, target, correct):
    e, c, y, inj = run_edge(pkg, orc, "mcc equal", "multiclass_classification", "feedforward_logistic", 100, np.zeros(100), classes(target),
                            y_row=np.full(100, 0.5))
    assert c == correct and abs(e - 8 * np.log(2.0)) < 1e-5


@pytest.mark.parametrize("target,correct", [(0, 8), (70, 0)])
def test_edge_all_outputs_negative_is_class_0(pkg, orc, target, correct):
    """tanh outputs all -0.5, but -0.25 at column 70: the largest output is not strictly greater than the start (0, class 0), so the
    estimate is class 0, not 70 (what an argmax over the outputs alone would say)."""
    bw = np.full(100, -0.5493061443340549); bw[70] = -0.25541281188299536
    e, c, y, _ = run_edge(pkg, orc, "mcc negative", "multiclass_classification", "feedforward_tanh", 100, bw, classes(target))
    assert np.all(np.abs(np.delete(y, 70, axis=1) + 0.5) < 1e-6) and np.all(np.abs(y[:, 70] + 0.25) < 1e-6)
    assert c == correct and abs(e - 8 * -np.log(pr.FLT_MIN)) < 1e-5 * 698.69      # log max(FLT_MIN, y < 0)


@pytest.mark.parametrize("target,correct", [(0, 8), (3, 0)])
def test_edge_all_outputs_exactly_zero_is_class_0(pkg, orc, target, correct):
    """tanh(0) = 0 everywhere: nothing is strictly greater than the start (a `>=` would walk to the last column)."""
    e, c, y, _ = run_edge(pkg, orc, "mcc zero", "multiclass_classification", "feedforward_tanh", 100, np.zeros(100), classes(target), y_row=np.zeros(100))
    assert c == correct and abs(e - 8 * -np.log(pr.FLT_MIN)) < 1e-5 * 698.69


def test_edge_target_output_underflowed_to_zero(pkg, orc):
    bw = np.zeros(100); bw[64] = -120.0
    row = np.full(100, 0.5); row[64] = 0.0
    e, c, y, inj = run_edge(pkg, orc, "mcc underflow", "multiclass_classification", "feedforward_logistic", 100, bw, classes(64), y_row=row)
    assert c == 0 and abs(e - 698.69) < 0.01        # 8 * -log FLT_MIN
    assert np.count_nonzero(inj) == 8 and np.all(inj[inj[:, 64] != 0, 64] == np.float32(-1.0 / pr.FLT_MIN))


@pytest.mark.parametrize("logit", [60.0, 120.0])
def test_edge_ce_clips_the_injected_error(pkg, orc, logit):
    """One logit at +60: the others' y = 8.8e-27, -t / y far beyond -100; at +120 they are 0 and max(FLT_MIN, 0) keeps it finite."""
    bw = np.zeros(100); bw[7] = logit
    ts = [np.full((n, 100), 0.01, np.float32) for n in PROBE]
    e, c, y, inj = run_edge(pkg, orc, "ce clip", "ce", "softmax", 100, bw, ts)
    real = inj[:, 7] != 0
    others = np.delete(y[real], 7, axis=1)
    assert real.sum() == 8 and np.all(np.abs(y[real][:, 7] - 1.0) < 1e-6)
    assert np.all(others == 0) if logit == 120.0 else (np.all(others > 0) and np.all(others < 1e-26))
    assert np.all(np.delete(inj[real], 7, axis=1) == -100.0) and np.all(np.abs(inj[real][:, 7] + 0.01) < 1e-7)
    assert np.isfinite(e)


def test_edge_binary_at_one_half(pkg, orc):
    ts = [np.array([0, 1, 0, 1, 1], np.int32), np.array([1, 0, 0], np.int32)]
    e, c, y, inj = run_edge(pkg, orc, "binary half", "binary_classification", "feedforward_logistic", 1, [0.0], ts, y_row=[0.5])
    assert c == 4 and abs(e - 8 * np.log(2.0)) < 1e-5               # correct iff the target is 0; log 2 either way


def test_edge_binary_output_underflowed_with_target_1(pkg, orc):
    ts = [np.array([1, 1, 0, 1, 1], np.int32), np.array([1, 0, 1], np.int32)]
    e, c, y, inj = run_edge(pkg, orc, "binary underflow", "binary_classification", "feedforward_logistic", 1, [-120.0], ts, y_row=[0.0])
    assert c == 2 and abs(e - 6 * -np.log(pr.FLT_MIN)) < 1e-5 * 524.02
    assert sorted(set(inj[inj != 0].tolist())) == [float(np.float32(-1.0 / pr.FLT_MIN)), 1.0]


# ---- 6. load routes ---------------------------------------------------------------------------------------------------------

def test_wide_interleaved_targets_load_alike_on_every_route(pkg):
    """weightedsse at L = 200: W = 400 target columns against 32 padded input columns (fraction_load_kernel's grid is sized by
    the inputs), through the staged route, option "overlap" 0 (strided copies) and load_sequences_resident: outputs, error and
    the injected errors bit-equal (the scheme of test_resident_fraction_load_matches_host_load)."""
    import torch
    L = 200
    layers, weights, frac = pr.random_case(pkg.make_fraction, random_weights, "weightedsse", "feedforward_identity", L, pr.SHORT)
    res = {}
    for mode in ("host", "host_strided", "resident"):
        with pkg.NeuralNetwork(layers, weights, pr.PS, frac["T"], precision=pkg.PREC_F32) as net:
            if mode == "host_strided":
                net.set_option("overlap", 0)
            if mode != "resident":
                net.load_sequences(frac)
            else:
                keep = {k: torch.from_numpy(np.ascontiguousarray(frac[k])).cuda() for k in ("inputs", "patTypes", "targets")}
                d = {"T": frac["T"], "Tmin": frac["Tmin"], "numSeqs": frac["numSeqs"], "inputPatternSize": pr.P_IN, "outputPatternSize": 2 * L}
                d.update({k: v.data_ptr() for k, v in keep.items()})
                net.load_sequences_resident(d)
            net.compute_forward_pass()
            e, _ = net.error_and_correct()
            y = net.outputs().reshape(-1, L)
            net.post_output_layer().backward()
            res[mode] = (y, e, net.output_layer().output_errors().reshape(-1, L))
    y, e, inj = res["host"]
    v, b = pr.inject("weightedsse", y, frac["targets"], frac["patTypes"])
    assert np.all(np.abs(inj - v) <= b) and np.count_nonzero(inj) > 0.9 * sum(pr.SHORT) * L
    for mode in ("host_strided", "resident"):
        assert np.array_equal(res[mode][0], y) and res[mode][1] == e and np.array_equal(res[mode][2], inj), mode
