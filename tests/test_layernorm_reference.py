"""The restatement the GPU is held to (tests/layernorm_reference.py), checked on the CPU: the fp64 autograd stack with nothing
normed is the double oracle; the handed-back error formula is autograd's; a gain and a bias on the normalised copy are absorbed
by the input and bias weights; the bf16 model of every net the GPU file runs through in bf16 stays within 1e-2 of the fp64 stack
(which is what lets that file keep the 3e-2 pin); and the feature is declared where the headers, the binding and the Makefile
declare such things."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import oracle_reference
from layernorm_reference import (BF16_THROUGH_NET, Case, autograd_stack, layer_norm_backward, layer_norm_rule, rel, stack_results,
                                 torch_layer_norm)
from residual_reference import flat_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unnormed_stack_is_the_double_oracle(pkg, orc):
    """(a) No layer normed: the stack against oracle_reference(orc.real64()), to the 1e-10 that
    test_double_oracle_equals_fp64_autograd_to_rounding_noise allows two fp64 statements of the same equations."""
    case = Case(pkg, "small")
    want = oracle_reference(orc.real64(), case.layers, case.weights, case.frac, case.PS)
    loss, post, grads, errs = stack_results(case.layers, case.weights, case.frac, case.lens)
    worst = {"loss": abs(loss - want["error"]) / max(1.0, abs(loss)), "post": float(np.abs(post - want["post"]).max())}
    for name, g in grads.items():
        worst["grad/" + name] = float(np.abs(g - want["grad/" + name]).max() / np.abs(g).max())
    for name, e in errs.items():
        worst["err/" + name] = float(np.abs(e - want["err/" + name]).max() / np.abs(e).max())
    print({k: float("%.2g" % v) for k, v in worst.items()})
    assert len(errs) == 4 and all(v <= 1e-10 for v in worst.values()), worst


def test_stack_clips_the_deltas_as_the_double_oracle_does(pkg, orc):
    """(a) again with weights large enough for the LSTM cell's delta clip to act (limitedError.cuh): behind a normalisation the
    handed-back errors are 1 / std times larger and reach it, so the stack states the clip, and states it as the oracle does."""
    import copy
    from test_oracle_autograd import lstm_layer as unclipped
    import layernorm_reference as R
    case = Case(pkg, "small")
    weights = copy.deepcopy(case.weights)
    weights["output"]["input"] = np.asarray(weights["output"]["input"]) * 40.0
    want = oracle_reference(orc.real64(), case.layers, weights, case.frac, case.PS)
    loss, post, grads, errs = stack_results(case.layers, weights, case.frac, case.lens)
    worst = {"loss": abs(loss - want["error"]) / max(1.0, abs(loss)), "post": float(np.abs(post - want["post"]).max())}
    for name, g in grads.items():
        worst["grad/" + name] = float(np.abs(g - want["grad/" + name]).max() / np.abs(g).max())
    for name, e in errs.items():
        worst["err/" + name] = float(np.abs(e - want["err/" + name]).max() / np.abs(e).max())
    print({k: float("%.2g" % v) for k, v in worst.items()})
    assert all(v <= 1e-10 for v in worst.values()), worst
    clipped, R.lstm_layer = R.lstm_layer, unclipped          # (the clip does act here: without it the gradients differ)
    try:
        plain = stack_results(case.layers, weights, case.frac, case.lens)
    finally:
        R.lstm_layer = clipped
    assert rel(plain[2]["lstm_0"], grads["lstm_0"]) > 1e-2


def test_handed_back_error_formula_is_autograds():
    """(b) dx = rstd * (g - mean(g) - xn * mean(g * xn)) on a 3 x 6 row block, to 1e-12."""
    rng = np.random.RandomState(11)
    x = (rng.randn(3, 6) * np.array([[1.0], [5.0], [0.01]]) + np.array([[0.0], [3.0], [-2.0]])).astype(np.float32)
    g = rng.randn(3, 6)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    (torch_layer_norm(xt, float(np.float32(1e-5))) * torch.tensor(g)).sum().backward()
    xn, _, rho = layer_norm_rule(x, np.ones(3, bool))
    got = layer_norm_backward(g, xn, rho)
    assert np.abs(got - xt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(got).max()), float(np.abs(got - xt.grad.numpy()).max())
    assert np.abs(got).max() > 1e-2
    # rows that are not real frames normalise to zeros
    assert np.all(layer_norm_rule(x, np.array([True, False, True]))[0][1] == 0)


def test_gain_and_bias_are_absorbed_by_the_weights(pkg):
    """(c) W (gamma * xn + beta) + b = (W diag gamma) xn + (W beta + b): the "first" net (an lstm, a blstm and the softmax layer
    normed) with a random gain and bias on every normalised copy gives the posteriors and the loss of the same net without them
    and with the folded weights, to 1e-12."""
    case = Case(pkg, "first")
    rng = np.random.RandomState(12)
    w = flat_weights(case.weights)
    affine, folded, prev = {}, {}, case.P
    for d in case.layers[1:-1]:
        name, size, bias = d["name"], d["size"], float(d["bias"])
        gamma, beta = 1.0 + 0.3 * rng.randn(prev), 0.2 * rng.randn(prev)
        affine[name] = (gamma, beta)
        rows = size * (4 if "lstm" in d["type"] else 1)              # (an LSTM layer: all four gates at once)
        f = w[name].copy()
        Win = w[name][:rows * prev].reshape(rows, prev)
        f[:rows * prev] = (Win * gamma[None, :]).reshape(-1)
        f[rows * prev:rows * (prev + 1)] += (Win @ beta) / bias
        folded[name] = f
        prev = size
    assert set(affine) == set(case.normed)
    with_affine = autograd_stack(case.layers, w, case.frac, case.lens, normed=case.normed, affine=affine)
    absorbed = autograd_stack(case.layers, folded, case.frac, case.lens, normed=case.normed)
    plain = autograd_stack(case.layers, w, case.frac, case.lens, normed=case.normed)
    assert np.abs(with_affine[1] - absorbed[1]).max() <= 1e-12 and abs(with_affine[0] - absorbed[0]) <= 1e-12 * abs(absorbed[0])
    assert np.abs(with_affine[1] - plain[1]).max() > 1e-3           # (the gain and bias did change the net)


@pytest.mark.parametrize("which", BF16_THROUGH_NET)
def test_bf16_model_stays_within_a_third_of_the_pin(pkg, which):
    """(d) The bf16 model's distance from the fp64 stack: at most 1e-2 on the posteriors, on every gradient and on every
    propagated error (relative to the layer's maximum) for every net tests/test_gpu_layernorm.py runs through in CN_PREC_BF16."""
    case = Case(pkg, which)
    loss, post, grads, errs = case.reference()
    _, post16, grads16, errs16 = case.reference(bf16=True)
    d = {"post": float(np.abs(post16 - post).max())}
    d.update({"grad/" + k: rel(grads16[k], grads[k]) for k in grads})
    d.update({"err/" + k: rel(errs16[k], errs[k]) for k in errs})
    print(which, {k: float("%.2g" % v) for k, v in d.items()})
    assert all(v <= 1e-2 for v in d.values()), d
    assert max(d.values()) > 1e-4                                    # (the model does round)


def test_feature_is_declared():
    """(e) Both headers declare the new symbols, binding.EXPORTS lists them in front of the Adam section, the Makefile names the
    new object."""
    api = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "currennt_hip_debug.h")).read()
    assert re.search(r"\bint\s+cn_layer_set_layer_norm\(cn_layer \*layer, int enable, float eps\);", api)
    assert "Layer normalization" in api
    assert re.search(r"\bint\s+cn_dbg_layer_norm_input\(cn_layer \*layer, float \*host, size_t count\);", dbg)
    binding = open(os.path.join(ROOT, "lstm-rnn_amd", "binding.py")).read()
    exports = re.findall(r'"(cn_\w+)"', binding[binding.index("EXPORTS = ["):binding.index("]", binding.index("EXPORTS = ["))])
    assert "cn_layer_set_layer_norm" in exports and "cn_dbg_layer_norm_input" in exports
    assert exports.index("cn_dbg_layer_norm_input") < exports.index("cn_adam_update")
    makefile = open(os.path.join(ROOT, "lstm-rnn_amd", "csrc", "Makefile")).read()
    objs = next(l for l in makefile.splitlines() if l.startswith("OBJS"))
    assert "cn_layernorm.o" in objs.split() and os.path.exists(os.path.join(ROOT, "lstm-rnn_amd", "csrc", "cn_layernorm.hip"))
