"""-m gpu: layer normalization of a layer's input (include/currennt_hip.h, section Layer normalization).  The normalised copy is
held per element to the float64 rule (tests/layernorm_reference.py) inside the bound that section derives, the step through the
net to the fp64 autograd stack with LN in front of the marked layers' weighted paths; then LN together with residual connections,
dropout, Adam, clipping and prefetch, that "off" is the old path bit for bit, and the errors."""
import copy
import ctypes as C

import numpy as np
import pytest

from dropout_reference import bf16_round, scale
from helpers import net_desc, random_sequences, random_weights, real_mask
from layernorm_reference import BF16_THROUGH_NET, CASES, Case, layer_norm_bound, layer_norm_rule, rel, stack_results
from test_gpu_dropout import TOL, ref_masks

pytestmark = pytest.mark.gpu

PRECS = ["PREC_F32", "PREC_BF16X3", "PREC_BF16"]
_cases = {}


@pytest.fixture(scope="module")
def case_of(pkg):
    """The nets of layernorm_reference.CASES, each built (and its fp64 stack computed) once."""
    def get(which):
        if which not in _cases:
            _cases[which] = Case(pkg, which)
        return _cases[which]
    return get


def forward_backward(net, frac):
    net.load_sequences(frac)
    net.compute_forward_pass()
    e, _ = net.error_and_correct()
    net.compute_backward_pass()
    return e


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the normalised copy, per element ------------------------------------------------------------------------------------------
def check_normalized(lay, N, real, bf16, eps=1e-5):
    """lay.normalized_input() against the float64 rule evaluated on the operand values the layer read."""
    x = lay.prev.outputs().reshape(N, -1)
    if bf16:
        x = bf16_round(x)              # (a feed-forward layer reports its fp32 outputs; its operand copy is their bf16 rounding)
    want, mu, rho = layer_norm_rule(x, real, eps)
    got = lay.normalized_input().reshape(N, -1).astype(np.float64)
    assert got.shape == want.shape
    excess = np.abs(got - want) - layer_norm_bound(want, mu, rho, bf16)
    assert np.all(excess[real] <= 0), (lay.name, float(excess[real].max()), float(np.abs(got - want)[real].max()))
    assert np.all(got[~real] == 0), lay.name                                       # rows that are not real frames: exactly zero
    return got, want


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", list(CASES))
def test_normalized_copy_per_element(pkg, case_of, prec, which):
    case = case_of(which)
    real = real_mask(case.frac)
    with case.net(pkg, prec) as net:
        net.load_sequences(case.frac)
        net.compute_forward_pass()
        seen = 0
        for lay in net.layers:
            if lay.name not in case.normed:
                continue
            got, want = check_normalized(lay, case.N, real, prec == "PREC_BF16")
            # (the check can tell: the rows have mean 0 up to the operand type's rounding, and they are not the input)
            assert np.abs(got[real].mean(axis=1)).max() < 2e-2 and np.abs(want[real]).max() > 0.5, lay.name
            seen += 1
        assert seen == len(case.normed) and (~real).any()
        for lay in net.layers:                                                         # an unmarked layer has no copy to report
            if lay.trainable and lay.name not in case.normed:
                with pytest.raises(pkg.CurrenntHipError) as ei:
                    lay.normalized_input()
                assert ei.value.code == -4


@pytest.mark.parametrize("prec", PRECS)
def test_degenerate_rows(pkg, prec):
    """LN on the first layer with hand-made input rows: a constant row and an all-zero row give exact zeros; a row of 1000 + 0.01 *
    randn (|mean| * rstd ~ 1e5) stays inside the bound, which a one-pass variance or a mean taken in fp32 does not."""
    P, PS, T = 40, 2, 4
    rng = np.random.RandomState(48)
    layers = net_desc(P, [("lstm", 4)], 3)
    layers[1]["layer_norm"] = True
    xs = [rng.randn(T, P).astype(np.float32), rng.randn(T - 1, P).astype(np.float32)]
    xs[0][0] = 3.25                                        # constant
    xs[0][1] = 0.0                                         # all zero
    xs[0][2] = (1000.0 + 0.01 * rng.randn(P)).astype(np.float32)
    xs[1][0] = -7.5
    xs[1][1] = (1000.0 + 0.01 * rng.randn(P)).astype(np.float32)
    ts = [rng.randint(0, 3, len(x)).astype(np.int32) for x in xs]
    frac = pkg.make_fraction(xs, ts, PS)
    real = real_mask(frac)
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.3), PS, T, precision=getattr(pkg, prec)) as net:
        net.load_sequences(frac)
        net.compute_forward_pass()
        got, want = check_normalized(net.layer("lstm_0"), T * PS, real, prec == "PREC_BF16")
        got = got.reshape(T, PS, P)
        assert np.all(got[0, 0] == 0) and np.all(got[1, 0] == 0) and np.all(got[0, 1] == 0)
        if prec == "PREC_BF16":        # (bf16 is 4 apart at 1000: the operand copy of such a row is constant, and so normalises to zeros)
            assert np.all(got[2, 0] == 0) and np.all(got[1, 1] == 0) and np.all(want.reshape(T, PS, P)[2, 0] == 0)
        else:
            assert np.abs(got[2, 0]).max() > 0.5 and np.abs(got[1, 1]).max() > 0.5
        assert np.isfinite(net.outputs()).all()


# ---- 2. parity through the net against the fp64 stack -----------------------------------------------------------------------------
def distances(net, case, want):
    loss, post, grads, errs = want
    real = real_mask(case.frac)
    e = forward_backward(net, case.frac)
    d = {"post": float(np.abs(net.outputs().reshape(-1, case.C)[real] - post).max()), "error": abs(e - loss) / max(1.0, abs(loss))}
    for lay in net.trainable_layers():
        d["grad/" + lay.name] = rel(lay.weight_updates(), grads[lay.name])
        if lay.name in errs:
            d["err/" + lay.name] = rel(lay.output_errors().reshape(case.N, -1)[real], errs[lay.name])
    return d


def assert_inside(d, prec):
    t_post, t_err, t_grad = TOL[prec]
    assert d["post"] < t_post and d["error"] <= t_err, d
    assert all(v < t_grad for k, v in d.items() if k[:4] in ("grad", "err/")), d


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide", "headline", "first"])
def test_parity_through_the_net(pkg, case_of, prec, which):
    """Posteriors, error, every gradient and every propagated error within DESIGN section 3's table.  CN_PREC_BF16: the nets whose
    bf16 model stays within 1e-2 of the fp64 stack (tests/test_layernorm_reference.py); "small", four normalised layers of 10
    units, is at 1.8e-2 there and is no bf16 case."""
    if prec == "PREC_BF16" and which not in BF16_THROUGH_NET:
        return
    case = case_of(which)
    with case.net(pkg, prec) as net:
        d = distances(net, case, case.reference())
    print(which, prec, {k: float("%.2g" % v) for k, v in d.items()})
    assert_inside(d, prec)
    assert sum(k.startswith("err/") for k in d) == len(case.hidden)


# ---- 3. together with the rest -----------------------------------------------------------------------------------------------------
SEED, PASS = 0x7654321, 9
TOGETHER_HIDDEN = [("lstm", 10), ("blstm", 10), ("lstm", 10)]
TOGETHER_NORMED = ("blstm_1", "lstm_2", "output")
TOGETHER_RATES = {"blstm_1": 0.3, "output": 0.2}


@pytest.fixture(scope="module")
def together(pkg):
    """7 -> lstm 10 -> blstm 10 (LN, residual, dropout 0.3) -> lstm 10 (LN) -> softmax 5 (LN, dropout 0.2), PS 3, lengths 9 / 6 / 4."""
    rng = np.random.RandomState(49)
    layers = net_desc(7, TOGETHER_HIDDEN, 5)
    weights = random_weights(layers, rng, 0.3)
    lens = [9, 6, 4]
    xs, ts = random_sequences(rng, lens, 7, C=5)
    frac = pkg.make_fraction(xs, ts, 3)
    desc = copy.deepcopy(layers)
    for d in desc:
        if d["name"] in TOGETHER_NORMED:
            d["layer_norm"] = True
        if d["name"] in TOGETHER_RATES:
            d["dropout"] = TOGETHER_RATES[d["name"]]
    desc[2]["residual"] = True
    return {"layers": layers, "desc": desc, "weights": weights, "lens": lens, "frac": frac, "rng": rng}


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16X3"])
def test_together_against_the_fp64_stack(pkg, together, prec):
    """The order LN -> dropout and the un-normalised skip path: the fp64 stack with the same masks, inside TOL."""
    t = together
    frac, N = t["frac"], t["frac"]["T"] * 3
    masks = ref_masks(t["desc"], TOGETHER_RATES, N, SEED, PASS)
    drop = {k: (m, scale(TOGETHER_RATES[k])) for k, m in masks.items()}
    want = stack_results(t["layers"], t["weights"], frac, t["lens"], normed=TOGETHER_NORMED, marked=("blstm_1",), drop=drop)
    real = real_mask(frac)
    with pkg.NeuralNetwork(t["desc"], t["weights"], 3, frac["T"], precision=getattr(pkg, prec)) as net:
        net.set_dropout_pass(1, SEED, PASS)
        e = forward_backward(net, frac)
        d = {"post": float(np.abs(net.outputs().reshape(-1, 5)[real] - want[1]).max()), "error": abs(e - want[0]) / max(1.0, abs(want[0]))}
        for lay in net.trainable_layers():
            d["grad/" + lay.name] = rel(lay.weight_updates(), want[2][lay.name])
            if lay.name in want[3]:
                d["err/" + lay.name] = rel(lay.output_errors().reshape(N, -1)[real], want[3][lay.name])
        # what K1 read is the masked copy of the normalised one
        lay = net.layer("blstm_1")
        xn, xd = lay.normalized_input().reshape(N, -1), lay.dropout_input().reshape(N, -1)
        m = masks["blstm_1"]
        assert np.all(xd[~m] == 0) and np.array_equal(bits(xd[m]), bits((xn * scale(0.3))[m])) and (xn[~m & real[:, None]] != 0).any()
    print(prec, {k: float("%.2g" % v) for k, v in d.items()})
    assert_inside(d, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_together_three_steps_twice(pkg, together, prec):
    """Three steps with the armed Adam update, clipping and prefetch in deterministic mode, run twice: equal bits, finite weights."""
    t = together
    rng = np.random.RandomState(50)
    lens2 = [4, 6, 9]
    xs, ts = random_sequences(rng, lens2, 7, C=5)
    fracs = [t["frac"], pkg.make_fraction(xs, ts, 3)]
    runs = []
    for _ in range(2):
        with pkg.NeuralNetwork(t["desc"], t["weights"], 3, max(f["T"] for f in fracs), precision=getattr(pkg, prec), deterministic=True) as net:
            net.set_grad_clip(0.5)
            for step in range(3):
                net.set_dropout_pass(1, SEED, step)
                net.load_sequences(fracs[step % 2])
                net.compute_forward_pass()
                if step + 1 < 3:
                    net.prefetch_sequences(fracs[(step + 1) % 2])
                net.arm_adam(1e-2, step=step + 1)
                net.compute_backward_pass()
                net.update_weights_adam(1e-2, step=step + 1)
            runs.append({l.name: l.weights() for l in net.trainable_layers()})
            assert net.prefetch_hits() == 2
    for name, w in runs[0].items():
        assert np.isfinite(w).all(), (prec, name)
        assert np.array_equal(bits(w), bits(runs[1][name])), (prec, name)
        assert not np.array_equal(w, np.concatenate([np.asarray(t["weights"][name][k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]))


# ---- 4. off is the old path --------------------------------------------------------------------------------------------------------
LR, MOM = 1e-2, 0.9


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
def test_off_is_the_old_path(pkg, case_of, prec):
    """A description without the member, one with "layer_norm": false everywhere, and one that was switched on for a step and off
    again (on a fresh copy of the weights): bit-equal weights after one step, equal launch counts per timing class, and no
    normalised copy to report.  (The marked net differs in both: the check can tell.)"""
    case = case_of("wide")

    def run(layers, toggle=False):
        with pkg.NeuralNetwork(layers, case.weights, case.PS, case.T, precision=getattr(pkg, prec), deterministic=True) as net:
            if toggle:
                for lay in net.trainable_layers():
                    lay.set_layer_norm(True)
                forward_backward(net, case.frac)
                net.update_weights(LR, MOM)
                assert net.layer("output").normalized_input().shape == (case.T, case.PS, 64)
                for lay in net.trainable_layers():
                    lay.set_layer_norm(False)
                    lay.upload("weights", np.concatenate([np.asarray(case.weights[lay.name][k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]))
                    lay.upload("weightDeltas", np.zeros(lay.weight_count, np.float32))
            net.timing_enable(True); net.timing_reset()
            forward_backward(net, case.frac)
            net.update_weights(LR, MOM)
            counts = {k: v[1] for k, v in net.timing_read().items()}
            net.timing_enable(False)
            if not any(d.get("layer_norm") for d in layers):
                for lay in net.trainable_layers():
                    with pytest.raises(pkg.CurrenntHipError) as ei:
                        lay.normalized_input()
                    assert ei.value.code == -4
            return {l.name: l.weights() for l in net.trainable_layers()}, counts
    absent, absent_n = run(case.layers)
    off, off_n = run(case.desc(normed=(), member=True))
    assert all(d.get("layer_norm") is False for d in case.desc(normed=(), member=True) if "bias" in d) and all("layer_norm" not in d for d in case.layers)
    toggled, toggled_n = run(case.layers, toggle=True)
    assert off_n == absent_n and toggled_n == absent_n
    for name in absent:
        assert np.array_equal(bits(off[name]), bits(absent[name])), (prec, name)
        assert np.array_equal(bits(toggled[name]), bits(absent[name])), (prec, name)
    on, on_n = run(case.desc())
    # three marked layers, two of them behind a trainable layer ... the third too: 3 forward and 3 backward launches
    assert on_n["other"] == absent_n["other"] + 6 and {k: v for k, v in on_n.items() if k != "other"} == {k: v for k, v in absent_n.items() if k != "other"}
    assert all(not np.array_equal(on[name], absent[name]) for name in absent)


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(pkg, case_of):
    BAD_ARG, SHAPE = -1, -2
    case = case_of("small")
    with case.net(pkg, "PREC_F32") as net:
        lib = net.lib
        for name in ("input", "postoutput"):
            assert lib.cn_layer_set_layer_norm(net.layer(name).handle, 1, 1e-5) == BAD_ARG, name
            assert b"only lstm, blstm, feedforward_* and softmax" in lib.cn_last_error(net.ctx)
        for eps in (0.0, -1e-5, float("nan"), float("inf")):
            assert lib.cn_layer_set_layer_norm(net.layer("lstm_3").handle, 1, eps) == BAD_ARG, eps
            assert b"eps must be finite and > 0" in lib.cn_last_error(net.ctx)
        # the refused calls changed nothing
        net.load_sequences(case.frac)
        net.compute_forward_pass()
        lay = net.layer("lstm_3")
        assert lay.layer_norm and lay.normalized_input().shape == (case.T, case.PS, 10)
        buf = np.empty(case.N * 10 + 1, np.float32)
        assert lib.cn_dbg_layer_norm_input(lay.handle, buf.ctypes.data_as(C.c_void_p), case.N * 10 + 1) == SHAPE
        assert lib.cn_dbg_layer_norm_input(lay.handle, buf.ctypes.data_as(C.c_void_p), case.N * 10 - 1) == SHAPE
    # a preceding layer of size 1
    layers = net_desc(1, [("lstm", 4), ("lstm", 1)], 3)
    with pkg.NeuralNetwork(layers, None, 2, 4, seed=1) as net:
        for name in ("lstm_0", "output"):
            assert net.lib.cn_layer_set_layer_norm(net.layer(name).handle, 1, 1e-5) == BAD_ARG, name
            assert b"at least 2 units" in net.lib.cn_last_error(net.ctx)
        assert net.lib.cn_layer_set_layer_norm(net.layer("lstm_1").handle, 1, 1e-5) == 0
    # the Python mirror refuses a description as the C++ driver does (tests/test_driver_layernorm.py), with the same texts
    for name, text in (("input", "only lstm, blstm, feedforward_\\* and softmax layers normalise their input"),
                       ("postoutput", "only lstm, blstm, feedforward_\\* and softmax layers normalise their input")):
        with pytest.raises(RuntimeError, match="Invalid value 'layer_norm' in layer '%s': %s" % (name, text)):
            case.net(pkg, "PREC_F32", normed=(name,))
    bad = case.desc()
    bad[2]["layer_norm"] = 1
    with pytest.raises(RuntimeError, match="Invalid value 'layer_norm' in layer 'blstm_1': true or false expected"):
        pkg.NeuralNetwork(bad, case.weights, case.PS, case.T)
    bad = case.desc()
    bad[2]["layer_norm_eps"] = 0.0
    with pytest.raises(RuntimeError, match="Invalid value 'layer_norm_eps' in layer 'blstm_1': a finite number above 0 expected"):
        pkg.NeuralNetwork(bad, case.weights, case.PS, case.T)
    layers[1]["layer_norm"] = True
    with pytest.raises(RuntimeError, match="Invalid value 'layer_norm' in layer 'lstm_0': the preceding layer's size 1 is below 2"):
        pkg.NeuralNetwork(layers, None, 2, 4, seed=1)
