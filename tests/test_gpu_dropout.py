"""-m gpu: dropout on the connections between layers (include/currennt_hip.h, section Dropout).  The masks are held bit for bit
to the numpy restatement (tests/dropout_reference.py), the step through the net to the fp64 autograd stack of
tests/test_oracle_autograd.py with the reference masks applied between the layers; then that "off" is the old path bit for bit,
what the keys select, the armed update and prefetch beside it, and the errors."""
import copy

import numpy as np
import pytest
import torch

from dropout_reference import apply, bf16_round, keep, scale
from helpers import net_desc, oracle_reference, random_sequences, random_weights, real_mask
from test_oracle_autograd import lstm_layer

pytestmark = pytest.mark.gpu

SEED, PASS = 0x1234567, 5
PRECS = ["PREC_F32", "PREC_BF16X3", "PREC_BF16"]
# posteriors max-abs, error relative, gradients and propagated errors relative to the layer's maximum
TOL = {"PREC_F32": (1e-4, 1e-4, 2e-4), "PREC_BF16X3": (1e-4, 1e-4, 2e-4), "PREC_BF16": (3e-2, 3e-2, 3e-2)}


def with_rates(layers, rates):
    out = copy.deepcopy(layers)
    for d in out:
        if d["name"] in rates:
            d["dropout"] = rates[d["name"]]
    return out


def ref_masks(layers, rates, N, seed=SEED, pass_=PASS):
    """{layer name: keep [N][size of the preceding layer]} of the layers with a non-zero rate; ordinal = index in `layers`."""
    return {d["name"]: keep(seed, i, pass_, N, layers[i - 1]["size"], rates[d["name"]])
            for i, d in enumerate(layers) if rates.get(d["name"], 0.0) > 0.0}


class Case:
    def __init__(self, pkg, P, hidden, C, PS, lens, wscale, seed, bias=1.0):
        rng = np.random.RandomState(seed)
        self.P, self.hidden, self.C, self.PS, self.lens = P, hidden, C, PS, lens
        self.layers = net_desc(P, hidden, C, bias=bias)
        self.weights = random_weights(self.layers, rng, wscale)
        self.xs, self.ts = random_sequences(rng, lens, P, C=C)
        self.frac = pkg.make_fraction(self.xs, self.ts, PS)
        self.T, self.N = self.frac["T"], self.frac["T"] * PS

    def net(self, pkg, prec, rates=None, **kw):
        return pkg.NeuralNetwork(with_rates(self.layers, rates or {}), self.weights, self.PS, self.T, precision=getattr(pkg, prec), **kw)


@pytest.fixture(scope="module")
def small(pkg):
    """7 -> lstm 6 -> blstm 10 -> softmax 5, PS 3, lengths 9 / 6 / 4: dummy frames, a pad slot (PSp = 4), H = 5 against Hp = 32 (the
    backward direction starts at unit 5: its four-column groups straddle two Philox calls), P = 7 no multiple of 4."""
    return Case(pkg, 7, [("lstm", 6), ("blstm", 10)], 5, 3, [9, 6, 4], 0.3, 31)


SMALL_RATES = {"lstm_0": 0.5, "blstm_1": 0.25, "output": 0.125}


@pytest.fixture(scope="module")
def mixed(pkg):
    """13 -> blstm 64 -> feedforward_tanh 24 -> lstm 32 -> softmax 9 (bias 0.7), PS 8 and T 17: a feed-forward layer that drops
    and one that is dropped from (ff_forward / ff_backward), more than one workgroup per launch."""
    return Case(pkg, 13, [("blstm", 64), ("feedforward_tanh", 24), ("lstm", 32)], 9, 8, [17 - (i % 5) for i in range(8)], 0.2, 22, bias=0.7)


MIXED_RATES = {"blstm_0": 0.2, "feedforward_tanh_1": 0.5, "lstm_2": 0.3, "output": 0.25}


@pytest.fixture(scope="module")
def headline(pkg):
    """39 -> blstm 250 -> blstm 250 -> softmax 20, PS 4, lengths 24 / 24 / 17 / 9: the headline layer width (H = 125, Hp = 128)."""
    return Case(pkg, 39, [("blstm", 250), ("blstm", 250)], 20, 4, [24, 24, 17, 9], 0.1, 33)


HEADLINE_RATES = {"blstm_1": 0.25, "output": 0.25}


def forward_backward(net, frac, enable=1, seed=SEED, pass_=PASS):
    net.set_dropout_pass(enable, seed, pass_)
    net.load_sequences(frac)
    net.compute_forward_pass()
    e, _ = net.error_and_correct()
    net.compute_backward_pass()
    return e


def check_masks(net, case, rates, prec, seed=SEED, pass_=PASS):
    """After a forward and a backward pass: every dropping layer's masked operand copy EQUALS the restatement applied to the
    preceding layer's outputs, and the error handed to the preceding layer is exactly zero wherever the mask drops."""
    bf16 = prec == "PREC_BF16"
    masks = ref_masks(case.layers, rates, case.N, seed, pass_)
    assert len(masks) == sum(1 for r in rates.values() if r > 0)
    real = real_mask(case.frac)
    for lay in net.layers:
        if lay.name not in masks:
            continue
        m, rate = masks[lay.name], rates[lay.name]
        x = lay.prev.outputs().reshape(case.N, -1)
        if bf16:
            x = bf16_round(x)          # (a feed-forward layer reports its fp32 outputs; its operand copy is their bf16 rounding)
        want = apply(x, m, rate, bf16)
        got = lay.dropout_input().reshape(case.N, -1)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            (prec, lay.name, int((got.view(np.uint32) != want.view(np.uint32)).sum()), float(np.abs(got - want).max()))
        assert np.abs(want[real]).max() > 0 and (want[m & real[:, None]] != 0).any()
        if lay.prev.trainable:
            e = lay.prev.output_errors().reshape(case.N, -1)
            assert np.all(e[~m] == 0), (prec, lay.name)
            for half in np.array_split(np.arange(e.shape[1]), 2):          # (a blstm's two directions)
                assert (e[:, half][m[:, half] & real[:, None]] != 0).any(), (prec, lay.name)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "mixed"])
def test_masks_bit_for_bit(pkg, small, mixed, prec, which):
    case, rates = (small, SMALL_RATES) if which == "small" else (mixed, MIXED_RATES)
    with case.net(pkg, prec, rates) as net:
        forward_backward(net, case.frac)
        check_masks(net, case, rates, prec)


def autograd_dropout(case, weights64, masks, rates):
    """The fp64 autograd stack (lstm_layer of tests/test_oracle_autograd.py, softmax, summed cross entropy) with the reference
    masks applied to each layer's input.  -> loss, posteriors of the real frames, {layer: gradient}, {layer: dL/d(outputs), real
    frames}."""
    T, PS, C = case.T, case.PS, case.C
    params = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in weights64.items()}
    lens = list(case.lens) + [0] * (PS - len(case.lens))

    def drop(h, name):
        if name not in masks:
            return h
        return h * torch.tensor(masks[name].reshape(T, PS, -1).astype(np.float64) * float(scale(rates[name])))

    h = torch.tensor(case.frac["inputs"].reshape(T, PS, case.P).astype(np.float64))
    prev, outs = case.P, {}
    for i, (kind, size) in enumerate(case.hidden):
        name = "%s_%d" % (kind, i)
        h = lstm_layer(drop(h, name), lens, params[name], prev, size, kind == "blstm", 1.0)
        h.retain_grad()
        outs[name] = h
        prev = size
    wo = params["output"]
    z = drop(h, "output") @ wo[:C * prev].reshape(C, prev).T + 1.0 * wo[C * prev:]
    logp = torch.log_softmax(z, dim=2)
    tc = torch.tensor(case.frac["targetClasses"].reshape(T, PS).astype(np.int64))
    loss = -(logp.gather(2, tc.clamp(min=0).unsqueeze(2)).squeeze(2) * (tc >= 0)).sum()
    loss.backward()
    real = real_mask(case.frac)
    post = torch.exp(logp).detach().numpy().reshape(-1, C)[real]
    return (float(loss.detach()), post, {k: v.grad.numpy() for k, v in params.items()},
            {k: v.grad.numpy().reshape(T * PS, -1)[real] for k, v in outs.items()})


def flat_weights(case):
    return {n: np.concatenate([np.asarray(w[k], np.float64).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in case.weights.items()}


@pytest.fixture(scope="module")
def small_fp64(small):
    return autograd_dropout(small, flat_weights(small), ref_masks(small.layers, SMALL_RATES, small.N), SMALL_RATES)


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


@pytest.mark.parametrize("prec", PRECS)
def test_parity_through_the_net(pkg, small, small_fp64, prec):
    loss, post, grads, errs = small_fp64
    t_post, t_err, t_grad = TOL[prec]
    real = real_mask(small.frac)
    with small.net(pkg, prec, SMALL_RATES) as net:
        e = forward_backward(net, small.frac)
        d = {"post": float(np.abs(net.outputs().reshape(-1, small.C)[real] - post).max()), "error": abs(e - loss) / max(1.0, abs(loss))}
        for lay in net.trainable_layers():
            d["grad/" + lay.name] = rel(lay.weight_updates(), grads[lay.name])
            if lay.name in errs:
                d["err/" + lay.name] = rel(lay.output_errors().reshape(small.N, -1)[real], errs[lay.name])
    print(prec, {k: float("%.2g" % v) for k, v in d.items()})
    assert d["post"] < t_post and d["error"] <= t_err, d
    assert all(v < t_grad for k, v in d.items() if k[:4] in ("grad", "err/")), d


@pytest.mark.parametrize("prec", PRECS)
def test_first_layer_alone_equals_premasked_inputs(pkg, orc, small, prec):
    """Rate 0.5 on the first hidden layer only (its predecessor is the input layer: no error is handed back): the same net fed
    the pre-masked inputs through the unchanged fp32 reference gives the same posteriors and gradients."""
    rates = {"lstm_0": 0.5}
    m = ref_masks(small.layers, rates, small.N)["lstm_0"]
    frac = dict(small.frac)
    frac["inputs"] = apply(small.frac["inputs"], m, 0.5)
    want = oracle_reference(orc, small.layers, small.weights, frac, small.PS)
    t_post, t_err, t_grad = TOL[prec]
    real = real_mask(small.frac)
    with small.net(pkg, prec, rates) as net:
        e = forward_backward(net, small.frac)
        d = {"post": float(np.abs(net.outputs().reshape(-1, small.C)[real] - want["post"]).max()),
             "error": abs(e - want["error"]) / max(1.0, abs(want["error"]))}
        for lay in net.trainable_layers():
            d["grad/" + lay.name] = rel(lay.weight_updates(), want["grad/" + lay.name])
            if "err/" + lay.name in want:
                d["err/" + lay.name] = rel(lay.output_errors().reshape(small.N, -1)[real], want["err/" + lay.name])
    print(prec, {k: float("%.2g" % v) for k, v in d.items()})
    assert d["post"] < t_post and d["error"] <= t_err, d
    assert all(v < t_grad for k, v in d.items() if k[:4] in ("grad", "err/")), d


def kernels_of(net):
    return [(lay.name, net.lib.cn_layer_recurrent_kernel(lay.handle, b).decode()) for lay in net.layers if lay.type in ("lstm", "blstm") for b in (0, 1)]


def test_headline_width(pkg, headline):
    """bf16, the headline layer width: dropout changes no kernel choice, the masks are the restatement's, the posteriors stay
    within 3e-2 of the fp64 stack."""
    masks = ref_masks(headline.layers, HEADLINE_RATES, headline.N)
    _, post, _, _ = autograd_dropout(headline, flat_weights(headline), masks, HEADLINE_RATES)
    with headline.net(pkg, "PREC_BF16") as plain:
        forward_backward(plain, headline.frac)
        names = kernels_of(plain)
        assert plain.recurrent_kernel(False) and plain.recurrent_kernel(True)
        first = (plain.recurrent_kernel(False), plain.recurrent_kernel(True))
    with headline.net(pkg, "PREC_BF16", HEADLINE_RATES) as net:
        forward_backward(net, headline.frac)
        assert kernels_of(net) == names and (net.recurrent_kernel(False), net.recurrent_kernel(True)) == first
        check_masks(net, headline, HEADLINE_RATES, "PREC_BF16")
        y = net.outputs().reshape(-1, headline.C)[real_mask(headline.frac)]
    assert np.abs(y - post).max() < 3e-2, float(np.abs(y - post).max())


def one_step(net, frac, enable, lr=1e-2, mom=0.9):
    forward_backward(net, frac, enable)
    out = {"post": net.outputs()}
    for lay in net.trainable_layers():
        out["grad/" + lay.name] = lay.weight_updates()
    net.update_weights(lr, mom)
    for lay in net.trainable_layers():
        out["w/" + lay.name] = lay.weights()
    return out


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
def test_off_means_off(pkg, mixed, prec):
    """Deterministic mode: rates set but not enabled, and enabled with every rate 0, are each the net built without "dropout"."""
    with mixed.net(pkg, prec, deterministic=True) as net:
        want = one_step(net, mixed.frac, 0)
    runs = {"rates set, not enabled": (MIXED_RATES, 0), "enabled, every rate 0": ({k: 0.0 for k in MIXED_RATES}, 1)}
    for what, (rates, enable) in runs.items():
        with mixed.net(pkg, prec, rates, deterministic=True) as net:
            got = one_step(net, mixed.frac, enable)
            with pytest.raises(pkg.CurrenntHipError) as ei:
                net.layer("output").dropout_input()
            assert ei.value.code == -4
        for k in want:
            assert np.array_equal(got[k], want[k]), (what, k)
    with mixed.net(pkg, prec, MIXED_RATES, deterministic=True) as net:          # ... and enabled, the rates do change the step
        got = one_step(net, mixed.frac, 1)
    assert all(not np.array_equal(got[k], want[k]) for k in want if not k.startswith("w/"))


def test_keys(pkg, small):
    def run(seed, pass_, between=None):
        with small.net(pkg, "PREC_F32", SMALL_RATES, deterministic=True) as net:
            net.set_dropout_pass(1, seed, pass_)
            net.load_sequences(small.frac); net.compute_forward_pass()
            if between is not None:
                net.set_dropout_pass(1, seed, between)
            net.compute_backward_pass()
            out = {"in/" + l.name: l.dropout_input() for l in net.trainable_layers()}
            out.update({"grad/" + l.name: l.weight_updates() for l in net.trainable_layers()})
            return out
    a, b = run(SEED, PASS), run(SEED, PASS)
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)
    for other in (run(SEED, PASS + 1), run(SEED + 1, PASS), run(SEED, PASS + (1 << 32)), run(SEED + (1 << 32), PASS)):
        assert all(not np.array_equal(a[k], other[k]) for k in a if k.startswith("in/"))
    torn = run(SEED, PASS, between=PASS + 1)          # the backward pass goes by the forward pass's record
    assert all(np.array_equal(a[k], torn[k]) for k in a)


def train(net, fracs, mode, steps=3, lr=1e-2, mom=0.9):
    for step in range(steps):
        frac = fracs[step % len(fracs)]
        net.set_dropout_pass(1, SEED, step)
        net.load_sequences(frac)
        net.compute_forward_pass()
        if mode == "prefetch" and step + 1 < steps:
            net.prefetch_sequences(fracs[(step + 1) % len(fracs)])
        if mode == "armed":
            net.arm_update(lr, mom)
        net.compute_backward_pass()
        if mode == "armed":
            net.update_weights_fused(lr, mom)
        else:
            net.update_weights(lr, mom)
    out = {l.name: l.weights() for l in net.trainable_layers()}
    out["hits"] = net.prefetch_hits()
    return out


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
def test_with_the_rest_of_the_step(pkg, mixed, prec):
    """Three steps over two fractions in deterministic mode: the armed, fused update and the prefetched loads each end in the
    weights of the plain sequence (load, forward, backward, update_weights) with the same keys, bit for bit."""
    rng = np.random.RandomState(5)
    xs, ts = random_sequences(rng, [17 - ((i + 2) % 5) for i in range(8)], mixed.P, C=mixed.C)
    fracs = [mixed.frac, pkg.make_fraction(xs, ts, mixed.PS)]
    res = {}
    for mode in ("plain", "armed", "prefetch"):
        with mixed.net(pkg, prec, MIXED_RATES, deterministic=True) as net:
            res[mode] = train(net, fracs, mode)
    assert res["prefetch"]["hits"] == 2 and res["plain"]["hits"] == 0
    for mode in ("armed", "prefetch"):
        for name, w in res["plain"].items():
            if name != "hits":
                assert np.array_equal(res[mode][name], w), (mode, name)
    flat = {n: np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in mixed.weights.items()}
    assert all(np.abs(res["plain"][n] - flat[n]).max() > 1e-4 for n in flat)


def test_errors(pkg, small):
    with small.net(pkg, "PREC_F32", SMALL_RATES) as net:
        lib = net.lib
        for lay in net.trainable_layers():
            for bad in (-0.1, 1.0, float("nan")):
                assert lib.cn_layer_set_dropout(lay.handle, bad) == -1
            assert lay.dropout == SMALL_RATES[lay.name]
        assert lib.cn_layer_set_dropout(net.layers[0].handle, 0.5) == -1           # an input layer
        assert lib.cn_layer_set_dropout(net.layers[-1].handle, 0.5) == -1          # a post output layer
        assert b"dropout" in lib.cn_last_error(net.ctx)
        forward_backward(net, small.frac, enable=0)
        for lay in net.trainable_layers():
            with pytest.raises(pkg.CurrenntHipError) as ei:
                lay.dropout_input()
            assert ei.value.code == -4
        forward_backward(net, small.frac, enable=1)                                 # the rejected rates changed nothing
        check_masks(net, small, SMALL_RATES, "PREC_F32")
        net.layer("blstm_1").set_dropout(0.0)                                       # rate 0 takes a layer off the path again
        forward_backward(net, small.frac, enable=1)
        with pytest.raises(pkg.CurrenntHipError):
            net.layer("blstm_1").dropout_input()
        check_masks(net, small, {"lstm_0": 0.5, "output": 0.125}, "PREC_F32")
    with pytest.raises(RuntimeError, match="dropout.*'lstm_0'"):
        small.net(pkg, "PREC_F32", {"lstm_0": 1.5})
    for name in ("input", "postoutput"):                                            # (as the C++ driver: tests/test_driver_dropout.py)
        with pytest.raises(RuntimeError, match="dropout.*'%s'" % name):
            small.net(pkg, "PREC_F32", {name: 0.2})
