"""-m gpu: context layers (include/currennt_hip.h, section Context layers).  The gather and the fold are held bit for bit to the
restated rule (tests/context_reference.py), a context layer behind the input layer to what input splicing produces, the step
through the net to the fp64 autograd stack with a context step between the layers; then run-to-run bits, the armed update with
prefetch beside it, the other input features on a context layer's follower, and the errors."""
import copy
import ctypes as C

import numpy as np
import pytest

from context_reference import Case, context_backward, context_forward, stack_results
from dropout_reference import bf16_round, keep, scale
from helpers import random_sequences, real_mask
from residual_reference import flat_weights
from test_gpu_dropout import TOL

pytestmark = pytest.mark.gpu

PRECS = ["PREC_F32", "PREC_BF16X3", "PREC_BF16"]


@pytest.fixture(scope="module")
def case_of(pkg):
    cache = {}

    def get(which):
        if which not in cache:
            cache[which] = Case(pkg, which)
        return cache[which]
    return get


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def forward_backward(net, frac):
    net.load_sequences(frac)
    net.compute_forward_pass()
    e, _ = net.error_and_correct()
    net.compute_backward_pass()
    return e


def context_layers(net):
    return [l for l in net.layers if l.type == "context"]


# ---- 1. the gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide", "from_input"])
def test_forward_bit_for_bit(pkg, case_of, prec, which):
    case = case_of(which)
    real = real_mask(case.frac)
    assert (~real).any()
    kinds = set()
    with case.net(pkg, prec) as net:
        net.load_sequences(case.frac)
        net.compute_forward_pass()
        assert len(context_layers(net)) == sum(t == "context" for t, _ in case.hidden)
        for lay in context_layers(net):
            L, R, D = lay.context()
            assert (L, R, D) == (lay.desc["left"], lay.desc["right"], lay.desc["dilation"]) and lay.size == (L + R + 1) * lay.prev.size
            x = lay.prev.outputs()
            if prec == "PREC_BF16":
                x = bf16_round(x)      # (a feed-forward predecessor reports its fp32 outputs; its operand copy is their bf16 rounding)
            want = context_forward(x, case.lens, L, R, D).reshape(case.N, -1)
            got = lay.outputs().reshape(case.N, -1)
            assert np.array_equal(bits(got), bits(want)), (prec, lay.name, int((bits(got) != bits(want)).sum()), float(np.abs(got - want).max()))
            assert np.all(bits(got[~real]) == 0) and np.abs(got[real]).max() > 0
            if lay.prev.type.startswith("feedforward"):
                assert np.all(x.reshape(case.N, -1)[~real] != 0)                           # (act(bias): it must not come through)
            kinds.add(lay.prev.type)
    assert kinds == {"small": {"lstm", "blstm", "feedforward_tanh"}, "wide": {"blstm", "feedforward_tanh"}, "from_input": {"input"}}[which]


# ---- 2. behind the input layer: what input splicing produces --------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_behind_the_input_layer_is_input_splicing(pkg, case_of, prec):
    case = case_of("from_input")
    t_post, _, t_grad = TOL[prec]
    real = real_mask(case.frac)
    spliced = copy.deepcopy([d for d in case.layers if d["type"] != "context"])
    spliced[0]["size"] = 6 * case.P
    with case.net(pkg, prec) as net, pkg.NeuralNetwork(spliced, case.weights, case.PS, case.T, precision=getattr(pkg, prec)) as ref:
        ref.set_input_splice(context=(2, 3), frame_skip=1)
        forward_backward(net, case.frac)
        forward_backward(ref, case.frac)
        got, want = net.layer("context_0").outputs(), ref.input_layer().outputs()
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)) and np.abs(want).max() > 0
        d = {"post": float(np.abs(net.outputs().reshape(-1, case.C)[real] - ref.outputs().reshape(-1, case.C)[real]).max())}
        for lay in net.trainable_layers():
            d["grad/" + lay.name] = rel(lay.weight_updates(), ref.layer(lay.name).weight_updates())
    print(prec, d)
    assert d["post"] < t_post and all(v < t_grad for k, v in d.items() if k != "post"), d


# ---- 3. the fold -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_backward_bit_for_bit(pkg, case_of, prec, which):
    case = case_of(which)
    real = real_mask(case.frac)
    rng = np.random.RandomState(6)
    kinds = set()
    with case.net(pkg, prec) as net:
        net.load_sequences(case.frac)
        net.compute_forward_pass()
        for lay in context_layers(net):
            L, R, D = lay.context()
            e = (rng.randn(case.T, case.PS, lay.size) + 0.5).astype(np.float32)
            assert np.all(e.reshape(case.N, -1)[~real] != 0)                              # (non-zero on dummy rows: they are not read)
            lay.write_output_errors(e)
            lay.backward()
            want = context_backward(e, case.lens, L, R, D).reshape(case.N, -1)
            got = lay.prev.output_errors().reshape(case.N, -1)
            assert np.array_equal(bits(got), bits(want)), (prec, lay.name, int((bits(got) != bits(want)).sum()), float(np.abs(got - want).max()))
            assert np.all(bits(got[~real]) == 0) and np.all(got[real] != 0)
            kinds.add(lay.prev.type)
    assert {"blstm", "feedforward_tanh"} <= kinds


@pytest.mark.parametrize("prec", PRECS)
def test_backward_behind_the_input_layer_is_a_no_op(pkg, case_of, prec):
    case = case_of("from_input")
    with case.net(pkg, prec) as net:
        net.load_sequences(case.frac)
        net.compute_forward_pass()
        lay = net.layer("context_0")
        before = lay.outputs()
        lay.write_output_errors(np.ones((case.N, lay.size), np.float32))
        lay.backward()
        assert np.array_equal(bits(lay.outputs()), bits(before)) and np.all(lay.output_errors() == 1)
        with pytest.raises(pkg.CurrenntHipError):
            lay.prev.output_errors()                                                     # (the input layer has none)


# ---- 4. the step through the net ---------------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("which", ["small", "wide"])
def test_parity_through_the_net(pkg, case_of, prec, which):
    """Posteriors, error, every gradient and every trainable layer's propagated error against the fp64 autograd stack, within the
    project's table for a step through a small net (TOL of tests/test_gpu_dropout.py)."""
    case = case_of(which)
    with case.net(pkg, prec) as net:
        d = distances(net, case, case.reference())
    print(which, prec, {k: float("%.2g" % v) for k, v in d.items()})
    assert sum(k.startswith("err/") for k in d) == sum(t != "context" for t, _ in case.hidden)
    assert_inside(d, prec)


# ---- 5. run to run -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_two_runs_give_the_same_bits(pkg, case_of, prec, which):
    case = case_of(which)
    runs = []
    for _ in range(2):
        with case.net(pkg, prec, deterministic=True) as net:
            forward_backward(net, case.frac)
            out = {"grad/" + l.name: l.weight_updates() for l in net.trainable_layers()}
            out.update({"err/" + l.name: l.output_errors() for l in context_layers(net)})
            runs.append(out)
    assert sum(k.startswith("err/") for k in runs[0]) >= 2
    for k, v in runs[0].items():
        assert np.array_equal(bits(v), bits(runs[1][k])) and np.abs(v).max() > 0, (prec, k)


# ---- 6. the armed update ---------------------------------------------------------------------------------------------------------------
LR, MOM = 1e-2, 0.9


def test_armed_update_is_the_unarmed_loop(pkg, case_of):
    """Three steps over two fractions in deterministic CN_PREC_F32: armed, with the next fraction announced beside the backward
    pass, against backward on every layer followed by the update of all layers -- the same weights, bit for bit.  (The fork and
    join decisions of the backward passes go by "does the preceding layer take an error", which a context layer passes on.)"""
    case = case_of("small")
    rng = np.random.RandomState(7)
    xs, ts = random_sequences(rng, list(reversed(case.lens)), case.P, C=case.C)
    fracs = [case.frac, pkg.make_fraction(xs, ts, case.PS)]

    def run(armed):
        with case.net(pkg, "PREC_F32", deterministic=True) as net:
            for step in range(3):
                net.load_sequences(fracs[step % 2])
                net.compute_forward_pass()
                if armed:
                    if step + 1 < 3:
                        net.prefetch_sequences(fracs[(step + 1) % 2])
                    net.arm_update(LR, MOM)
                net.compute_backward_pass()
                net.update_weights_fused(LR, MOM)
            assert net.prefetch_hits() == (2 if armed else 0)
            return {l.name: l.weights() for l in net.trainable_layers()}
    armed, plain = run(True), run(False)
    w0 = flat_weights(case.weights)
    for name, w in plain.items():
        assert np.array_equal(bits(armed[name]), bits(w)), name
        assert np.abs(w - w0[name]).max() > 1e-4


# ---- 7. with the other input features ----------------------------------------------------------------------------------------------------
SEED, PASS = 0x2468ACE, 3


@pytest.mark.parametrize("prec", PRECS)
def test_follower_drops_normalises_and_is_residual(pkg, case_of, prec):
    """blstm 6 -> context(1, 1) -> feedforward_tanh 18 with dropout 0.2, layer_norm and residual: the follower reads, normalises
    and adds the context layer's output like any other predecessor's."""
    case = case_of("features")
    name, rate = "feedforward_tanh_2", 0.2
    desc = copy.deepcopy(case.layers)
    idx = [d["name"] for d in desc].index(name)
    desc[idx].update({"dropout": rate, "layer_norm": True, "residual": True})
    assert desc[idx - 1]["type"] == "context" and desc[idx - 1]["size"] == desc[idx]["size"] == 18
    mask = keep(SEED, idx, PASS, case.N, 18, rate)
    want = stack_results(case.layers, case.weights, case.frac, case.lens, normed=(name,), marked=(name,), drop={name: (mask, scale(rate))})
    with case.net(pkg, prec, layers=desc) as net:
        net.set_dropout_pass(1, SEED, PASS)
        d = distances(net, case, want)
        lay = net.layer(name)
        assert lay.residual and lay.layer_norm and np.all(lay.dropout_input().reshape(case.N, -1)[~mask] == 0)
    print(prec, {k: float("%.2g" % v) for k, v in d.items()})
    assert_inside(d, prec)


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors(pkg, case_of):
    BAD_ARG = -1
    case = case_of("small")
    with case.net(pkg, "PREC_F32") as net:
        lib, prev = net.lib, net.layer("lstm_0")
        h = C.c_void_p()
        for left, right, dil in ((-1, 0, 1), (0, 33, 1), (1, 1, 0), (1, 1, 17)):
            assert lib.cn_layer_create_context(net.ctx, prev.handle, left, right, dil, C.byref(h)) == BAD_ARG and not h.value, (left, right, dil)
            assert b"cn_layer_create_context" in lib.cn_last_error(net.ctx)
        assert lib.cn_layer_create(net.ctx, pkg.KIND_CONTEXT, prev.handle, 30, 0.0, 0, 0, C.byref(h)) == BAD_ARG and not h.value
        assert b"cn_layer_create_context" in lib.cn_last_error(net.ctx)
        ctx = net.layer("context_1")
        assert lib.cn_layer_set_dropout(ctx.handle, 0.5) == BAD_ARG and b"only lstm, blstm" in lib.cn_last_error(net.ctx)
        assert lib.cn_layer_set_residual(ctx.handle, 1) == BAD_ARG and b"only lstm, blstm" in lib.cn_last_error(net.ctx)
        assert lib.cn_layer_set_layer_norm(ctx.handle, 1, 1e-5) == BAD_ARG and b"only lstm, blstm" in lib.cn_last_error(net.ctx)
        w = np.zeros(4, np.float32)
        assert lib.cn_layer_set_weights(ctx.handle, w.ctypes.data_as(C.c_void_p), 4) == BAD_ARG and b"has no weights" in lib.cn_last_error(net.ctx)
        assert lib.cn_layer_weight_count(ctx.handle) == 0 and lib.cn_layer_kind_of(ctx.handle) == pkg.KIND_CONTEXT
        # a post output layer directly behind a context layer
        assert lib.cn_layer_create(net.ctx, pkg.LAYER_KINDS["sse"], ctx.handle, ctx.size, 0.0, 0, 0, C.byref(h)) == BAD_ARG and not h.value
        assert b"needs a trainable preceding layer" in lib.cn_last_error(net.ctx)
        # the members of another kind
        l, r, d = C.c_int(), C.c_int(), C.c_int()
        assert lib.cn_layer_context(prev.handle, C.byref(l), C.byref(r), C.byref(d)) == BAD_ARG
        assert lib.cn_layer_context(ctx.handle, C.byref(l), C.byref(r), C.byref(d)) == 0 and (l.value, r.value, d.value) == (2, 1, 1)
        with pytest.raises(pkg.CurrenntHipError) as ei:
            prev.context()
        assert ei.value.code == BAD_ARG
    # the mirror: members out of range come back with the library's code, a size that is not B * P with the reference's text
    for member, value in (("left", -1), ("right", 33), ("dilation", 0), ("dilation", 17)):
        desc = copy.deepcopy(case.layers)
        desc[2][member] = value
        desc[2]["size"] = (desc[2]["left"] + desc[2]["right"] + 1) * desc[1]["size"]
        with pytest.raises(pkg.CurrenntHipError) as ei:
            case.net(pkg, "PREC_F32", layers=desc)
        assert ei.value.code == BAD_ARG, (member, value)
    desc = copy.deepcopy(case.layers)
    desc[2]["size"] += 1
    with pytest.raises(RuntimeError, match="Size mismatch: 41 vs. 40 in layer 'context_1'"):
        case.net(pkg, "PREC_F32", layers=desc)
    # the members are optional: no frames to the left, none to the right, dilation 1
    layers = [{"name": "in", "type": "input", "size": 3}, {"name": "l", "type": "lstm", "size": 4, "bias": 1.0},
              {"name": "c", "type": "context", "size": 4}, {"name": "out", "type": "softmax", "size": 3, "bias": 1.0},
              {"name": "post", "type": "multiclass_classification", "size": 3}]
    with pkg.NeuralNetwork(layers, None, 2, 4, seed=1) as net:
        assert net.layer("c").context() == (0, 0, 1)
    layers[3], layers[4] = {"name": "post", "type": "sse", "size": 4}, {"name": "post2", "type": "sse", "size": 4}
    with pytest.raises(pkg.CurrenntHipError) as ei:                                         # a post output layer behind a context layer
        pkg.NeuralNetwork(layers[:4], None, 2, 4, seed=1)
    assert ei.value.code == BAD_ARG and "trainable preceding layer" in str(ei.value)
