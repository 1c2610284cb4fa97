"""-m gpu: weight averaging (cn_ctx_average_weights, cn_ctx_swap_weight_average, cn_ctx_weight_average_state,
cn_layer_read_weight_average, cn_layer_upload_weight_average) against its numpy restatement (tests/average_reference.py), bit
for bit, behind every path that completes an update; beyond one pass of the launch grid; the swap around forward passes; that
a context which never averages is untouched; behind a skipped (clipped) step; and the protocol's errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gpu_adam as A
from adam_reference import test_gradients
from average_reference import average_step
from helpers import net_desc, random_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, MOM, HP = A.LR, 0.9, A.HP
DECAYS = (0.5, 0.9, 0.0, 0.999, np.float32(0.9999))          # the first call must copy whatever it says; 0 copies by rule


def update(net, family, step, per_layer=False):
    if family == "adam":
        net.update_weights_adam(LR, step=step, per_layer=per_layer, **HP)
    elif per_layer:
        net.update_weights(LR, MOM)
    else:
        net.update_weights_fused(LR, MOM)


def arm(net, family, step):
    if family == "adam":
        net.arm_adam(LR, step=step, **HP)
    else:
        net.arm_update(LR, MOM)


def averages(net):
    return {l.name: l.weight_average() for l in net.trainable_layers()}


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16", "PREC_BF16X3"])
@pytest.mark.parametrize("family", ["sgd", "adam"])
@pytest.mark.parametrize("path", ["all", "layer", "armed"])
def test_average_equals_restatement(pkg, prec, family, path):
    """Five steps, cn_ctx_average_weights behind each, with the decays 0.5 (first call: must copy), 0.9, 0 (copy), 0.999,
    float32(0.9999).  "all" / "layer": uploaded gradients, completed by *_update_all (the grouped launch) / *_update per layer (the
    flat kernel); "armed": real forward and backward passes on two alternating fractions, deterministic, the armed step completed
    by *_update_all.  After every step each layer's average EQUALS average_step(previous average, weights read after the update,
    decay)."""
    rng = np.random.RandomState(41)
    layers = A.second_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = A.two_fractions(pkg, rng)
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=getattr(pkg, prec), deterministic=True) as net:
        assert net.weight_average_state() == (False, False)
        start = {l.name: l.weights() for l in net.trainable_layers()}
        prev = None
        for step, decay in enumerate(DECAYS, 1):
            if path == "armed":
                net.load_sequences(fracs[(step - 1) % 2]); net.compute_forward_pass()
                arm(net, family, step)
                net.compute_backward_pass()
            else:
                for l in net.trainable_layers():
                    l.upload("weightUpdates", test_gradients(rng, l.weight_count))
            update(net, family, step, per_layer=(path == "layer"))
            net.average_weights(decay)
            assert net.weight_average_state() == (True, False)
            got = averages(net)
            for l in net.trainable_layers():
                w = l.weights()
                want = w if prev is None else average_step(prev[l.name], w, decay)
                assert np.array_equal(got[l.name], want), (step, l.name, float(np.abs(got[l.name] - want).max()), int((got[l.name] != want).sum()))
                if decay == 0.0:
                    assert np.array_equal(got[l.name], w)
            prev = got
        for l in net.trainable_layers():                          # the weights moved, and the average is not the weights
            assert not np.array_equal(l.weights(), start[l.name]) and not np.array_equal(prev[l.name], l.weights())


def elements_per_grid_pass():
    """What one pass of the full launch grid covers, from the constants beside the launcher (csrc/cn_average.hip)."""
    src = open(os.path.join(ROOT, "lstm-rnn_amd", "csrc", "cn_average.hip")).read()
    m = re.search(r"AVERAGE_THREADS = (\d+), AVERAGE_MAX_BLOCKS = (\d+);", src)
    assert m and "AVERAGE_PASS_ELEMS = (size_t)AVERAGE_MAX_BLOCKS * AVERAGE_THREADS * 4;" in src
    return int(m.group(1)) * int(m.group(2)) * 4


def test_average_and_swap_beyond_one_grid_pass(pkg):
    """16 -> blstm 1024 -> softmax 4 (about 2.17 M weights, PS 2, T 3, no pass is run): the arena exceeds what one pass of the
    capped grid covers at 16 bytes per lane, so the grid-stride loops take a second, partial round.  Every entry of the average
    equals the restatement; a swap exchanges every entry, a second one restores every bit."""
    rng = np.random.RandomState(42)
    layers = net_desc(16, [("blstm", 1024)], 4)
    with pkg.NeuralNetwork(layers, None, 2, 3, precision=pkg.PREC_BF16, seed=1) as net:
        count = net.param_arena()[3]
        assert count > elements_per_grid_pass() == 2048 * 256 * 4 and count % 4 == 0
        w1 = {l.name: rng.uniform(-0.5, 0.5, l.weight_count).astype(np.float32) for l in net.trainable_layers()}
        w2 = {l.name: rng.uniform(-0.5, 0.5, l.weight_count).astype(np.float32) for l in net.trainable_layers()}
        for l in net.trainable_layers():
            l.set_weights(w1[l.name])
        net.average_weights(0.3)                                  # the first step copies
        for l in net.trainable_layers():
            assert np.array_equal(l.weight_average(), w1[l.name])
            l.set_weights(w2[l.name])
        net.average_weights(0.9)
        avg = averages(net)
        for l in net.trainable_layers():
            want = average_step(w1[l.name], w2[l.name], 0.9)
            assert np.array_equal(avg[l.name], want), (l.name, int((avg[l.name] != want).sum()))
            assert np.array_equal(l.weights(), w2[l.name])
        net.swap_weight_average()
        assert net.weight_average_state() == (True, True)
        for l in net.trainable_layers():
            assert np.array_equal(l.weights(), avg[l.name]) and np.array_equal(l.weight_average(), w2[l.name])
        net.swap_weight_average()
        assert net.weight_average_state() == (True, False)
        for l in net.trainable_layers():
            assert np.array_equal(l.weights(), w2[l.name]) and np.array_equal(l.weight_average(), avg[l.name])


def full_state(net):
    return {l.name: (l.weights(), l.first_moments(), l.second_moments(), l.weight_average()) for l in net.trainable_layers()}


def train_step(net, fracs, step, noise, average=True):
    net.load_sequences(fracs[step % 2]); net.compute_forward_pass()
    if noise:
        net.set_weight_noise(0.01, seed=5, pass_=step)
    net.compute_backward_pass()
    net.update_weights_adam(LR, step=step, **HP)
    if average:
        net.average_weights(0.5)


@pytest.mark.parametrize("prec,noise", [("PREC_F32", False), ("PREC_BF16", False), ("PREC_BF16", True)])
def test_swap_and_forward(pkg, prec, noise):
    """Three real Adam steps with decay 0.5 (deterministic).  Swapped, a forward pass gives the posteriors of a fresh network
    built from the average, bit for bit; swapped back, those of before the swap; and one more training step leaves weights,
    moments and average bit-equal to a twin run that never swapped."""
    rng = np.random.RandomState(43)
    layers = A.second_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = A.two_fractions(pkg, rng)
    precision = getattr(pkg, prec)

    def make():
        return pkg.NeuralNetwork(layers, weights, 8, 17, precision=precision, deterministic=True)

    with make() as twin:
        for step in (1, 2, 3, 4):
            train_step(twin, fracs, step, noise)
        want = full_state(twin)
    with make() as net:
        for step in (1, 2, 3):
            train_step(net, fracs, step, noise)
        avg = averages(net)
        raw = {l.name: l.weights() for l in net.trainable_layers()}
        net.load_sequences(fracs[0]); net.compute_forward_pass()
        y_raw = net.outputs()
        net.swap_weight_average()
        net.compute_forward_pass()
        y_avg = net.outputs()
        for l in net.trainable_layers():
            assert np.array_equal(l.weights(), avg[l.name]) and np.array_equal(l.weight_average(), raw[l.name])
        with make() as fresh:
            for l in fresh.trainable_layers():
                l.set_weights(avg[l.name])
            fresh.load_sequences(fracs[0]); fresh.compute_forward_pass()
            assert np.array_equal(fresh.outputs(), y_avg)
        assert not np.array_equal(y_avg, y_raw)                   # (the average is another model)
        net.swap_weight_average()
        net.compute_forward_pass()
        assert np.array_equal(net.outputs(), y_raw)
        train_step(net, fracs, 4, noise)
        got = full_state(net)
    for name in want:
        for what, a, b in zip(("weights", "first moments", "second moments", "average"), got[name], want[name]):
            assert np.array_equal(a, b), (name, what, float(np.abs(a - b).max()))


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
def test_unused_means_untouched(pkg, prec):
    """Three steps with an averaging call behind each and three without end in bit-identical weights and moments; the run
    without calls never has an average."""
    rng = np.random.RandomState(44)
    layers = A.second_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = A.two_fractions(pkg, rng)
    res = {}
    for average in (True, False):
        with pkg.NeuralNetwork(layers, weights, 8, 17, precision=getattr(pkg, prec), deterministic=True) as net:
            for step in (1, 2, 3):
                train_step(net, fracs, step, False, average=average)
            assert net.weight_average_state() == (average, False)
            res[average] = A.state_of(net)
    assert A.same_state(res[True], res[False])


def test_average_behind_a_skipped_step(pkg):
    """Clipping on; the third step's gradient holds an inf, so the update is skipped: weights and moments stay, and the averaging
    step behind it still is the restatement, towards the unchanged weights."""
    rng = np.random.RandomState(45)
    layers = A.second_net()
    weights = random_weights(layers, rng, 0.2)
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=pkg.PREC_F32) as net:
        net.set_grad_clip(1e3)
        prev = None
        for step, decay in ((1, 0.5), (2, 0.9), (3, 0.9)):
            before = {l.name: l.weights() for l in net.trainable_layers()}
            for k, l in enumerate(net.trainable_layers()):
                g = test_gradients(rng, l.weight_count)
                if step == 3 and k == 1:
                    g[7] = np.inf
                l.upload("weightUpdates", g)
            net.update_weights_fused(LR, MOM)
            net.average_weights(decay)
            got = averages(net)
            for l in net.trainable_layers():
                w = l.weights()
                assert np.array_equal(w, before[l.name]) == (step == 3), (step, l.name)
                want = w if prev is None else average_step(prev[l.name], w, decay)
                assert np.array_equal(got[l.name], want), (step, l.name)
                if step == 3:
                    assert not np.array_equal(got[l.name], prev[l.name])      # it did move towards w
            prev = got
        stats = net.grad_clip_stats()
        assert stats["skipped"] == 1 and stats["updates"] == 3


def test_average_errors_and_state(pkg):
    rng = np.random.RandomState(46)
    layers = A.small_net()
    weights = random_weights(layers, rng, 0.3)
    xs, ts = A.random_sequences(rng, [6, 5, 4, 6], 5, C=3)
    frac = pkg.make_fraction(xs, ts, 4)
    E = pkg.CurrenntHipError

    def fresh():
        return pkg.NeuralNetwork(layers, weights, 4, 6, precision=pkg.PREC_F32)

    def refused(call, code, match=None):
        with pytest.raises(E, match=match) as e:
            call()
        assert e.value.code == code, str(e.value)

    with fresh() as net:
        lib = net.lib
        assert net.weight_average_state() == (False, False)
        for l in net.trainable_layers():                           # before an average exists: the weights
            assert np.array_equal(l.weight_average(), l.weights())
        assert net.weight_average_state() == (False, False)        # (a read creates nothing)
        refused(net.swap_weight_average, -4, "no average")         # CN_ERR_STATE
        for bad in (-0.1, 1.0, 1.5, float("nan")):
            refused(lambda: net.average_weights(bad), -1)          # CN_ERR_BAD_ARG
        assert net.weight_average_state() == (False, False)
        buf = np.zeros(1024, np.float32)
        p = buf.ctypes.data_as(C.c_void_p)
        lay = net.trainable_layers()[0]
        for h in (net.layers[0].handle, net.layers[-1].handle):    # layers without weights
            assert lib.cn_layer_read_weight_average(h, p, 4) == -1
            assert lib.cn_layer_upload_weight_average(h, p, 4) == -1
        assert lib.cn_layer_read_weight_average(lay.handle, p, lay.weight_count + 1) == -2       # CN_ERR_SHAPE
        assert lib.cn_layer_upload_weight_average(lay.handle, p, lay.weight_count - 1) == -2
        assert net.weight_average_state() == (False, False)
        # either pointer of the state call may be NULL
        one = C.c_int(7)
        assert lib.cn_ctx_weight_average_state(net.ctx, None, C.byref(one)) == 0 and one.value == 0
        assert lib.cn_ctx_weight_average_state(net.ctx, C.byref(one), None) == 0 and one.value == 0
        # an upload creates the average: a copy of all weights, this layer's part overwritten; the next step does not copy
        u = rng.uniform(-1, 1, lay.weight_count).astype(np.float32)
        lay.upload_weight_average(u)
        assert net.weight_average_state() == (True, False)
        for l in net.trainable_layers():
            assert np.array_equal(l.weight_average(), u if l is lay else l.weights())
        net.average_weights(0.9)
        for l in net.trainable_layers():
            assert np.array_equal(l.weight_average(), average_step(u if l is lay else l.weights(), l.weights(), 0.9))
        assert not np.array_equal(lay.weight_average(), lay.weights())

    with fresh() as net:
        net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
        net.update_weights_fused(LR, MOM)
        net.average_weights(0.5)
        net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
        net.update_weights_fused(LR, MOM)
        net.average_weights(0.5)
        # a swap while an armed update is pending: refused until the completing call
        net.load_sequences(frac); net.compute_forward_pass()
        net.arm_update(LR, MOM)
        refused(net.swap_weight_average, -4, "armed")
        net.compute_backward_pass()
        refused(net.swap_weight_average, -4, "armed")
        net.update_weights_fused(LR, MOM)
        net.average_weights(0.5)
        avg, raw = averages(net), {l.name: l.weights() for l in net.trainable_layers()}
        net.swap_weight_average()
        assert net.weight_average_state() == (True, True)
        lay = net.trainable_layers()[0]
        g = np.zeros(lay.weight_count, np.float32)
        for call in (net.compute_backward_pass, lambda: net.update_weights_fused(LR, MOM), lambda: net.update_weights(LR, MOM),
                     lambda: net.update_weights_adam(LR, step=1, **HP), lambda: net.update_weights_adam(LR, step=1, per_layer=True, **HP),
                     lambda: net.arm_update(LR, MOM), lambda: net.arm_adam(LR, step=1, **HP),
                     lambda: net.accumulate_updates(True), net.take_accumulated, net.allreduce_grads,
                     lambda: net.average_weights(0.5), lambda: lay.set_weights(g), lambda: lay.upload("weights", g),
                     lambda: lay.upload("weightUpdates", g), lambda: lay.upload("weightDeltas", g),
                     lambda: lay.upload_weight_average(g)):
            refused(call, -4, "swap")
        assert net.weight_average_state() == (True, True)
        # forward passes, loads, loss calls and reads stay allowed
        net.load_sequences(frac); net.compute_forward_pass()
        net.loss_accumulate()
        assert np.isfinite(net.calculate_error()) and np.isfinite(net.loss_read()[0])
        for l in net.trainable_layers():
            assert np.array_equal(l.weights(), avg[l.name]) and np.array_equal(l.weight_average(), raw[l.name])
        net.swap_weight_average()
        assert net.weight_average_state() == (True, False)
        for l in net.trainable_layers():
            assert np.array_equal(l.weights(), raw[l.name]) and np.array_equal(l.weight_average(), avg[l.name])
        # and training goes on
        net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
        net.update_weights_fused(LR, MOM)
        net.average_weights(0.5)
        # armed with clipping on: the step waits for the completing calls, and so does the swap, until the last layer's has come
        net.set_grad_clip(1e3)
        net.load_sequences(frac); net.compute_forward_pass()
        net.arm_update(LR, MOM)
        refused(net.swap_weight_average, -4, "armed")
        net.compute_backward_pass()
        first, second = net.trainable_layers()
        assert net.lib.cn_sgd_update(first.handle, LR, MOM) == 0
        refused(net.swap_weight_average, -4, "armed")
        assert net.lib.cn_sgd_update(second.handle, LR, MOM) == 0
        net.average_weights(0.5)
        net.swap_weight_average()
        assert net.weight_average_state() == (True, True)
        net.swap_weight_average()
        assert net.weight_average_state() == (True, False)
