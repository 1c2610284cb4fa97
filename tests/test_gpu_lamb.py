"""-m gpu: the LAMB update (cn_lamb_update, cn_lamb_update_all, cn_ctx_arm_lamb, cn_ctx_set_trust_bounds, cn_layer_trust_ratio)
against its numpy restatement (tests/lamb_reference.py), bit for bit: weights, both moments and every layer's record {ratio, weight
norm, update norm}; pad entries and counts that are no multiple of four, layers past one row of lanes and past the direction
kernel's unrolled pass, the bounds, clipping in front, the three ways to run a step, the operand copies, the protocol's errors,
an untouched Adam path, and two data-parallel ranks.  PS = 3, T <= 8, fp32 unless said, "deterministic" on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lamb_reference as LR_
from adam_reference import adam_step, test_gradients
from helpers import net_desc, random_sequences, random_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LR, DECAY = 2e-3, 0.01
PS, T = 3, 8

NETS = {"ff": (5, [("feedforward_tanh", 7)], 3),        # 42 and 24 weights: 42 is no multiple of four (two pad entries)
        "lstm": (3, [("lstm", 5)], 4),                  # 195 (one pad entry) and 24
        "blstm": (4, [("blstm", 6)], 3)}                # 210 (two pad entries) and 21 (three)


def layout(layers):
    """(segments [(start, stop, count)], decay mask, total) of the net's arena, from the network description"""
    kinds, prev = [], None
    for d in layers:
        if d["type"] in ("lstm", "blstm", "softmax") or d["type"].startswith("feedforward_"):
            kinds.append((d["type"], int(d["size"]), int(prev["size"])))
        prev = d
    return LR_.arena_layout(kinds)


def arena(net, segs, total, read):
    """a per-layer vector of every trainable layer in arena order, pad entries zero"""
    out = np.zeros(total, np.float32)
    for (a, _, n), l in zip(segs, net.trainable_layers()):
        out[a:a + n] = read(l)
    return out


def state_of(net, segs, total):
    return tuple(arena(net, segs, total, f) for f in (lambda l: l.weights(), lambda l: l.first_moments(), lambda l: l.second_moments()))


def records_of(net):
    return [l.trust_ratio() for l in net.trainable_layers()]


def rated(net, segs, lr=LR):
    return [(a, b, l.learning_rate if l.learning_rate >= 0.0 else lr) for (a, b, _), l in zip(segs, net.trainable_layers())]


def upload_gradients(net, rng):
    for l in net.trainable_layers():
        l.upload("weightUpdates", test_gradients(rng, l.weight_count))


def assert_step(net, segs, total, want, tag):
    got = state_of(net, segs, total)
    for what, a, b in zip(("weights", "first moments", "second moments"), got, want[:3]):
        assert np.array_equal(a, b), (tag, what, float(np.abs(a - b).max()), int((a != b).sum()))
    if want[3] is not None:
        for l, rec, ref in zip(net.trainable_layers(), records_of(net), want[3]):
            assert all(np.float32(x) == np.float32(y) for x, y in zip(rec, ref)), (tag, l.name, rec, ref)


def make(pkg, layers, weights, prec="PREC_F32"):
    return pkg.NeuralNetwork(layers, weights, PS, T, precision=getattr(pkg, prec), deterministic=True)


# ---- 1: five steps on three nets, decay on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(NETS))
def test_five_lamb_steps_equal_the_restatement(pkg, which):
    layers = net_desc(*NETS[which])
    rng = np.random.RandomState(51)
    weights = random_weights(layers, rng, 0.3)
    segs, mask, total = layout(layers)
    with make(pkg, layers, weights) as net:
        assert [n for _, _, n in segs] == [l.weight_count for l in net.trainable_layers()]
        assert any(n % 4 for _, _, n in segs)
        assert records_of(net) == [(1.0, 0.0, 0.0)] * len(segs)           # before the first LAMB step
        net.set_weight_decay(DECAY)
        for step in range(1, 6):
            before = state_of(net, segs, total)
            upload_gradients(net, rng)
            g = arena(net, segs, total, lambda l: l.weight_updates())
            net.update_weights_lamb(LR, step=step, **HP)
            want = LR_.lamb_step(before[0], g, before[1], before[2], rated(net, segs), mask, decay=DECAY, step=step, **HP)
            assert_step(net, segs, total, want, (which, step))
            # the bias and peephole entries show no decay term: w - step * r with the decay-free quotient r
            after = state_of(net, segs, total)
            for (a, b, _), rec in zip(segs, records_of(net)):
                _, _, r = LR_.lamb_direction(before[0][a:b], g[a:b], before[1][a:b], before[2][a:b], mask[a:b], 0.0, step=step, **HP)
                plain = before[0][a:b] - (np.float32(LR) * np.float32(rec[0])) * r
                free = ~mask[a:b]
                assert free.any() and np.array_equal(after[0][a:b][free], plain[free])
                assert not np.array_equal(after[0][a:b][~free], plain[~free])
        assert not after[0][~np.concatenate([np.arange(b - a) < n for a, b, n in segs])].any()      # pad entries stay zero


# ---- 2: past one row of lanes, past the unrolled pass -------------------------------------------------------------------------
@pytest.mark.parametrize("P,L", [(129, 131), (300, 440)])
def test_layers_past_a_row_of_lanes_and_past_the_unrolled_pass(pkg, P, L):
    """131 x 130 = 17 030 weights: more than the 16 384 lanes, so lanes add a second entry.  440 x 301 = 132 440 weights: the
    direction kernel loads 4 rows of 16 384 entries per pass (LAMB_UNROLL = 4), so this layer takes a third pass (and is past
    8 x 16 384 as well), with a last pass that is only partly inside the layer."""
    layers = net_desc(P, [("feedforward_tanh", L)], 3)
    rng = np.random.RandomState(52)
    weights = random_weights(layers, rng, 0.3)
    segs, mask, total = layout(layers)
    assert segs[0][2] == L * (P + 1) and segs[0][2] > (16384 if L == 131 else 8 * 16384)
    with make(pkg, layers, weights) as net:
        net.set_weight_decay(DECAY)
        before = state_of(net, segs, total)
        upload_gradients(net, rng)
        g = arena(net, segs, total, lambda l: l.weight_updates())
        net.update_weights_lamb(LR, step=1, **HP)
        want = LR_.lamb_step(before[0], g, before[1], before[2], rated(net, segs), mask, decay=DECAY, step=1, **HP)
        assert_step(net, segs, total, want, (P, L))


# ---- 3: the bounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["min", "max"])
def test_trust_bounds_bite(pkg, side):
    layers = net_desc(*NETS["lstm"])
    rng = np.random.RandomState(53)
    weights = random_weights(layers, rng, 0.3)
    segs, mask, total = layout(layers)
    with make(pkg, layers, weights) as net:
        before = state_of(net, segs, total)
        upload_gradients(net, rng)
        g = arena(net, segs, total, lambda l: l.weight_updates())
        natural = [float(r[0]) for r in LR_.lamb_step(before[0], g, before[1], before[2], rated(net, segs), mask, step=1, **HP)[3]]
        bounds = (2.0 * max(natural), 0.0) if side == "min" else (0.0, 0.5 * min(natural))
        net.set_trust_bounds(*bounds)
        assert net.trust_bounds() == tuple(np.float32(x) for x in bounds)
        net.update_weights_lamb(LR, step=1, **HP)
        want = LR_.lamb_step(before[0], g, before[1], before[2], rated(net, segs), mask, bounds=bounds, step=1, **HP)
        assert_step(net, segs, total, want, side)
        bound = np.float32(bounds[0] if side == "min" else bounds[1])
        for rec, nat in zip(records_of(net), natural):
            assert rec[0] == bound and rec[0] != np.float32(nat) and rec[1] > 0 and rec[2] > 0


# ---- 4: clipping in front -------------------------------------------------------------------------------------------------------
def test_clipping_scales_and_skips_in_front_of_lamb(pkg):
    layers = net_desc(*NETS["blstm"])
    rng = np.random.RandomState(54)
    weights = random_weights(layers, rng, 0.3)
    segs, mask, total = layout(layers)
    xs, ts = random_sequences(rng, [8, 6, 5], 4, C=3)
    frac = pkg.make_fraction(xs, ts, PS)
    with make(pkg, layers, weights) as net:
        net.set_weight_decay(DECAY)
        before = state_of(net, segs, total)
        upload_gradients(net, rng)
        g = arena(net, segs, total, lambda l: l.weight_updates())
        bound = 0.5 * float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        net.set_grad_clip(bound)
        net.update_weights_lamb(LR, step=1, **HP)
        st = net.grad_clip_stats()
        assert st["clipped"] == 1 and 0.4 < float(st["last_scale"]) < 0.6
        want = LR_.lamb_step(before[0], g, before[1], before[2], rated(net, segs), mask, decay=DECAY, max_norm=bound, step=1, **HP)
        assert_step(net, segs, total, want, "scaled")
        unclipped = LR_.lamb_step(before[0], g, before[1], before[2], rated(net, segs), mask, decay=DECAY, step=1, **HP)
        assert not np.array_equal(unclipped[1], want[1])
        # an inf in the gradient: the step is skipped, every buffer, every record and the forward outputs keep every bit
        net.load_sequences(frac); net.compute_forward_pass()
        y = net.outputs()
        before, recs = state_of(net, segs, total), records_of(net)
        for k, l in enumerate(net.trainable_layers()):
            gl = test_gradients(rng, l.weight_count)
            if k == 0:
                gl[11] = np.inf
            l.upload("weightUpdates", gl)
        g = arena(net, segs, total, lambda l: l.weight_updates())
        net.update_weights_lamb(LR, step=2, **HP)
        assert net.grad_clip_stats()["skipped"] == 1
        want = LR_.lamb_step(before[0], g, before[1], before[2], rated(net, segs), mask, decay=DECAY, max_norm=bound, step=2, **HP)
        assert want[3] is None
        assert_step(net, segs, total, want, "skipped")
        assert_step(net, segs, total, before + (None,), "skipped: unchanged")
        assert records_of(net) == recs
        net.compute_forward_pass()
        assert np.array_equal(net.outputs(), y)


# ---- 5: three ways to run a step ----------------------------------------------------------------------------------------------
def test_per_layer_all_and_armed_leave_the_same_bits(pkg):
    """gradients of one real backward pass per step, two steps; a layer with a rate of its own"""
    layers = net_desc(4, [("blstm", 6), ("feedforward_tanh", 7)], 3)
    layers[2]["learningRate"] = 5e-3
    rng = np.random.RandomState(55)
    weights = random_weights(layers, rng, 0.3)
    segs, mask, total = layout(layers)
    xs, ts = random_sequences(rng, [8, 6, 5], 4, C=3)
    frac = pkg.make_fraction(xs, ts, PS)
    final = {}
    for mode in ("all", "layer", "armed", "armed_layer"):
        with make(pkg, layers, weights) as net:
            net.set_weight_decay(DECAY)
            for step in (1, 2):
                before = state_of(net, segs, total)
                net.load_sequences(frac); net.compute_forward_pass()
                if mode.startswith("armed"):
                    net.arm_lamb(LR, step=step, **HP)
                net.compute_backward_pass()
                if mode.startswith("armed"):                    # deferred: nothing is applied before the completing call
                    assert all(np.array_equal(a, b) for a, b in zip(state_of(net, segs, total), before))
                net.update_weights_lamb(LR, step=step, per_layer=mode.endswith("layer"), **HP)
                g = arena(net, segs, total, lambda l: l.weight_updates())
                assert np.abs(g).max() > 0
                want = LR_.lamb_step(before[0], g, before[1], before[2], rated(net, segs), mask, decay=DECAY, step=step, **HP)
                assert abs(rated(net, segs)[1][2] - 5e-3) < 1e-9 and rated(net, segs)[0][2] == LR
                assert_step(net, segs, total, want, (mode, step))
            final[mode] = state_of(net, segs, total) + (records_of(net),)
    for mode in ("layer", "armed", "armed_layer"):
        assert all(np.array_equal(a, b) for a, b in zip(final[mode][:3], final["all"][:3])), mode
        assert final[mode][3] == final["all"][3], mode


# ---- 6: operand copies --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
def test_operand_copies_follow_the_lamb_weights(pkg, prec):
    layers = net_desc(4, [("blstm", 6), ("feedforward_tanh", 7)], 3)
    rng = np.random.RandomState(56)
    weights = random_weights(layers, rng, 0.3)
    xs, ts = random_sequences(rng, [8, 6, 5], 4, C=3)
    frac = pkg.make_fraction(xs, ts, PS)
    with make(pkg, layers, weights, prec) as net:
        for step in (1, 2):
            net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
            net.update_weights_lamb(LR, step=step, **HP)
        net.compute_forward_pass()
        y = net.outputs()
        trained = net.export_weights()
    assert all(np.abs(np.asarray(trained[n]["input"], np.float32) - weights[n]["input"]).max() > 1e-4 for n in weights)
    with make(pkg, layers, trained, prec) as fresh:
        fresh.load_sequences(frac); fresh.compute_forward_pass()
        assert np.array_equal(fresh.outputs(), y)


# ---- 7: errors ----------------------------------------------------------------------------------------------------------------
def test_lamb_state_and_argument_errors(pkg):
    layers = net_desc(*NETS["lstm"])
    rng = np.random.RandomState(57)
    weights = random_weights(layers, rng, 0.3)
    xs, ts = random_sequences(rng, [8, 6, 5], 3, C=4)
    frac = pkg.make_fraction(xs, ts, PS)
    E = pkg.CurrenntHipError

    def refused(call, code, match=None):
        with pytest.raises(E, match=match) as e:
            call()
        assert e.value.code == code, str(e.value)

    with make(pkg, layers, weights) as net:
        for bad in (dict(step=0), dict(step=-3), dict(beta1=1.0), dict(beta2=1.0), dict(beta1=-0.1), dict(eps=0.0)):
            for call in (net.update_weights_lamb, net.arm_lamb, lambda *a, **k: net.update_weights_lamb(*a, per_layer=True, **k)):
                refused(lambda: call(LR, **dict(dict(step=1), **bad)), -1)                   # CN_ERR_BAD_ARG
        for bad in ((-1.0, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("nan")), (float("inf"), 0.0), (0.0, float("inf")), (2.0, 1.0)):
            refused(lambda: net.set_trust_bounds(*bad), -1)
        assert net.trust_bounds() == (0.0, 0.0)
        net.set_trust_bounds(2.0, 0.0); net.set_trust_bounds(1.0, 1.0); net.set_trust_bounds(0.0, 0.0)      # (accepted)
        refused(net.layers[0].trust_ratio, -1, "no weights")                                  # the input layer
        # (a refused call binds nothing) LAMB first: the other two families are refused
        net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
        net.update_weights_lamb(LR, step=1, **HP)
        for call in (lambda: net.update_weights_adam(LR, step=2), lambda: net.arm_adam(LR, step=2), lambda: net.update_weights_adam(LR, step=2, per_layer=True),
                     lambda: net.update_weights_fused(1e-3, 0.9), lambda: net.update_weights(1e-3, 0.9), lambda: net.arm_update(1e-3, 0.9)):
            refused(call, -4, "LAMB")                                                       # CN_ERR_STATE
        # an armed step: other values, bounds changed while armed, then the right values
        net.load_sequences(frac); net.compute_forward_pass()
        net.arm_lamb(LR, step=2, **HP)
        refused(lambda: net.set_trust_bounds(0.5, 0.0), -4, "armed")
        refused(lambda: net.accumulate_updates(True), -4, "armed")
        net.compute_backward_pass()
        for other in (dict(step=3), dict(beta1=0.8), dict(beta2=0.99), dict(eps=1e-7)):
            refused(lambda: net.update_weights_lamb(LR, **dict(dict(HP, step=2), **other)), -4, "differ from what cn_ctx_arm_lamb armed")
        refused(lambda: net.update_weights_lamb(2 * LR, step=2, **HP), -4, "differ from what cn_ctx_arm_lamb armed")
        refused(lambda: net.update_weights_lamb(2 * LR, step=2, per_layer=True, **HP), -4, "differ from what cn_ctx_arm_lamb armed")
        net.update_weights_lamb(LR, step=2, **HP)
        net.set_trust_bounds(0.5, 0.0)
        # while the weights are swapped with their average: no update of any kind
        net.average_weights(0.9)
        net.swap_weight_average()
        for call in (lambda: net.update_weights_lamb(LR, step=3, **HP), lambda: net.update_weights_lamb(LR, step=3, per_layer=True, **HP),
                     lambda: net.arm_lamb(LR, step=3, **HP)):
            refused(call, -4, "swapped")
        net.swap_weight_average()
        net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
        net.update_weights_lamb(LR, step=3, **HP)
    for first in ("adam", "sgd"):                       # and the reverse: LAMB after Adam or steepest descent
        with make(pkg, layers, weights) as net:
            net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
            if first == "adam":
                net.update_weights_adam(LR, step=1, **HP)
            else:
                net.update_weights_fused(1e-3, 0.9)
            for call in (lambda: net.update_weights_lamb(LR, step=2, **HP), lambda: net.arm_lamb(LR, step=2, **HP),
                         lambda: net.update_weights_lamb(LR, step=2, per_layer=True, **HP)):
                refused(call, -4, "LAMB")


# ---- 8: a context that never calls LAMB ---------------------------------------------------------------------------------------
def test_a_context_without_lamb_keeps_its_adam_step(pkg):
    layers = net_desc(*NETS["blstm"])
    rng = np.random.RandomState(58)
    weights = random_weights(layers, rng, 0.3)
    with make(pkg, layers, weights) as net:
        assert net.trust_bounds() == (0.0, 0.0)
        ref = {l.name: (l.weights(), np.zeros(l.weight_count, np.float32), np.zeros(l.weight_count, np.float32)) for l in net.trainable_layers()}
        for step in (1, 2, 3):
            for l in net.trainable_layers():
                g = test_gradients(rng, l.weight_count)
                l.upload("weightUpdates", g)
                ref[l.name] = adam_step(ref[l.name][0], g, ref[l.name][1], ref[l.name][2], LR, step=step, **HP)
            net.update_weights_adam(LR, step=step, per_layer=(step == 2), **HP)
            for l in net.trainable_layers():
                for a, b in zip((l.weights(), l.first_moments(), l.second_moments()), ref[l.name]):
                    assert np.array_equal(a, b), (step, l.name)
        assert records_of(net) == [(1.0, 0.0, 0.0)] * 2 and net.trust_bounds() == (0.0, 0.0)


# ---- two data-parallel ranks --------------------------------------------------------------------------------------------------
def test_lamb_data_parallel_replicas_stay_identical(pkg, tmp_path):
    """Two ranks on one device through the library's test backend (tests/lamb_rank.py): different sequences per rank, each layer's
    gradient exchanged behind its backward pass, the LAMB step behind the exchange.  After 3 steps the replicas hold bit-identical
    weights, moments and records, and every step is the restatement's on the summed gradient."""
    world = 2
    env = dict(os.environ, CN_COMM_BACKEND="ipc", HSA_ENABLE_IPC_MODE_LEGACY="0", CN_COMM_IPC_TIMEOUT="60")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "lamb_rank.py"), str(r), str(world), str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, (r, outs[r][-3000:])
    res = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    assert str(res[0]["backend"]) == "ipc"
    for key in ("w", "m", "v", "g", "rec"):
        assert np.array_equal(res[0][key], res[1][key]), key
    import lamb_rank
    layers = lamb_rank.network()
    segs, mask, total = layout(layers)
    rates = [(a, b, lamb_rank.OWN_LR if k == 1 else lamb_rank.LR) for k, (a, b, _) in enumerate(segs)]
    w, m, v = res[0]["w0"], np.zeros(total, np.float32), np.zeros(total, np.float32)
    for step in (1, 2, 3):
        w, m, v, recs = LR_.lamb_step(w, res[0]["g"][step - 1], m, v, rates, mask, decay=lamb_rank.DECAY, step=step)
    for key, want in (("w", w), ("m", m), ("v", v), ("rec", np.asarray(recs, np.float32))):
        assert np.array_equal(res[0][key], want), key
    assert np.abs(w - res[0]["w0"]).max() > 1e-3
