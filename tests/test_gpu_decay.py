"""-m gpu: decoupled weight decay (cn_ctx_set_weight_decay) against its numpy restatement (tests/decay_reference.py), bit for bit:
every update path under both optimizers, the exempt blocks, clipping, the operand copies, the flat kernels beyond their first
grid pass, batch learning, the protocol's errors and two data-parallel ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_reference as CR
import decay_reference as DR
from adam_reference import test_gradients
from helpers import net_desc, random_sequences, random_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LR, OWN_LR, MOM, WD = 1e-2, 3e-2, 0.9, 0.1
PS, T = 2, 3
PRECS = ["PREC_F32", "PREC_BF16", "PREC_BF16X3"]


def three_layer_net():
    """39 -> lstm 8 -> blstm 12 (own learningRate) -> softmax 5: 1560 | 756 | 65 weights, the last layer padded to 68"""
    layers = net_desc(39, [("lstm", 8), ("blstm", 12)], 5)
    layers[2]["learningRate"] = OWN_LR
    return layers


def ff_net():
    """... with a feedforward_tanh 6 layer in front of the softmax layer: 1560 | 756 | 78 (padded to 80) | 35 (padded to 36)"""
    layers = net_desc(39, [("lstm", 8), ("blstm", 12), ("feedforward_tanh", 6)], 5)
    layers[2]["learningRate"] = OWN_LR
    return layers


NETS = {"three": three_layer_net, "ff": ff_net}


def fractions(pkg, rng, n=1):
    out = []
    for k in range(n):
        xs, ts = random_sequences(rng, [T, T - 1], 39, C=5)
        out.append(pkg.make_fraction(xs, ts, PS))
    return out


def segments(net, lr):
    """(start, stop, rate, layer) of every trainable layer in the arena (each rounded up to four entries), the arena's size and
    the mask of its entries that decay"""
    out, off = [], 0
    sizes = {l.name: l.size for l in net.layers}
    prev = {b.name: a for a, b in zip(net.layers[:-1], net.layers[1:])}
    ranges = []
    for l in net.trainable_layers():
        out.append((off, off + l.weight_count, np.float32(l.learning_rate if l.learning_rate >= 0.0 else lr), l))
        P = sizes[prev[l.name].name]
        assert DR.weight_count(l.type, l.size, P) == l.weight_count
        ranges += [(off + a, off + b) for a, b in DR.decayed_ranges(l.type, l.size, P)]
        off += (l.weight_count + 3) // 4 * 4
    assert off == net.param_arena()[3]
    return out, off, DR.decay_mask(off, ranges)


def arena(segs, total, read):
    a = np.zeros(total, np.float32)
    for s, e, _, l in segs:
        a[s:e] = read(l)
    return a


def state_of(segs, total):
    return tuple(arena(segs, total, f) for f in (lambda l: l.weights(), lambda l: l.first_moments(), lambda l: l.second_moments()))


def reference_step(rule, state, g, segs, mask, decay, step, bound=None, mom=MOM):
    """the step over the arena; returns (w, d | m, v, scale, skip)"""
    w, d, v = state
    if rule == "adam":
        sg = [(s, e, lr) for s, e, lr, _ in segs]
        if bound is None:
            return DR.decay_adam_step(w, g, d, v, sg, decay, mask, step=step, **HP) + (None, False)
        r = DR.clip_decay_adam_step(w, g, d, v, sg, decay, mask, bound, step=step, **HP)
        return r[:3] + r[4:]
    rates = np.zeros(w.size, np.float32)
    for s, e, lr, _ in segs:
        rates[s:e] = lr
    if bound is None:
        w2, d2 = DR.decay_sgd_step(w, g, d, rates, mom, decay, mask)
        return w2, d2, v, None, False
    w2, d2, _, scale, skip = DR.clip_decay_sgd_step(w, g, d, rates, mom, decay, mask, bound)
    return w2, d2, v, scale, skip


def update(net, rule, how, step, mom=MOM):
    if rule == "adam":
        net.update_weights_adam(LR, step=step, per_layer=(how == "layer"), **HP)
    elif how == "layer":
        net.update_weights(LR, mom)
    else:
        net.update_weights_fused(LR, mom)


def arm(net, rule, step, mom=MOM):
    if rule == "adam":
        net.arm_adam(LR, step=step, **HP)
    else:
        net.arm_update(LR, mom)


def assert_state(got, want, rule, where):
    for what, a, b in zip(("weights", "deltas / first moments", "second moments"), got, want[:3]):
        if what == "second moments" and rule != "adam":
            continue
        assert np.array_equal(a, b), (where, what, float(np.abs(a - b).max()), int((a != b).sum()))


# ---- 1. every path ---------------------------------------------------------------------------------------------------------------
# path: (how the completing call is made, armed, deterministic, clipping bound)
PATHS = {"layer": ("layer", False, True, None), "all": ("all", False, True, None), "armed": ("all", True, False, None),
         "armed deterministic": ("all", True, True, None), "armed clipped": ("all", True, True, 0.05)}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", list(NETS))
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_every_update_path_equals_the_restatement(pkg, rule, path, which, prec):
    """Three consecutive updates from real backward passes (PS 2, T 3), so that deltas and moments carry; after each one
    weightUpdates is read back and the step replayed: weights, deltas / first moments, second moments."""
    how, armed, det, bound = PATHS[path]
    rng = np.random.RandomState(51)
    layers = NETS[which]()
    weights = random_weights(layers, rng, 0.2)
    fracs = fractions(pkg, rng, 2)
    with pkg.NeuralNetwork(layers, weights, PS, T, precision=getattr(pkg, prec), deterministic=det) as net:
        segs, total, mask = segments(net, LR)
        assert which != "three" or total == 1560 + 756 + 68
        net.set_weight_decay(WD)
        if bound is not None:
            net.set_grad_clip(bound)
        scales = []
        for step in (1, 2, 3):
            before = state_of(segs, total)
            net.load_sequences(fracs[step % 2]); net.compute_forward_pass()
            if armed:
                arm(net, rule, step)
            net.compute_backward_pass()
            update(net, rule, how, step)
            g = arena(segs, total, lambda l: l.weight_updates())
            assert g.any()
            want = reference_step(rule, before, g, segs, mask, WD, step, None if bound is None else np.float32(bound))
            assert not want[4]
            scales.append(want[3])
            assert_state(state_of(segs, total), want, rule, (rule, path, which, prec, step))
            plain = reference_step(rule, before, g, segs, mask, 0.0, step, None if bound is None else np.float32(bound))
            assert not np.array_equal(plain[0][mask], want[0][mask])              # (the decay is visible in the bits compared)
        if bound is not None:
            assert any(s is not None for s in scales)                             # (the bound clips)


# ---- 2. the exempt blocks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["all", "layer"])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_bias_peephole_and_pad_entries_never_decay(pkg, rule, how):
    """A zero gradient uploaded, momentum 0, decay 0.5: the step is the decay alone.  lstm, blstm, feedforward and softmax layers:
    bias and peephole entries keep their bits, every other entry is w - ld * w exactly; the arena's pad entries stay zero."""
    rng = np.random.RandomState(52)
    layers = ff_net()
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.2), PS, T, precision=pkg.PREC_F32) as net:
        segs, total, mask = segments(net, LR)
        assert [l.type for _, _, _, l in segs] == ["lstm", "blstm", "feedforward_tanh", "softmax"]
        net.set_weight_decay(0.5)
        for _, _, _, l in segs:
            l.upload("weightUpdates", np.zeros(l.weight_count, np.float32))
        w = arena(segs, total, lambda l: l.weights())
        update(net, rule, how, 1, mom=0.0)
        w1 = arena(segs, total, lambda l: l.weights())
        for s, e, lr, l in segs:
            m = mask[s:e]
            ld = np.float32(float(lr) * 0.5)
            assert (~m).sum() == {"lstm": 4 * 8 + 3 * 8, "blstm": 4 * 12 + 3 * 12, "feedforward_tanh": 6, "softmax": 5}[l.type]
            assert w1[s:e][~m].tobytes() == w[s:e][~m].tobytes(), l.type
            assert w1[s:e][m].tobytes() == (w[s:e][m] - ld * w[s:e][m]).astype(np.float32).tobytes(), l.type
            assert np.all(w1[s:e][m] != w[s:e][m])
        import torch
        wptr, _, _, count = net.param_arena()
        assert count == total
        net.join(); net.synchronize()
        raw = torch.as_tensor(pkg.parallel.DeviceArray(wptr, count), device="cuda").cpu().numpy()
        pads = np.ones(total, bool)
        for s, e, _, _ in segs:
            pads[s:e] = False
        assert pads.sum() == 2 + 1 and raw[pads].tobytes() == np.zeros(3, np.float32).tobytes()
        assert raw[~pads].tobytes() == w1[~pads].tobytes()


# ---- 3. clipping ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["all", "layer"])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_clipping_scales_the_gradient_only_and_a_skipped_step_decays_nothing(pkg, rule, how):
    rng = np.random.RandomState(53)
    layers = three_layer_net()
    frac = fractions(pkg, rng)[0]
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.2), PS, T, precision=pkg.PREC_F32) as net:
        segs, total, mask = segments(net, LR)
        net.set_weight_decay(WD)
        net.set_grad_clip(0.05)
        net.load_sequences(frac)
        before = state_of(segs, total)
        for _, _, _, l in segs:
            l.upload("weightUpdates", test_gradients(rng, l.weight_count))
        g = arena(segs, total, lambda l: l.weight_updates())
        update(net, rule, how, 1)
        want = reference_step(rule, before, g, segs, mask, WD, 1, np.float32(0.05))
        assert want[3] is not None and want[3] < 1 and not want[4]                # clipped
        assert net.grad_clip_stats()["last_scale"].tobytes() == want[3].tobytes()
        got = state_of(segs, total)
        assert_state(got, want, rule, (rule, how, "clipped"))
        if rule == "sgd":                                                         # spelled out: the factor is on g, not on ld * w
            rates = np.zeros(total, np.float32)
            for s, e, lr, _ in segs:
                rates[s:e] = lr
            w0 = DR.decay_weights(before[0], mask, rates, WD)
            assert got[0].tobytes() == (w0 + (np.float32(MOM) * before[1] - rates * (want[3] * g))).astype(np.float32).tobytes()
        net.compute_forward_pass()
        y1 = net.outputs()
        before = got
        for k, (_, _, _, l) in enumerate(segs):                                   # an inf in the gradient: the step is skipped
            gk = test_gradients(rng, l.weight_count)
            if k == 1:
                gk[7] = np.inf
            l.upload("weightUpdates", gk)
        update(net, rule, how, 2)
        assert net.grad_clip_stats()["skipped"] == 1
        assert_state(state_of(segs, total), before, "adam", (rule, how, "skipped"))
        net.compute_forward_pass()
        assert np.array_equal(net.outputs(), y1)                                  # ... the operand copies included


# ---- 4. operand copies ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
@pytest.mark.parametrize("armed", [False, True])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_operand_copies_hold_the_decayed_weights(pkg, rule, armed, prec):
    """after fused / armed steps with decay a fresh network built from the weights read back computes bit-identical posteriors"""
    rng = np.random.RandomState(54)
    layers = ff_net()
    weights = random_weights(layers, rng, 0.2)
    frac = fractions(pkg, rng)[0]
    with pkg.NeuralNetwork(layers, weights, PS, T, precision=getattr(pkg, prec), deterministic=True) as net:
        net.set_weight_decay(0.5)
        for step in (1, 2):
            net.load_sequences(frac); net.compute_forward_pass()
            if armed:
                arm(net, rule, step)
            net.compute_backward_pass()
            update(net, rule, "all", step)
        net.compute_forward_pass()
        y = net.outputs()
        trained = net.export_weights()
    assert all(not np.array_equal(np.asarray(trained[n]["input"], np.float32), weights[n]["input"]) for n in weights)
    with pkg.NeuralNetwork(layers, trained, PS, T, precision=getattr(pkg, prec), deterministic=True) as fresh:
        fresh.load_sequences(frac); fresh.compute_forward_pass()
        assert np.array_equal(fresh.outputs(), y)


# ---- 5. the flat kernels beyond their first grid pass ---------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_flat_kernels_beyond_their_first_grid_pass(pkg, rule):
    """one softmax layer 700 -> 750: 525 750 weights, more than the 2048 x 256 threads a launch is capped at; the 750 bias
    weights, exempt, lie in the second pass.  Per-layer call, two steps."""
    rng = np.random.RandomState(55)
    layers = net_desc(700, [], 750)
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.1), PS, T, precision=pkg.PREC_F32) as net:
        segs, total, mask = segments(net, LR)
        assert total == 525752 and total > 2048 * 256 and mask.sum() == 525000 and not mask[525000:].any()
        net.set_weight_decay(WD)
        for step in (1, 2):
            before = state_of(segs, total)
            g = test_gradients(rng, 525750)
            segs[0][3].upload("weightUpdates", g)
            update(net, rule, "layer", step)
            want = reference_step(rule, before, np.pad(g, (0, 2)), segs, mask, WD, step)
            assert_state(state_of(segs, total), want, rule, (rule, step))
            assert want[0][525000:525750].tobytes() == reference_step(rule, before, np.pad(g, (0, 2)), segs, mask, 0.0, step)[0][525000:525750].tobytes()


# ---- 6. batch learning --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_batch_learning_decays_once_per_update(pkg, rule):
    rng = np.random.RandomState(56)
    layers = three_layer_net()
    fracs = fractions(pkg, rng, 2)
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.2), PS, T, precision=pkg.PREC_F32) as net:
        segs, total, mask = segments(net, LR)
        net.set_weight_decay(WD)
        before = state_of(segs, total)
        single = []
        for k, f in enumerate(fracs):
            net.load_sequences(f); net.compute_forward_pass(); net.compute_backward_pass()
            single.append(arena(segs, total, lambda l: l.weight_updates()))
            net.accumulate_updates(k == 0)
            assert np.array_equal(arena(segs, total, lambda l: l.weights()), before[0])         # (a fraction decays nothing)
        net.take_accumulated()
        g = arena(segs, total, lambda l: l.weight_updates())
        assert np.array_equal(g, single[0] + single[1])
        update(net, rule, "all", 1)
        assert_state(state_of(segs, total), reference_step(rule, before, g, segs, mask, WD, 1), rule, rule)


# ---- 7. arguments and state -----------------------------------------------------------------------------------------------------
def test_weight_decay_arguments_and_state(pkg):
    rng = np.random.RandomState(57)
    layers = three_layer_net()
    weights = random_weights(layers, rng, 0.2)
    frac = fractions(pkg, rng)[0]
    E = pkg.CurrenntHipError
    with pkg.NeuralNetwork(layers, weights, PS, T, precision=pkg.PREC_F32) as net:
        segs, total, mask = segments(net, LR)
        assert float(net.weight_decay()) == 0.0                   # a fresh context is off
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(E) as e:
                net.set_weight_decay(bad)
            assert e.value.code == -1                             # CN_ERR_BAD_ARG
        assert float(net.weight_decay()) == 0.0
        net.set_weight_decay(0.3)
        assert net.weight_decay().tobytes() == np.float32(0.3).tobytes()         # the getter round-trips
        net.load_sequences(frac); net.compute_forward_pass()
        net.arm_update(LR, MOM)                                   # armed: the coefficient may not change under it
        with pytest.raises(E, match="armed") as e:
            net.set_weight_decay(0.1)
        assert e.value.code == -4                                 # CN_ERR_STATE
        before = state_of(segs, total)
        net.compute_backward_pass()
        with pytest.raises(E, match="armed") as e:
            net.set_weight_decay(0.0)
        assert e.value.code == -4
        net.update_weights_fused(LR, MOM)
        g = arena(segs, total, lambda l: l.weight_updates())
        assert_state(state_of(segs, total), reference_step("sgd", before, g, segs, mask, np.float32(0.3), 1), "sgd", "armed at 0.3")
        net.set_grad_clip(1e30)
        net.compute_forward_pass()
        net.arm_update(LR, MOM)                                   # armed with clipping on (deferred): pending just the same
        with pytest.raises(E, match="armed") as e:
            net.set_weight_decay(0.1)
        assert e.value.code == -4
        net.compute_backward_pass()
        net.update_weights_fused(LR, MOM)
        net.set_grad_clip(0.0)
        net.set_weight_decay(0.0)                                 # between steps: accepted; 0 after a non-zero decay is the plain step
        assert float(net.weight_decay()) == 0.0
        before = state_of(segs, total)
        net.compute_forward_pass(); net.compute_backward_pass()
        net.update_weights_fused(LR, MOM)
        g = arena(segs, total, lambda l: l.weight_updates())
        rates = np.zeros(total, np.float32)
        for s, e_, lr, _ in segs:
            rates[s:e_] = lr
        w, d = CR.sgd_step(before[0], g, before[1], rates, MOM)
        got = state_of(segs, total)
        assert got[0].tobytes() == w.tobytes() and got[1].tobytes() == d.tobytes()
        net.average_weights(0.5); net.swap_weight_average()       # while swapped: it only stores a number
        net.set_weight_decay(0.2)
        assert net.weight_decay().tobytes() == np.float32(0.2).tobytes()
        net.swap_weight_average()


# ---- 8. data-parallel -------------------------------------------------------------------------------------------------------------
def test_decay_data_parallel_replicas_stay_identical(pkg, tmp_path):
    """Two ranks on one device through the library's test backend (tests/decay_rank.py): different sequences per rank, three
    armed Adam steps with decay.  Both ranks hold bit-identical weights and moments, and they are the restatement's."""
    world = 2
    env = dict(os.environ, CN_COMM_BACKEND="ipc", HSA_ENABLE_IPC_MODE_LEGACY="0", CN_COMM_IPC_TIMEOUT="60")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "decay_rank.py"), str(r), str(world), str(tmp_path)],
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
    for key in ("w", "m", "v", "g"):
        assert res[0][key].tobytes() == res[1][key].tobytes(), key
    w, m, v = res[0]["w0"], np.zeros_like(res[0]["w0"]), np.zeros_like(res[0]["w0"])
    segs = [tuple(s) for s in res[0]["segments"]]
    mask = res[0]["mask"]
    for step in range(3):
        w, m, v = DR.decay_adam_step(w, res[0]["g"][step], m, v, [(int(a), int(b), np.float32(lr)) for a, b, lr in segs],
                                     float(res[0]["decay"]), mask, step=step + 1)
    assert w.tobytes() == res[0]["w"].tobytes() and m.tobytes() == res[0]["m"].tobytes() and v.tobytes() == res[0]["v"].tobytes()
    plain = DR.decay_adam_step(res[0]["w0"], res[0]["g"][0], np.zeros_like(w), np.zeros_like(w),
                               [(int(a), int(b), np.float32(lr)) for a, b, lr in segs], 0.0, mask, step=1)[0]
    assert not np.array_equal(plain, res[0]["w"])
