"""-m gpu: gradient clipping by the global L2 norm (cn_ctx_set_grad_clip, cn_ctx_grad_clip_stats) against its numpy restatement
(tests/clip_reference.py), bit for bit: the norm at the edges of the reduction, clipped and unclipped steps on every update
path, skipped steps, values whose squares overflow fp32, the operand copies, batch learning, the protocol's errors and two
data-parallel ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_reference as CR
from adam_reference import test_gradients
from helpers import net_desc, random_sequences, random_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LR, OWN_LR, MOM = 1e-2, 3e-2, 0.9
FLT_MAX = float(np.finfo(np.float32).max)
L = CR.L
PRECS = ["PREC_F32", "PREC_BF16", "PREC_BF16X3"]


def three_layer_net():
    """39 -> lstm 8 -> blstm 12 (own learningRate) -> softmax 5: an arena of three layers (1560 | 756 | 65 weights, the last one
    padded to 68)"""
    layers = net_desc(39, [("lstm", 8), ("blstm", 12)], 5)
    layers[2]["learningRate"] = OWN_LR
    return layers


def softmax_net(P, C):
    return net_desc(P, [], C)


def segments(net, lr):
    """(start, stop, rate, layer) of every trainable layer in the arena: creation order, each rounded up to four entries"""
    out, off = [], 0
    for l in net.trainable_layers():
        out.append((off, off + l.weight_count, np.float32(l.learning_rate if l.learning_rate >= 0.0 else lr), l))
        off += (l.weight_count + 3) // 4 * 4
    assert off == net.param_arena()[3]
    return out, off


def arena(net, segs, total, read):
    a = np.zeros(total, np.float32)
    for s, e, _, l in segs:
        a[s:e] = read(l)
    return a


def state_of(net, segs, total):
    return tuple(arena(net, segs, total, f) for f in (lambda l: l.weights(), lambda l: l.first_moments(), lambda l: l.second_moments()))


def reference_step(rule, state, g, segs, bound, step):
    """the clipped step over the arena; returns (w, d | m, v, norm, scale, skip)"""
    w, d, v = state
    if rule == "adam":
        return CR.clip_adam_step(w, g, d, v, [(s, e, lr) for s, e, lr, _ in segs], bound, step=step, **HP)
    rates = np.zeros(w.size, np.float32)
    for s, e, lr, _ in segs:
        rates[s:e] = lr
    w2, d2, norm, scale, skip = CR.clip_sgd_step(w, g, d, rates, MOM, bound)
    return w2, d2, v, norm, scale, skip


def update(net, rule, how, step):
    if rule == "adam":
        net.update_weights_adam(LR, step=step, per_layer=(how == "layer"), **HP)
    elif how == "layer":
        net.update_weights(LR, MOM)
    else:
        net.update_weights_fused(LR, MOM)


def arm(net, rule, step):
    if rule == "adam":
        net.arm_adam(LR, step=step, **HP)
    else:
        net.arm_update(LR, MOM)


def assert_state(got, want, rule, where):
    for what, a, b in zip(("weights", "deltas / first moments", "second moments"), got, want[:3]):
        if what == "second moments" and rule != "adam":
            continue
        assert np.array_equal(a, b), (where, what, float(np.abs(a - b).max()), int((a != b).sum()))


# ---- the norm at the edges of the reduction ----------------------------------------------------------------------------------
EDGE_NETS = {"8": softmax_net(1, 4), "L": softmax_net(127, 128), "L+128": softmax_net(128, 128), "4L+513": softmax_net(256, 257),
             "three layers": three_layer_net()}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", list(EDGE_NETS))
def test_norm_and_factor_equal_the_restatement(pkg, prec, which):
    """Gradients uploaded through cn_layer_upload (1e-6 ... 1, exact zeros); weight counts 8, L, L + 128, 4 L + 513 and a three-
    layer arena.  last_norm and last_scale are the restatement's floats, with a bound below the norm and with one above it."""
    layers = EDGE_NETS[which]
    rng = np.random.RandomState(31)
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.1), 2, 3, precision=getattr(pkg, prec)) as net:
        segs, total = segments(net, LR)
        assert total == {"8": 8, "L": L, "L+128": L + 128, "4L+513": 4 * L + 516, "three layers": 1560 + 756 + 68}[which]
        for k, share in enumerate((0.37, 4.0)):
            for _, _, _, l in segs:
                l.upload("weightUpdates", test_gradients(rng, l.weight_count))
            g = arena(net, segs, total, lambda l: l.weight_updates())
            bound = np.float32(share) * CR.clip_factor(g, 0.0)[0]
            norm, scale, skip = CR.clip_factor(g, bound)
            assert not skip and (scale is None) == (share > 1)
            net.set_grad_clip(bound)
            net.update_weights_fused(LR, MOM)
            st = net.grad_clip_stats()
            assert st["last_norm"].tobytes() == norm.tobytes(), (which, st["last_norm"], norm)
            assert st["last_scale"].tobytes() == np.float32(1.0 if scale is None else scale).tobytes(), (which, st["last_scale"], scale)
            assert (st["updates"], st["clipped"], st["skipped"]) == (k + 1, 1, 0)
            assert np.array_equal(arena(net, segs, total, lambda l: l.weight_updates()), g)       # never rewritten


# ---- steps -------------------------------------------------------------------------------------------------------------------
def two_fractions(pkg, rng, PS=8, T=17):
    """the second fraction is much shorter: its gradient (a sum over the frames) is smaller, so a bound between the two norms
    clips every other step"""
    out = []
    for k, lens in enumerate(([T - (i % 5) for i in range(PS)], [3, 2, 3])):
        xs, ts = random_sequences(rng, lens, 39, C=5)
        out.append(pkg.make_fraction(xs, ts, PS))
    return out


@pytest.mark.parametrize("prec,det", [("PREC_F32", True), ("PREC_BF16", True), ("PREC_BF16", False), ("PREC_BF16X3", True)])
@pytest.mark.parametrize("armed", [False, True])
@pytest.mark.parametrize("how", ["all", "layer"])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_clipped_steps_equal_the_restatement(pkg, rule, how, armed, prec, det):
    """Five updates of the three-layer net from real backward passes (PS 8, T 17; the blstm layer has a rate of its own).  The
    bound is half the first step's norm, which clips the long fractions and not the short ones.  After each update weightUpdates
    is read back -- the unclipped gradient -- and the step replayed: weights, deltas / first moments, second moments."""
    rng = np.random.RandomState(32)
    layers = three_layer_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = two_fractions(pkg, rng)
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=getattr(pkg, prec), deterministic=det) as net:
        segs, total = segments(net, LR)
        net.set_grad_clip(FLT_MAX)               # (a monitor, until the first gradient is known)
        bound = None
        for step in range(1, 6):
            before = state_of(net, segs, total)
            net.load_sequences(fracs[(step - 1) % 2]); net.compute_forward_pass()
            if bound is None:
                net.compute_backward_pass()
                bound = np.float32(0.5) * CR.clip_factor(arena(net, segs, total, lambda l: l.weight_updates()), 0.0)[0]
                net.set_grad_clip(bound)
                net.compute_forward_pass()
            if armed:
                arm(net, rule, step)
            net.compute_backward_pass()
            update(net, rule, how, step)
            g = arena(net, segs, total, lambda l: l.weight_updates())
            want = reference_step(rule, before, g, segs, bound, step)
            assert not want[5]
            st = net.grad_clip_stats()
            assert st["last_norm"].tobytes() == want[3].tobytes(), (step, st["last_norm"], want[3])
            assert st["last_scale"].tobytes() == np.float32(1.0 if want[4] is None else want[4]).tobytes()
            assert_state(state_of(net, segs, total), want, rule, (rule, how, armed, prec, step))
        st = net.grad_clip_stats(reset=True)
        assert st["updates"] == 5 and st["skipped"] == 0 and 0 < st["clipped"] < 5, st       # some steps clip, some do not
        assert st["max_norm_seen"] >= st["last_norm"] > 0
        st = net.grad_clip_stats()
        assert (st["updates"], st["clipped"], st["skipped"], float(st["max_norm_seen"])) == (0, 0, 0, 0.0)


def run_plain(pkg, layers, weights, fracs, prec, rule, armed, clip):
    """three steps; clip: None (never called), or the bound given to cn_ctx_set_grad_clip"""
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=prec, deterministic=True) as net:
        segs, total = segments(net, LR)
        if clip is not None:
            net.set_grad_clip(clip)
        for step in (1, 2, 3):
            net.load_sequences(fracs[step % 2]); net.compute_forward_pass()
            if armed:
                arm(net, rule, step)
            net.compute_backward_pass()
            update(net, rule, "all", step)
        st = net.grad_clip_stats()
        return state_of(net, segs, total), st


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
@pytest.mark.parametrize("armed", [False, True])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_off_means_off_and_below_the_bound_means_untouched(pkg, rule, armed, prec):
    """clipping never set, max_norm = 0 set explicitly, and a bound far above every norm end in bit-identical weights and state"""
    rng = np.random.RandomState(33)
    layers = three_layer_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = two_fractions(pkg, rng)
    res = [run_plain(pkg, layers, weights, fracs, getattr(pkg, prec), rule, armed, clip) for clip in (None, 0.0, 1e30)]
    for other, _ in res[1:]:
        for a, b in zip(res[0][0], other):
            assert np.array_equal(a, b)
    for st in (res[0][1], res[1][1]):                       # with clipping off the stats are zeros
        assert (float(st["last_norm"]), float(st["last_scale"]), st["updates"], st["clipped"], st["skipped"]) == (0.0, 0.0, 0, 0, 0)
    assert res[2][1]["updates"] == 3 and res[2][1]["clipped"] == 0 and res[2][1]["last_norm"] > 0


# ---- skipped steps, large values -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["all", "layer"])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_non_finite_gradient_skips_the_step(pkg, bad, rule, how):
    """one inf / NaN entry: weights, deltas, second moments and the next forward pass's posteriors are unchanged, `skipped`
    counts it, and the finite step that follows is the restatement's.  (Ordinary arithmetic on non-finite values.)"""
    rng = np.random.RandomState(34)
    layers = three_layer_net()
    weights = random_weights(layers, rng, 0.2)
    frac = two_fractions(pkg, rng)[0]
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=pkg.PREC_F32) as net:
        segs, total = segments(net, LR)
        net.set_grad_clip(0.05)
        net.load_sequences(frac); net.compute_forward_pass()
        y0 = net.outputs()
        for _, _, _, l in segs:                             # one finite clipped step first, so that the state is not all zeros
            l.upload("weightUpdates", test_gradients(rng, l.weight_count))
        update(net, rule, how, 1)
        net.compute_forward_pass()
        y1 = net.outputs()
        assert not np.array_equal(y0, y1)
        before = state_of(net, segs, total)
        for k, (_, _, _, l) in enumerate(segs):
            g = test_gradients(rng, l.weight_count)
            if k == 1:
                g[7] = bad
            l.upload("weightUpdates", g)
        update(net, rule, how, 2)
        st = net.grad_clip_stats()
        assert (st["updates"], st["clipped"], st["skipped"]) == (2, 1, 1) and float(st["last_scale"]) == 0.0
        assert_state(state_of(net, segs, total), before, "adam", (bad, rule, how, "skipped"))
        net.compute_forward_pass()
        assert np.array_equal(net.outputs(), y1)
        for _, _, _, l in segs:
            l.upload("weightUpdates", test_gradients(rng, l.weight_count))
        g = arena(net, segs, total, lambda l: l.weight_updates())
        update(net, rule, how, 3)
        want = reference_step(rule, before, g, segs, np.float32(0.05), 3)
        assert not want[5] and want[4] is not None
        assert_state(state_of(net, segs, total), want, rule, (bad, rule, how, "after"))
        assert net.grad_clip_stats()["skipped"] == 1


@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_squares_beyond_fp32_clip_to_the_bound(pkg, rule):
    """a gradient of all 3e19: every square overflows fp32, the double sum does not; the step clips as the restatement says"""
    layers = softmax_net(1, 4)
    rng = np.random.RandomState(35)
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.1), 2, 3, precision=pkg.PREC_F32) as net:
        segs, total = segments(net, LR)
        net.set_grad_clip(1.0)
        before = state_of(net, segs, total)
        segs[0][3].upload("weightUpdates", np.full(8, 3e19, np.float32))
        update(net, rule, "all", 1)
        want = reference_step(rule, before, np.full(8, 3e19, np.float32), segs, np.float32(1.0), 1)
        st = net.grad_clip_stats()
        assert not want[5] and st["skipped"] == 0 and st["clipped"] == 1
        assert st["last_norm"].tobytes() == want[3].tobytes() and st["last_scale"].tobytes() == want[4].tobytes()
        got = state_of(net, segs, total)
        assert_state(got, want, rule, rule)
        assert all(np.all(np.isfinite(a)) for a in got) and np.isfinite(st["last_norm"])
        assert not np.array_equal(got[0], before[0])


# ---- operand copies, batch learning --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
@pytest.mark.parametrize("armed", [False, True])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_operand_copies_follow_the_clipped_weights(pkg, rule, armed, prec):
    """after clipped updates a fresh network built from the weights read back computes bit-identical posteriors"""
    rng = np.random.RandomState(36)
    layers = three_layer_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = two_fractions(pkg, rng)
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=getattr(pkg, prec), deterministic=True) as net:
        net.set_grad_clip(0.1)
        for step in (1, 2, 3):
            net.load_sequences(fracs[0]); net.compute_forward_pass()
            if armed:
                arm(net, rule, step)
            net.compute_backward_pass()
            update(net, rule, "all", step)
        assert net.grad_clip_stats()["clipped"] == 3
        net.compute_forward_pass()
        y = net.outputs()
        trained = net.export_weights()
    assert all(not np.array_equal(np.asarray(trained[n]["input"], np.float32), weights[n]["input"]) for n in weights)
    with pkg.NeuralNetwork(layers, trained, 8, 17, precision=getattr(pkg, prec), deterministic=True) as fresh:
        fresh.load_sequences(fracs[0]); fresh.compute_forward_pass()
        assert np.array_equal(fresh.outputs(), y)


@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_batch_learning_clips_the_epoch_sum(pkg, rule):
    rng = np.random.RandomState(37)
    layers = three_layer_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = two_fractions(pkg, rng)
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=pkg.PREC_F32) as net:
        segs, total = segments(net, LR)
        before = state_of(net, segs, total)
        single = []
        for k, f in enumerate(fracs):
            net.load_sequences(f); net.compute_forward_pass(); net.compute_backward_pass()
            single.append(arena(net, segs, total, lambda l: l.weight_updates()))
            net.accumulate_updates(k == 0)
        net.take_accumulated()
        g = arena(net, segs, total, lambda l: l.weight_updates())
        assert np.array_equal(g, single[0] + single[1])
        bound = np.float32(0.25) * CR.clip_factor(g, 0.0)[0]
        net.set_grad_clip(bound)
        update(net, rule, "all", 1)
        want = reference_step(rule, before, g, segs, bound, 1)
        st = net.grad_clip_stats()
        assert st["last_norm"].tobytes() == want[3].tobytes() and want[4] is not None        # the norm of the epoch sum
        assert st["last_norm"] > CR.clip_factor(single[1], 0.0)[0]
        assert_state(state_of(net, segs, total), want, rule, rule)


# ---- arguments and state -------------------------------------------------------------------------------------------------------
def test_grad_clip_arguments_and_state(pkg):
    rng = np.random.RandomState(38)
    layers = three_layer_net()
    weights = random_weights(layers, rng, 0.2)
    frac = two_fractions(pkg, rng)[0]
    E = pkg.CurrenntHipError
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=pkg.PREC_F32) as net:
        st = net.grad_clip_stats()                            # a fresh context is off: zeros
        assert (float(st["last_norm"]), float(st["last_scale"]), st["updates"], st["clipped"], st["skipped"], float(st["max_norm_seen"])) == (0.0, 0.0, 0, 0, 0, 0.0)
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(E) as e:
                net.set_grad_clip(bad)
            assert e.value.code == -1                         # CN_ERR_BAD_ARG
        assert net.lib.cn_ctx_grad_clip_stats(net.ctx, None, None, None, None, None, None, 0) == 0      # any pointer may be NULL
        net.load_sequences(frac); net.compute_forward_pass()
        net.arm_update(LR, MOM)                               # armed without clipping: the bound may not change under it
        with pytest.raises(E, match="armed") as e:
            net.set_grad_clip(1.0)
        assert e.value.code == -4                             # CN_ERR_STATE
        net.compute_backward_pass()
        with pytest.raises(E, match="armed") as e:
            net.set_grad_clip(1.0)
        assert e.value.code == -4
        net.update_weights_fused(LR, MOM)
        net.set_grad_clip(1.0)                                # completed: accepted
        net.compute_forward_pass()
        net.arm_update(LR, MOM)                               # armed with clipping on: accepted, checked, pending
        for call in (lambda: net.set_grad_clip(2.0), lambda: net.set_grad_clip(0.0), lambda: net.accumulate_updates(True)):
            with pytest.raises(E, match="armed") as e:
                call()
            assert e.value.code == -4
        net.compute_backward_pass()
        with pytest.raises(E, match="differ from what cn_ctx_arm_update armed") as e:
            net.update_weights_fused(2 * LR, MOM)
        assert e.value.code == -4
        net.update_weights_fused(LR, MOM)
        net.set_grad_clip(2.0)                                # may be changed between steps
        st = net.grad_clip_stats(reset=True)
        assert st["updates"] == 1 and st["last_norm"] > 0
        st = net.grad_clip_stats()
        assert st["updates"] == 0 and float(st["max_norm_seen"]) == 0.0 and st["last_norm"] > 0
        net.set_grad_clip(0.0)
        st = net.grad_clip_stats()
        assert (float(st["last_norm"]), st["updates"]) == (0.0, 0)


# ---- data-parallel -------------------------------------------------------------------------------------------------------------
def test_clip_data_parallel_replicas_stay_identical(pkg, tmp_path):
    """Two ranks on one device through the library's test backend (tests/clip_rank.py): different sequences per rank, a bound
    that clips, three armed steps.  Both ranks report the same norm bits each step and hold bit-identical weights and state."""
    world = 2
    env = dict(os.environ, CN_COMM_BACKEND="ipc", HSA_ENABLE_IPC_MODE_LEGACY="0", CN_COMM_IPC_TIMEOUT="60")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "clip_rank.py"), str(r), str(world), str(tmp_path)],
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
    for key in ("w", "m", "v", "g", "norms", "scales"):
        assert res[0][key].tobytes() == res[1][key].tobytes(), key
    assert int(res[0]["clipped"]) == 3 and np.all(res[0]["scales"] < 1) and np.all(res[0]["norms"] > 0)
    assert np.abs(res[0]["w"] - res[0]["w0"]).max() > 1e-4 and res[0]["v"].any()
    # ... and the norm each rank reports is the restatement's norm of the reduced gradient (the arena: layers padded to four)
    for step in range(3):
        assert res[0]["norms"][step].tobytes() == CR.clip_factor(res[0]["g"][step], 0.0)[0].tobytes()
