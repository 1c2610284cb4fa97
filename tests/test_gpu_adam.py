"""-m gpu: the Adam update (cn_adam_update, cn_adam_update_all, cn_ctx_arm_adam) against its numpy restatement
(tests/adam_reference.py), bit for bit, on every path that applies it: the flat kernel, the update fused into the grouped
operand-copy launch, the armed per-layer forms that unpack the packed gradient or add the stored partial sums; then the
protocol's errors, the driver option with autosave / continue, and two data-parallel ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from adam_reference import adam_step, test_gradients
from helpers import GOLDEN, net_desc, random_sequences, random_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
HP = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LR, OWN_LR = 1e-3, 4e-3


def small_net():
    return net_desc(5, [("lstm", 8)], 3)


def second_net():
    """13 -> blstm 64 -> feedforward_tanh 24 (own learningRate) -> lstm 32 -> softmax 9: input, bias, recurrent and peephole
    sections of both LSTM pack bodies' directions, a feed-forward layer with the bias scale (bias 0.7), a per-layer rate."""
    layers = net_desc(13, [("blstm", 64), ("feedforward_tanh", 24), ("lstm", 32)], 9, bias=0.7)
    layers[2]["learningRate"] = OWN_LR
    return layers


def lr_of(lay):
    return lay.learning_rate if lay.learning_rate >= 0.0 else LR


def state_of(net):
    return {l.name: (l.weights(), l.first_moments(), l.second_moments()) for l in net.trainable_layers()}


def same_state(a, b):
    return all(np.array_equal(x, y) for n in a for x, y in zip(a[n], b[n]))


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16", "PREC_BF16X3"])
@pytest.mark.parametrize("per_layer", [False, True])
@pytest.mark.parametrize("which", ["small", "second"])
def test_adam_update_equals_restatement(pkg, prec, per_layer, which):
    """Gradients uploaded through cn_layer_upload (magnitudes 1e-6 ... 1, exact zeros), 5 steps of cn_adam_update_all (the
    grouped launch) or cn_adam_update per layer (the flat kernel): weights, first and second moments EQUAL the restatement."""
    layers = small_net() if which == "small" else second_net()
    rng = np.random.RandomState(21)
    weights = random_weights(layers, rng, 0.3)
    with pkg.NeuralNetwork(layers, weights, 4, 6, precision=getattr(pkg, prec)) as net:
        ref = {l.name: (l.weights(), np.zeros(l.weight_count, np.float32), np.zeros(l.weight_count, np.float32)) for l in net.trainable_layers()}
        for l in net.trainable_layers():
            assert not l.second_moments().any() and not l.first_moments().any()
        for step in range(1, 6):
            for l in net.trainable_layers():
                g = test_gradients(rng, l.weight_count)
                l.upload("weightUpdates", g)
                ref[l.name] = adam_step(ref[l.name][0], g, ref[l.name][1], ref[l.name][2], lr_of(l), step=step, **HP)
            net.update_weights_adam(LR, step=step, per_layer=per_layer, **HP)
            got = state_of(net)
            for l in net.trainable_layers():
                for what, a, b in zip(("weights", "first moments", "second moments"), got[l.name], ref[l.name]):
                    assert np.array_equal(a, b), (step, l.name, what, float(np.abs(a - b).max()), int((a != b).sum()))
        assert all(np.abs(ref[n][0] - np.concatenate([weights[n][k] for k in ("input", "bias", "internal")])).max() > 1e-3 for n in ref)


def two_fractions(pkg, rng, PS=8, T=17):
    out = []
    for k in range(2):
        xs, ts = random_sequences(rng, [T - ((i + k) % 5) for i in range(PS)], 13, C=9)
        out.append(pkg.make_fraction(xs, ts, PS))
    return out


def run_armed(pkg, layers, weights, fracs, prec, det, mode, steps=4):
    """mode: "armed_all" (cn_ctx_arm_adam, completed by cn_adam_update_all), "armed_layer" (completed per layer), "plain"
    (update after the backward pass).  Every step is held to the restatement: weights and moments read before, weightUpdates
    read after -> weights and moments read after."""
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=prec, deterministic=det) as net:
        for step in range(1, steps + 1):
            before = state_of(net)
            net.load_sequences(fracs[(step - 1) % 2]); net.compute_forward_pass()
            if mode != "plain":
                net.arm_adam(LR, step=step, **HP)
            net.compute_backward_pass()
            net.update_weights_adam(LR, step=step, per_layer=(mode == "armed_layer"), **HP)
            after = state_of(net)
            for l in net.trainable_layers():
                g = l.weight_updates()
                assert np.abs(g).max() > 0
                want = adam_step(before[l.name][0], g, before[l.name][1], before[l.name][2], lr_of(l), step=step, **HP)
                for what, a, b in zip(("weights", "first moments", "second moments"), after[l.name], want):
                    assert np.array_equal(a, b), (mode, step, l.name, what, float(np.abs(a - b).max()), int((a != b).sum()))
        return state_of(net)


@pytest.mark.parametrize("prec,det", [("PREC_F32", True), ("PREC_BF16", True), ("PREC_BF16", False)])
def test_armed_adam_forms(pkg, prec, det):
    """Real forward and backward passes on the second net (PS 8, T 17, two alternating fractions, 4 steps).  Deterministic: the
    armed update adds the stored partial sums itself (update mode 3); the three ways to run a step end in bit-identical weights
    and moments.  Not deterministic (bf16's default): the armed update unpacks the packed accumulators (mode 2); runs differ in
    the order of their atomic sums, each step is still the restatement of its own gradient."""
    rng = np.random.RandomState(22)
    layers = second_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = two_fractions(pkg, rng)
    res = {mode: run_armed(pkg, layers, weights, fracs, getattr(pkg, prec), det, mode) for mode in ("armed_all", "armed_layer", "plain")}
    if det:
        assert same_state(res["armed_all"], res["armed_layer"]) and same_state(res["armed_all"], res["plain"])


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
@pytest.mark.parametrize("armed", [False, True])
def test_operand_copies_follow_the_adam_weights(pkg, prec, armed):
    """After 3 Adam steps the operand copies the kernels read are those of the updated weights: a fresh network built from
    the weights read back computes bit-identical posteriors."""
    rng = np.random.RandomState(23)
    layers = second_net()
    weights = random_weights(layers, rng, 0.2)
    fracs = two_fractions(pkg, rng)
    with pkg.NeuralNetwork(layers, weights, 8, 17, precision=getattr(pkg, prec), deterministic=True) as net:
        for step in (1, 2, 3):
            net.load_sequences(fracs[step % 2]); net.compute_forward_pass()
            if armed:
                net.arm_adam(LR, step=step, **HP)
            net.compute_backward_pass()
            net.update_weights_adam(LR, step=step, **HP)
        net.load_sequences(fracs[0]); net.compute_forward_pass()
        y = net.outputs()
        trained = net.export_weights()
    assert any(np.abs(np.asarray(trained[n]["input"], np.float32) - weights[n]["input"]).max() > 1e-3 for n in weights)
    with pkg.NeuralNetwork(layers, trained, 8, 17, precision=getattr(pkg, prec), deterministic=True) as fresh:
        fresh.load_sequences(fracs[0]); fresh.compute_forward_pass()
        assert np.array_equal(fresh.outputs(), y)


def test_adam_state_and_argument_errors(pkg):
    rng = np.random.RandomState(24)
    layers = small_net()
    weights = random_weights(layers, rng, 0.3)
    xs, ts = random_sequences(rng, [6, 5, 4, 6], 5, C=3)
    frac = pkg.make_fraction(xs, ts, 4)
    E = pkg.CurrenntHipError

    def fresh():
        return pkg.NeuralNetwork(layers, weights, 4, 6, precision=pkg.PREC_F32)

    with fresh() as net:
        for l in net.trainable_layers():                       # before any Adam call: zeros
            assert l.second_moments().shape == (l.weight_count,) and not l.second_moments().any()
        for bad in (dict(step=0), dict(step=-3), dict(beta1=1.0), dict(beta2=1.0), dict(beta1=-0.1), dict(eps=0.0)):
            for call in (net.update_weights_adam, net.arm_adam, lambda *a, **k: net.update_weights_adam(*a, per_layer=True, **k)):
                with pytest.raises(E) as e:
                    call(LR, **dict(dict(step=1), **bad))
                assert e.value.code == -1, (bad, str(e.value))             # CN_ERR_BAD_ARG
        # (a refused call binds nothing: the context still takes steepest descent)
        net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
        net.update_weights_fused(1e-3, 0.9)
        for call in (lambda: net.update_weights_adam(LR, step=1), lambda: net.arm_adam(LR, step=1),
                     lambda: net.update_weights_adam(LR, step=1, per_layer=True)):
            with pytest.raises(E, match="steepest descent.*Adam|Adam.*steepest descent") as e:
                call()
            assert e.value.code == -4                                      # CN_ERR_STATE
    with fresh() as net:
        net.load_sequences(frac); net.compute_forward_pass()
        net.arm_adam(LR, step=1, **HP)
        with pytest.raises(E, match="armed") as e:
            net.accumulate_updates(True)
        assert e.value.code == -4
        net.compute_backward_pass()
        with pytest.raises(E, match="has not been completed") as e:        # a second backward pass before completion
            net.compute_backward_pass()
        assert e.value.code == -4
        for other in (dict(step=2), dict(beta1=0.8), dict(beta2=0.99), dict(eps=1e-7)):
            with pytest.raises(E, match="differ from what cn_ctx_arm_adam armed") as e:
                net.update_weights_adam(LR, **dict(dict(HP, step=1), **other))
            assert e.value.code == -4
        with pytest.raises(E, match="differ from what cn_ctx_arm_adam armed"):
            net.update_weights_adam(2 * LR, step=1, **HP)
        with pytest.raises(E, match="differ from what cn_ctx_arm_adam armed"):
            net.update_weights_adam(2 * LR, step=1, per_layer=True, **HP)
        net.update_weights_adam(LR, step=1, **HP)                          # the right values complete it
        for call in (lambda: net.update_weights_fused(1e-3, 0.9), lambda: net.update_weights(1e-3, 0.9), lambda: net.arm_update(1e-3, 0.9)):
            with pytest.raises(E, match="steepest descent.*Adam|Adam.*steepest descent") as e:
                call()
            assert e.value.code == -4
        net.load_sequences(frac); net.compute_forward_pass(); net.compute_backward_pass()
        net.update_weights_adam(LR, step=2, **HP)                          # and the context goes on with Adam
        assert all(l.second_moments().any() for l in net.trainable_layers())


def test_second_moments_upload_and_device_pointer(pkg):
    """CN_BUF_ADAM_SECOND_MOMENTS in cn_layer_upload / cn_layer_read / cn_layer_device_ptr: an uploaded state is what the next
    step starts from (the autosave path)."""
    rng = np.random.RandomState(25)
    layers = small_net()
    weights = random_weights(layers, rng, 0.3)
    with pkg.NeuralNetwork(layers, weights, 4, 6, precision=pkg.PREC_F32) as net:
        ref = {}
        ptrs = set()
        for l in net.trainable_layers():
            m = rng.uniform(-1e-2, 1e-2, l.weight_count).astype(np.float32)
            v = rng.uniform(1e-8, 1e-3, l.weight_count).astype(np.float32)
            g = test_gradients(rng, l.weight_count)
            l.upload("weightDeltas", m); l.upload("adamSecondMoments", v); l.upload("weightUpdates", g)
            assert np.array_equal(l.second_moments(), v) and np.array_equal(l.first_moments(), m)
            ptr = net.lib.cn_layer_device_ptr(l.handle, pkg.binding.BUF["adamSecondMoments"])
            assert ptr and ptr not in ptrs
            ptrs.add(ptr)
            ref[l.name] = adam_step(l.weights(), g, m, v, LR, step=7, **HP)
        net.update_weights_adam(LR, step=7, **HP)
        for l in net.trainable_layers():
            for a, b in zip((l.weights(), l.first_moments(), l.second_moments()), ref[l.name]):
                assert np.array_equal(a, b), l.name


def _weights_of(path):
    doc = json.load(open(path))
    return {n: np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in doc["weights"].items()}


def test_driver_adam_autosave_continue(pkg, tmp_path):
    """`--optimizer adam` in the C++ driver on a few sequences of tests/golden/val_1_speaker.nc (39 -> lstm 8 -> softmax 51),
    3 epochs, deterministic: the epoch-2 autosave carries both moment vectors and the step count, and --continue from it ends
    in the uninterrupted run's network bit for bit; steepest descent ends elsewhere; the other optimizer refuses the file."""
    nc = os.path.join(GOLDEN, "val_1_speaker.nc")
    rng = np.random.RandomState(26)
    layers = net_desc(39, [("lstm", 8)], 51)
    weights = random_weights(layers, rng, 0.1)
    net = str(tmp_path / "network.jsn")
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    common = [BIN, "--train", "true", "--stochastic", "true", "--train_file", nc, "--train_fraction", "0.06", "--network", net,
              "--parallel_sequences", "3", "--learning_rate", "1e-3", "--deterministic", "true", "--shuffle_fractions", "false",
              "--shuffle_sequences", "false", "--random_seed", "3"]
    straight, prefix = str(tmp_path / "straight.jsn"), str(tmp_path / "run")
    out = subprocess.run(common + ["--optimizer", "adam", "--momentum", "0.5", "--max_epochs", "3", "--autosave", "true", "--autosave_prefix", prefix,
                                   "--save_network", straight], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Optimizer type: Adam" in out.stdout and "ignored" in out.stdout
    auto = prefix + "_epoch002.autosave"
    state = json.load(open(auto))
    assert state["optimizer_cur_epoch"] == 2 and state["adam_optimizer_step"] == 4          # 6 sequences, 3 at a time, 2 epochs
    assert "steepest_descent_optimizer_weight_deltas" not in state
    for key in ("adam_optimizer_first_moments", "adam_optimizer_second_moments"):
        assert any(np.abs(np.asarray(a)).max() > 0 for a in state[key] if len(a))
    resumed = str(tmp_path / "resumed.jsn")
    out = subprocess.run([BIN, "--continue", auto, "--max_epochs", "3", "--autosave", "false", "--save_network", resumed],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Restoring state from" in out.stdout and "Optimizer type: Adam" in out.stdout
    a, b = _weights_of(straight), _weights_of(resumed)
    for name in a:
        assert np.array_equal(a[name], b[name]), (name, float(np.abs(a[name] - b[name]).max()))
    sgd = str(tmp_path / "sgd.jsn")
    out = subprocess.run(common + ["--optimizer", "steepest_descent", "--momentum", "0.9", "--max_epochs", "3", "--save_network", sgd],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Optimizer type: Steepest descent with momentum" in out.stdout
    c = _weights_of(sgd)
    assert any(not np.array_equal(a[n], c[n]) for n in a)
    out = subprocess.run([BIN, "--continue", auto, "--optimizer", "steepest_descent", "--max_epochs", "3", "--autosave", "false",
                          "--save_network", str(tmp_path / "never.jsn")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2
    assert "FAILED: The autosave file was written by the adam optimizer and cannot be continued with steepest_descent" in out.stdout
    assert not os.path.exists(str(tmp_path / "never.jsn"))


def test_adam_data_parallel_replicas_stay_identical(pkg, tmp_path):
    """Two ranks on one device through the library's test backend (tests/adam_rank.py): different sequences per rank, each
    layer's gradient exchanged behind its backward pass, the armed Adam step behind the exchange.  After 3 steps the replicas
    hold bit-identical weights and moments (and saw the same summed gradients)."""
    world = 2
    env = dict(os.environ, CN_COMM_BACKEND="ipc", HSA_ENABLE_IPC_MODE_LEGACY="0", CN_COMM_IPC_TIMEOUT="60")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "adam_rank.py"), str(r), str(world), str(tmp_path)],
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
        assert np.array_equal(res[0][key], res[1][key]), key
    assert np.abs(res[0]["w"] - res[0]["w0"]).max() > 1e-3 and res[0]["v"].any()
