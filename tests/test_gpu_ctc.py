"""-m gpu: the CTC post output layer (csrc/cn_ctc.hip) against its float64 model (tests/ctc_reference.py).

Kernel level, through cn_dbg_ctc (the layer's launches on posteriors of the test's choice): the loss is compared relatively,
the output errors as the scale-free product y * dL/dy (in [-1, 0]) by maximum absolute difference.  The bound is K * D_ref
with D_ref the distance of the model run in float32 from the model run in float64 on the same inputs (computed here, on the
CPU) and K = 8.46, the factor tests/test_gpu_long_fp64.py holds the GPU to against the fp64 oracle: it covers another summation
order and v_exp / v_log.  Only where D_ref is exactly 0 (the float32 model hit the rounded float64 value) does half an ulp of
the compared quantity, 2^-24, stand in for it.

Then through a net (6 -> blstm 8 -> softmax 5 -> ctc), the state and argument errors, and the driver."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ctc_reference import ctc_fraction, softmax_jacobian

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
K = 8.46
HALF_ULP = 2.0 ** -24         # stands in for a D_ref of exactly 0


def bound(d_ref):
    return K * (d_ref if d_ref > 0 else HALF_ULP)
GRAD_TOL = 2e-4               # gradients against the layer's maximum: test_gpu_parity.check_network


@pytest.fixture(scope="module")
def ctx(pkg, hiplib):
    h = C.c_void_p()
    pkg.binding.check(hiplib.cn_ctx_create(0, pkg.PREC_F32, None, C.byref(h)))
    yield h
    hiplib.cn_ctx_destroy(h)


def dbg_ctc(pkg, hiplib, ctx, y, pat, labels):
    """cn_dbg_ctc on y [T][PS][C] float32, pat [T][PS]: (loss [PS], dL/dy [T][PS][C])."""
    T, PS, Cn = y.shape
    y = np.ascontiguousarray(y, np.float32)
    pat = np.ascontiguousarray(pat, np.int8)
    lens = np.asarray([len(l) for l in labels], np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in labels] + [np.zeros(1, np.int32)]))
    loss = np.full(PS, np.nan, np.float32)
    err = np.full((T, PS, Cn), np.nan, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    pkg.binding.check(hiplib.cn_dbg_ctc(ctx, vp(y), vp(pat), T, PS, Cn, vp(flat), vp(lens), vp(loss), vp(err)), ctx)
    return loss, err


def posteriors(rng, T, PS, Cn, sharp=1.5):
    z = rng.randn(T, PS, Cn) * sharp
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def pattern(T, PS, lens):
    pat = np.zeros((T, PS), np.int8)
    for s, n in enumerate(lens):
        pat[:n, s] = 2
    return pat


def check_against_model(pkg, hiplib, ctx, y, pat, labels, name):
    """Runs the hook and holds it to the float64 model; returns (loss, err, feasible flags of the model)."""
    loss, err = dbg_ctc(pkg, hiplib, ctx, y, pat, labels)
    l64, g64, ok = ctc_fraction(y, pat, labels, np.float64)
    l32, g32, ok32 = ctc_fraction(y, pat, labels, np.float32)
    assert np.array_equal(ok, ok32)
    assert np.isfinite(loss).all() and np.isfinite(err).all(), name
    real = pat != 0
    assert not err[~real].any(), "%s: output errors outside the real frames are not exactly 0" % name
    assert not err[:, ~ok].any() and not loss[~ok].any(), "%s: a sequence without an alignment contributes" % name
    y64 = y.astype(np.float64)
    d_ref = np.abs(y64 * g32 - y64 * g64).max()
    d_gpu = np.abs(y64 * err - y64 * g64).max()
    dl_ref = (np.abs(l32[ok] - l64[ok]) / np.abs(l64[ok])).max() if ok.any() else 0.0
    dl_gpu = (np.abs(loss[ok] - l64[ok]) / np.abs(l64[ok])).max() if ok.any() else 0.0
    print("%s: y*dL/dy gpu %.3g ref %.3g ratio %.2f | loss rel gpu %.3g ref %.3g ratio %.2f"
          % (name, d_gpu, d_ref, d_gpu * K / bound(d_ref), dl_gpu, dl_ref, dl_gpu * K / bound(dl_ref)))
    assert d_gpu <= bound(d_ref), name
    assert dl_gpu <= bound(dl_ref), name
    return loss, err, ok


def test_three_slots_one_empty(pkg, hiplib, ctx):
    """PS = 3 with one empty slot, lengths 12 / 7 / 0, a repeated label."""
    rng = np.random.RandomState(1)
    y, pat = posteriors(rng, 12, 3, 6), pattern(12, 3, [12, 7, 0])
    loss, err, ok = check_against_model(pkg, hiplib, ctx, y, pat, [[0, 3, 3, 1], [2], []], "ps3")
    assert list(ok) == [True, True, False] and loss[0] > 0 and loss[1] > 0


def test_five_slots_no_labels_and_five_repeats(pkg, hiplib, ctx):
    """PS = 5 (not a multiple of the slot padding): U = 0, one label repeated five times with U + repeats == len exactly, an
    infeasible sequence (U + repeats = 5 > len = 3) among feasible ones."""
    rng = np.random.RandomState(2)
    lens = [9, 5, 8, 3, 6]
    y, pat = posteriors(rng, 9, 5, 7), pattern(9, 5, lens)
    labels = [[1, 1, 1, 1, 1], [], [0, 5, 0], [2, 2, 2], [4, 3]]
    loss, err, ok = check_against_model(pkg, hiplib, ctx, y, pat, labels, "ps5")
    assert list(ok) == [True, True, True, False, True]
    assert loss[3] == 0.0 and (loss[[0, 1, 2, 4]] > 0).all()
    # U = 0: only the blank carries an error, -1 / y on every real frame
    assert np.allclose(y[:5, 1, 6] * err[:5, 1, 6], -1.0, atol=1e-6) and not err[:, 1, :6].any()


@pytest.mark.parametrize("U,T,Cn,PS", [(130, 300, 40, 2), (300, 640, 20, 1), (600, 1300, 12, 1), (1100, 2300, 12, 1)],
                         ids=["S261", "S601", "S1201", "S2201"])
def test_more_states_than_threads(pkg, hiplib, ctx, U, T, Cn, PS):
    """S = 261 (two states per thread) and one shape for each further count of states per thread (4, 8, 16): random posteriors,
    where the states an alignment must pass through lie far below the largest of their column."""
    rng = np.random.RandomState(U)
    lens = [T, T - 20][:PS]
    y, pat = posteriors(rng, T, PS, Cn, sharp=1.0), pattern(T, PS, lens)
    labels = [list(rng.randint(0, Cn - 1, U)), list(rng.randint(0, Cn - 1, U - 30))][:PS]
    check_against_model(pkg, hiplib, ctx, y, pat, labels, "S%d" % (2 * U + 1))


def test_underflow_territory(pkg, hiplib, ctx):
    """T = 64: posteriors of 1e-30 on every label but the one of a fixed alignment (0.9 there)."""
    rng = np.random.RandomState(4)
    T, Cn = 64, 8
    labels = [3, 3, 0, 5, 1, 1, 6, 2]
    path = []
    for k in labels:
        path += [Cn - 1] * int(rng.randint(1, 4)) + [k] * int(rng.randint(2, 5))
    path = (path + [Cn - 1] * T)[:T]
    y = np.full((T, 1, Cn), 1e-30, np.float32)
    y[:, 0, 4] = 0.1                                                    # (a class outside the labels takes the rest)
    y[np.arange(T), 0, path] = 0.9
    loss, err, ok = check_against_model(pkg, hiplib, ctx, y, pattern(T, 1, [T]), [labels], "underflow")
    assert ok[0]
    # and a second sequence whose alignment must leave the path: p is of the order 1e-30 per frame off it
    y2 = np.concatenate([y, y], axis=1)
    check_against_model(pkg, hiplib, ctx, y2, pattern(T, 2, [T, T - 9]), [labels, labels[:5] + [4, 4]], "underflow_off_path")


def test_exact_zeros(pkg, hiplib, ctx):
    """Posteriors with exact zeros: classes outside l', and classes of l' away from one alignment that keeps p > 0.  A posterior
    of exactly 0 gives an output error of 0, not NaN."""
    rng = np.random.RandomState(5)
    T, Cn = 20, 6
    labels = [1, 4, 4, 0]
    path = [5, 1, 1, 5, 4, 4, 5, 5, 4, 4, 4, 0, 0, 5, 5, 5, 5, 5, 5, 5]
    y = posteriors(rng, T, 2, Cn).astype(np.float64)
    y[rng.rand(T, 2, Cn) < 0.4] = 0.0
    y[np.arange(T), 0, path] += 0.2
    y[np.arange(T), 1, path] += 0.2
    y[:, :, 2] = 0.0
    y = (y / y.sum(axis=-1, keepdims=True)).astype(np.float32)
    assert (y == 0).sum() > 40
    loss, err, ok = check_against_model(pkg, hiplib, ctx, y, pattern(T, 2, [T, 17]), [labels, labels], "zeros")
    assert ok.all() and not err[y == 0].any()
    # every alignment of the second label sequence crosses a zero: p = 0, nothing contributes
    y0 = y.copy()
    y0[:, 0, 3] = 0.0
    loss, err = dbg_ctc(pkg, hiplib, ctx, y0[:, :1], pattern(T, 1, [T]), [[3, 1]])
    assert loss[0] == 0.0 and not err.any()


def test_two_runs_bit_identical(pkg, hiplib, ctx):
    """Repeated labels (several states per class) and more states than threads: the sums have a fixed order."""
    rng = np.random.RandomState(6)
    y, pat = posteriors(rng, 300, 3, 9, sharp=1.0), pattern(300, 3, [300, 250, 120])
    labels = [list(rng.randint(0, 8, 140)), list(rng.randint(0, 3, 90)), [7] * 60]
    assert hiplib.cn_ctx_set_option(ctx, b"deterministic", 1) == 0
    a = dbg_ctc(pkg, hiplib, ctx, y, pat, labels)
    b = dbg_ctc(pkg, hiplib, ctx, y, pat, labels)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].all()


# ---- through a net -----------------------------------------------------------------------------------------------------------

def ctc_net():
    return [{"name": "input", "type": "input", "size": 6},
            {"name": "blstm", "type": "blstm", "size": 8, "bias": 1.0},
            {"name": "output", "type": "softmax", "size": 5, "bias": 1.0},
            {"name": "postoutput", "type": "ctc", "size": 5}]


def toy_set(rng, n_seq, max_len=14):
    """One distinct input pattern per label (a unit vector plus a little noise), runs of 2-4 frames per label."""
    xs, labels = [], []
    while len(xs) < n_seq:
        l = list(rng.randint(0, 4, rng.randint(1, 5)))
        frames = [k for k in l for _ in range(rng.randint(2, 5))]
        if len(frames) > max_len:
            continue
        x = np.zeros((len(frames), 6), np.float32)
        x[np.arange(len(frames)), frames] = 1.0
        xs.append(x + 0.05 * rng.randn(len(frames), 6).astype(np.float32))
        labels.append(l)
    return xs, labels


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16X3"])
def test_net_error_and_output_gradient(pkg, prec):
    from helpers import random_weights
    rng = np.random.RandomState(8)
    layers = ctc_net()
    weights = random_weights(layers, rng, 0.4)
    xs, labels = toy_set(rng, 3)
    labels[2] = [0] * (len(xs[2]) // 2 + 2)                            # U + repeats = 2U - 1 > len: no alignment
    frac = pkg.make_fraction(xs, None, 3, labels=labels)
    with pkg.NeuralNetwork(layers, weights, 3, 14, precision=getattr(pkg, prec)) as net:
        net.load_sequences(frac)
        net.compute_forward_pass()
        err, count = net.error_and_correct()
        y = net.outputs()                                               # [T][PS][5] float32, as the layer saw them
        pat = frac["patTypes"].reshape(net.T, 3)
        l64, g64, ok = ctc_fraction(y, pat, labels, np.float64)
        l32, _, _ = ctc_fraction(y, pat, labels, np.float32)
        assert list(ok) == [True, True, False] and count == 2
        d_ref = abs(float(l32.sum()) - l64.sum()) / l64.sum()
        print("%s: error %.8g model %.8g rel %.3g ref %.3g" % (prec, err, l64.sum(), abs(err - l64.sum()) / l64.sum(), d_ref))
        assert abs(err - l64.sum()) / l64.sum() <= bound(d_ref)
        net.compute_backward_pass()
        x = net.layer("blstm").outputs().astype(np.float64).reshape(-1, 8)
        delta = softmax_jacobian(y, g64).reshape(-1, 5)
        want = np.concatenate([(delta.T @ x).reshape(-1), 1.0 * delta.sum(axis=0)])          # [unit][input], then bias * column sums
        got = net.layer("output").weight_updates().astype(np.float64)
        d = np.abs(got - want).max() / np.abs(want).max()
        print("%s: output layer weightUpdates against sum_n x_n delta_n^T: %.3g of the layer's max" % (prec, d))
        assert d <= GRAD_TOL
        oe = net.layer("output").output_errors()                        # dL/dz after the softmax backward pass
        assert not oe[pat == 0].any() and not oe[:, 2].any()


def test_forty_updates_lower_the_error(pkg):
    from helpers import random_weights
    rng = np.random.RandomState(9)
    layers = ctc_net()
    xs, labels = toy_set(rng, 6)
    fracs = [pkg.make_fraction(xs[i:i + 3], None, 3, labels=labels[i:i + 3]) for i in (0, 3)]
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.1), 3, 14, precision=pkg.PREC_F32) as net:
        def total():
            e = 0.0
            for f in fracs:
                net.load_sequences(f); net.compute_forward_pass()
                e += net.calculate_error()
            return e
        before = total()
        for step in range(40):
            f = fracs[step % 2]
            net.load_sequences(f); net.compute_forward_pass(); net.compute_backward_pass()
            net.update_weights(1e-2, 0.9)
        after = total()
        print("summed ctc error: %.6g before, %.6g after forty updates" % (before, after))
        assert np.isfinite(after) and after < before


# ---- state and argument errors -----------------------------------------------------------------------------------------------

def test_state_and_argument_errors(pkg):
    from helpers import random_weights
    rng = np.random.RandomState(10)
    layers = ctc_net()
    xs, labels = toy_set(rng, 3)
    frac = pkg.make_fraction(xs, None, 3, labels=labels)
    bare = dict(frac); bare.pop("labels")
    E = pkg.binding.CurrenntHipError
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.1), 3, 14, options={"ctc_max_labels": 6}) as net:
        assert net.get_option("ctc_max_labels") == 6
        net.load_sequences(bare); net.compute_forward_pass()
        for call in (net.calculate_error, net.loss_accumulate, net.compute_backward_pass):
            with pytest.raises(E) as ei:                              # loss before labels
                call()
            assert ei.value.code == -4
        net.set_label_sequences(labels)
        assert np.isfinite(net.calculate_error())
        net.load_sequences(bare); net.compute_forward_pass()          # the labels belonged to the previous fraction
        with pytest.raises(E) as ei:
            net.calculate_error()
        assert ei.value.code == -4
        with pytest.raises(E) as ei:                                  # the blank is not a label
            net.set_label_sequences([[4], [0], [1]])
        assert ei.value.code == -1
        with pytest.raises(E) as ei:                                  # another number of sequences than the fraction's
            net.set_label_sequences(labels[:2])
        assert ei.value.code == -1
        with pytest.raises(E) as ei:                                  # above the cap
            net.set_label_sequences([[0] * 7, [0], [1]])
        assert ei.value.code == -2 and "6" in str(ei.value) and "ctc_max_labels" in str(ei.value)
        net.set_label_sequences(labels)
        assert np.isfinite(net.calculate_error())
    bad = ctc_net()
    bad[2]["type"] = "feedforward_identity"
    with pytest.raises(E) as ei:                                      # a ctc layer behind a non-softmax layer
        pkg.NeuralNetwork(bad, random_weights(bad, rng, 0.1), 3, 14)
    assert ei.value.code == -1


# ---- driver ------------------------------------------------------------------------------------------------------------------

def test_driver_trains_a_ctc_net(tmp_path):
    """`--train true` on a written .nc (labels = the collapsed target classes): a finite error per epoch, a label error rate
    for the validation set, '-' in the training column; twice with --optimizer steepest_descent in f32: the same table to the
    last digit."""
    from helpers import random_weights
    from test_host_dataset import write_nc
    rng = np.random.RandomState(12)
    files = {}
    for name, n_seq in (("train", 7), ("val", 4)):
        xs, labels = toy_set(rng, n_seq)
        ts = [np.argmax(np.round(x), axis=1).astype(np.int32) for x in xs]            # the frame's pattern is its class
        files[name] = str(tmp_path / (name + ".nc"))
        write_nc(files[name], xs, ts, 4, name[0])
    layers = ctc_net()
    weights = random_weights(layers, rng, 0.1)
    net = str(tmp_path / "ctc.jsn")
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    args = [BIN, "--train", "true", "--train_file", files["train"], "--val_file", files["val"], "--network", net,
            "--parallel_sequences", "3", "--max_epochs", "4", "--max_epochs_no_best", "10", "--learning_rate", "1e-2", "--momentum", "0.9",
            "--optimizer", "steepest_descent", "--precision", "f32", "--shuffle_fractions", "false", "--shuffle_sequences", "false"]
    tables = []
    for _ in range(2):
        out = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = [re.sub(r"\|\s*[0-9.]+ \|", "|", l, count=1) for l in out.stdout.splitlines() if re.match(r"^\s+\d+ \|", l)]     # without the duration
        assert len(rows) == 4, out.stdout
        for r in rows:
            cols = [c.strip() for c in r.split("|")]
            train, val = cols[1], cols[2]
            assert re.fullmatch(r"-\s+[0-9]+\.[0-9]{3}", train), r
            m = re.fullmatch(r"([0-9]+\.[0-9]{2})%\s+([0-9]+\.[0-9]{3})", val)
            assert m and np.isfinite(float(m.group(2))) and 0.0 <= float(m.group(1)), r
        tables.append(rows)
    assert tables[0] == tables[1]
