"""-m gpu: residual connections between layers (include/currennt_hip.h, section Residual connections).  The forward sum is held
bit for bit to the restated rule (tests/residual_reference.py), the skip path of the backward pass to exact equality, the step
through the net to the fp64 autograd stack with h = branch(h) + h on the marked layers; then the recurrent-weight gradient on its
own, the armed update with prefetch beside it, that "off" is the old path bit for bit, and the errors."""
import copy
import ctypes as C

import numpy as np
import pytest

from dropout_reference import bf16_round
from helpers import net_desc, random_sequences, random_weights, real_mask
from residual_reference import autograd_residual, ff_delta, flat_weights, residual_sum
from test_gpu_dropout import TOL

pytestmark = pytest.mark.gpu

PRECS = ["PREC_F32", "PREC_BF16X3", "PREC_BF16"]


class Case:
    def __init__(self, pkg, P, hidden, marked, C, PS, lens, wscale, seed, bias=1.0):
        rng = np.random.RandomState(seed)
        self.P, self.hidden, self.C, self.PS, self.lens = P, hidden, C, PS, lens
        self.layers = net_desc(P, hidden, C, bias=bias)
        self.marked = tuple("%s_%d" % (hidden[i][0], i) for i in marked)
        self.weights = random_weights(self.layers, rng, wscale)
        self.xs, self.ts = random_sequences(rng, lens, P, C=C)
        self.frac = pkg.make_fraction(self.xs, self.ts, PS)
        self.T, self.N = self.frac["T"], self.frac["T"] * PS
        self._fp64 = {}

    def desc(self, marked=None, member=True):
        out = copy.deepcopy(self.layers)
        for d in out:
            if d["name"] in (self.marked if marked is None else marked):
                d["residual"] = True
            elif member and "bias" in d and d["type"] != "softmax":
                d["residual"] = False
        return out

    def net(self, pkg, prec, marked=None, weights=None, **kw):
        return pkg.NeuralNetwork(self.desc(marked), weights or self.weights, self.PS, self.T, precision=getattr(pkg, prec), **kw)

    def fp64(self, marked=None):
        """(loss, posteriors, gradients, errors as the library's buffers hold them after the backward pass) of the fp64 stack,
        computed once per marking."""
        marked = self.marked if marked is None else tuple(marked)
        if marked not in self._fp64:
            branches = {}
            loss, post, grads, errs = autograd_residual(self.layers, flat_weights(self.weights), self.frac, self.lens, marked, branches=branches)
            for kind, name in ((d["type"], d["name"]) for d in self.layers):
                if kind.startswith("feedforward") and name in errs:
                    errs[name] = ff_delta(kind, branches[name], errs[name])
            self._fp64[marked] = (loss, post, grads, errs)
        return self._fp64[marked]


@pytest.fixture(scope="module")
def small(pkg):
    """7 -> lstm 10 -> blstm 10 (R) -> feedforward_tanh 10 (R) -> lstm 10 (R) -> softmax 5, PS 3, lengths 9 / 6 / 4: dummy frames, a
    pad slot (PSp 4), H = 5 against Hp = 32; dense -> split, split -> dense and dense -> dense column maps; a residual LSTM layer
    whose predecessor is act(bias) on dummy frames."""
    return Case(pkg, 7, [("lstm", 10), ("blstm", 10), ("feedforward_tanh", 10), ("lstm", 10)], (1, 2, 3), 5, 3, [9, 6, 4], 0.3, 41)


@pytest.fixture(scope="module")
def wide(pkg):
    """13 -> blstm 64 -> feedforward_tanh 64 (R) -> lstm 64 (R) -> softmax 9, PS 8, T 17: more than one workgroup per launch, the
    16-byte path (dense -> dense)."""
    return Case(pkg, 13, [("blstm", 64), ("feedforward_tanh", 64), ("lstm", 64)], (1, 2), 9, 8, [17 - (i % 5) for i in range(8)], 0.2, 42, bias=0.7)


@pytest.fixture(scope="module")
def headline(pkg):
    """39 -> blstm 250 -> blstm 250 (R) -> blstm 250 (R) -> softmax 20, PS 4, lengths 24 / 24 / 17 / 9: the hand-written loops,
    H 125 / Hp 128, the 16-byte path (split -> split), residual on residual."""
    return Case(pkg, 39, [("blstm", 250), ("blstm", 250), ("blstm", 250)], (1, 2), 20, 4, [24, 24, 17, 9], 0.1, 43)


@pytest.fixture(scope="module")
def from_input(pkg):
    """10 -> lstm 10 (R) -> softmax 5: the predecessor is the input layer, nothing is added backward."""
    return Case(pkg, 10, [("lstm", 10)], (0,), 5, 3, [7, 5, 2], 0.3, 44)


def forward_backward(net, frac):
    net.load_sequences(frac)
    net.compute_forward_pass()
    e, _ = net.error_and_correct()
    net.compute_backward_pass()
    return e


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the forward sum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide", "headline", "from_input"])
def test_forward_sum_bit_for_bit(pkg, small, wide, headline, from_input, prec, which):
    case = {"small": small, "wide": wide, "headline": headline, "from_input": from_input}[which]
    bf16 = prec == "PREC_BF16"
    real = real_mask(case.frac)
    assert (~real).any()
    with case.net(pkg, prec) as net:
        net.load_sequences(case.frac)
        net.compute_forward_pass()
        branch_of = {}
        for lay in net.layers:
            if lay.name not in case.marked:
                continue
            b = lay.residual_branch().reshape(case.N, -1)
            x = lay.prev.outputs().reshape(case.N, -1)
            if bf16:
                x = bf16_round(x)      # (an unmarked feed-forward predecessor reports its fp32 outputs; its operand copy is their bf16 rounding)
            want = residual_sum(b, x, real, bf16)
            got = lay.outputs().reshape(case.N, -1)
            assert np.array_equal(bits(got), bits(want)), (prec, lay.name, int((bits(got) != bits(want)).sum()), float(np.abs(got - want).max()))
            assert np.array_equal(bits(got[~real]), bits(b[~real]))                       # rows that are no real frames: the branch
            if lay.type in ("lstm", "blstm"):
                assert np.all(got[~real] == 0)
            else:
                assert np.all(got[~real] != 0)                                             # (act(bias): the rule is not "zero")
            assert np.abs(x[real]).max() > 0 and (got[real] != b[real]).any()
            branch_of[lay.name] = b
    # the branch of a marked LSTM layer is what the layer computes unmarked on the same (summed) input
    for name in case.marked:
        if "lstm" not in name:
            continue
        before = case.marked[:case.marked.index(name)]
        with case.net(pkg, prec, marked=before) as net:
            net.load_sequences(case.frac)
            net.compute_forward_pass()
            y = net.layer(name).outputs().reshape(case.N, -1)
            with pytest.raises(pkg.CurrenntHipError) as ei:
                net.layer(name).residual_branch()
            assert ei.value.code == -4
        assert np.array_equal(bits(y), bits(branch_of[name])), (prec, name)


# ---- 2. the skip path, exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["lstm_3", "feedforward_tanh_2"])
@pytest.mark.parametrize("rate", [0.0, 0.5])
def test_skip_path_is_exact_and_never_dropped(pkg, small, prec, name, rate):
    """Input weights of exactly 0: the layer's own backward pass hands back exactly 0, so the predecessor's outputErrors are the
    injected ones on real frames -- with dropout on the layer too: the skip path passes no mask and no rescaling."""
    weights = copy.deepcopy(small.weights)
    weights[name]["input"] = np.zeros_like(weights[name]["input"])
    rng = np.random.RandomState(3)
    inject = rng.randn(small.N, 10).astype(np.float32)
    real = real_mask(small.frac)
    with small.net(pkg, prec, weights=weights) as net:
        lay = net.layer(name)
        if rate:
            lay.set_dropout(rate)
            net.set_dropout_pass(1, 77, 1)
        net.load_sequences(small.frac)
        net.compute_forward_pass()
        lay.write_output_errors(inject)
        assert net.lib.cn_layer_backward(lay.handle) == 0, net.lib.cn_last_error(net.ctx)
        got = lay.prev.output_errors().reshape(small.N, -1)
        if rate:
            assert (lay.dropout_input().reshape(small.N, -1)[real] == 0).any()             # (the pass did drop)
    assert np.array_equal(bits(got[real]), bits(inject[real])), (prec, name, rate, float(np.abs(got[real] - inject[real]).max()))


# ---- 3. and 4. against the fp64 autograd stack ------------------------------------------------------------------------------------
def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def internal_part(lay, flat):
    """The recurrent weights (and peepholes) of an LSTM layer's flat vector."""
    return flat[4 * lay.size * (lay.prev.size + 1):]


def distances(net, case, marked):
    loss, post, grads, errs = case.fp64(marked)
    real = real_mask(case.frac)
    e = forward_backward(net, case.frac)
    d = {"post": float(np.abs(net.outputs().reshape(-1, case.C)[real] - post).max()), "error": abs(e - loss) / max(1.0, abs(loss))}
    for lay in net.trainable_layers():
        d["grad/" + lay.name] = rel(lay.weight_updates(), grads[lay.name])
        if lay.type in ("lstm", "blstm"):
            d["grad_internal/" + lay.name] = rel(internal_part(lay, lay.weight_updates()), internal_part(lay, grads[lay.name]))
        if lay.name in errs:
            d["err/" + lay.name] = rel(lay.output_errors().reshape(case.N, -1)[real], errs[lay.name])
    return d


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide", "headline", "from_input"])
def test_parity_through_the_net(pkg, small, wide, headline, from_input, prec, which):
    """Posteriors, error, every gradient (the recurrent part of each LSTM layer also on its own: it is wrong by O(1) if K9 reads
    the sum instead of the branch) and every propagated error within DESIGN section 3's table.  f32 / bf16x3: the feature adds one
    fp32 addition per element, no new error source.  bf16: where the 3e-2 pin is not met the same net UNMARKED is measured
    against its own fp64 stack in the same run and the marked net is allowed twice that distance (activations up to twice as
    large carry twice the bf16 rounding)."""
    case = {"small": small, "wide": wide, "headline": headline, "from_input": from_input}[which]
    t_post, t_err, t_grad = TOL[prec]
    with case.net(pkg, prec) as net:
        d = distances(net, case, None)
    print(which, prec, "marked", {k: float("%.2g" % v) for k, v in d.items()})
    bound = {k: (t_post if k == "post" else t_err if k == "error" else t_grad) for k in d}
    if prec == "PREC_BF16" and any(d[k] >= bound[k] for k in d):
        with case.net(pkg, prec, marked=()) as net:
            d0 = distances(net, case, ())
        print(which, prec, "unmarked", {k: float("%.2g" % v) for k, v in d0.items()})
        bound = {k: max(bound[k], 2 * d0[k]) for k in d}
    assert all(d[k] < bound[k] or (k == "error" and d[k] <= bound[k]) for k in d), (d, bound)
    assert any(k.startswith("grad_internal/") for k in d)


# ---- 5. three armed steps with prefetch -----------------------------------------------------------------------------------------
LR, MOM = 1e-2, 0.9


def second_fraction(pkg, case, seed=5):
    rng = np.random.RandomState(seed)
    lens = list(reversed(case.lens))
    xs, ts = random_sequences(rng, lens, case.P, C=case.C)
    return lens, pkg.make_fraction(xs, ts, case.PS)


def fp64_three_steps(case, fracs_lens):
    w = flat_weights(case.weights)
    delta = {k: np.zeros_like(v) for k, v in w.items()}
    for step in range(3):
        lens, frac = fracs_lens[step % len(fracs_lens)]
        _, _, grads, _ = autograd_residual(case.layers, w, frac, lens, case.marked)
        for k in w:                                   # SteepestDescentOptimizer.cu:39-59
            delta[k] = MOM * delta[k] - LR * grads[k]
            w[k] = w[k] + delta[k]
    return w


def armed_steps(net, fracs):
    for step in range(3):
        net.load_sequences(fracs[step % len(fracs)])
        net.compute_forward_pass()
        if step + 1 < 3:
            net.prefetch_sequences(fracs[(step + 1) % len(fracs)])
        net.arm_update(LR, MOM)
        net.compute_backward_pass()
        net.update_weights_fused(LR, MOM)
    out = {l.name: l.weights() for l in net.trainable_layers()}
    assert net.prefetch_hits() == 2
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_three_armed_steps_with_prefetch(pkg, small, prec):
    """Deterministic mode, the armed fused update, the next fraction announced beside the backward pass: two runs end in the same
    bits, and in the weights of three momentum-SGD steps of the fp64 stack within the single-pass table's gradient column taken
    relative to the layer's largest weight (the form test_gpu_parity.py holds trained weights to)."""
    lens2, frac2 = second_fraction(pkg, small)
    want = fp64_three_steps(small, [(small.lens, small.frac), (lens2, frac2)])
    runs = []
    for _ in range(2):
        with small.net(pkg, prec, deterministic=True) as net:
            runs.append(armed_steps(net, [small.frac, frac2]))
    t = TOL[prec][2]
    w0 = flat_weights(small.weights)
    for name, w in runs[0].items():
        assert np.array_equal(bits(w), bits(runs[1][name])), (prec, name)
        d, moved = rel(w, want[name]), float(np.abs(want[name] - w0[name]).max())
        print(prec, name, "weights %.2g of their max; moved by %.2g" % (d, moved))
        assert d < t, (prec, name, d)
        assert moved > 1e-4


# ---- 6. off is the old path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
def test_off_is_the_old_path(pkg, wide, prec):
    """"residual": false on every layer that may carry the member against descriptions without it: bit-equal weights after three
    steps, and the same number of timed spans in every kernel class.  (The marked net differs in both: the check can tell.)"""
    _, frac2 = second_fraction(pkg, wide)

    def run(layers):
        with pkg.NeuralNetwork(layers, wide.weights, wide.PS, wide.T, precision=getattr(pkg, prec), deterministic=True) as net:
            w = armed_steps(net, [wide.frac, frac2])
            net.timing_enable(True); net.timing_reset()
            forward_backward(net, wide.frac)
            net.update_weights(LR, MOM)
            counts = {k: v[1] for k, v in net.timing_read().items()}
            net.timing_enable(False)
            return w, counts
    absent, absent_n = run(wide.layers)
    off, off_n = run(wide.desc(marked=()))
    assert any(d.get("residual") is False for d in wide.desc(marked=())) and all("residual" not in d for d in wide.layers)
    assert off_n == absent_n
    for name in absent:
        assert np.array_equal(bits(off[name]), bits(absent[name])), (prec, name)
    on, on_n = run(wide.desc())
    assert on_n["other"] > absent_n["other"] and {k: v for k, v in on_n.items() if k != "other"} == {k: v for k, v in absent_n.items() if k != "other"}
    assert all(not np.array_equal(on[name], absent[name]) for name in absent)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def test_errors(pkg, small):
    BAD_ARG, STATE = -1, -4
    with small.net(pkg, "PREC_F32", marked=("blstm_1",)) as net:
        lib = net.lib
        for name, text in (("input", b"only lstm, blstm and feedforward"), ("output", b"only lstm, blstm and feedforward"),
                           ("postoutput", b"only lstm, blstm and feedforward"), ("lstm_0", b"size of its preceding layer")):
            assert lib.cn_layer_set_residual(net.layer(name).handle, 1) == BAD_ARG, name
            assert text in lib.cn_last_error(net.ctx), (name, lib.cn_last_error(net.ctx))
        # a post output layer created behind a marked layer, and a layer marked in front of one
        ff = C.c_void_p()
        assert lib.cn_layer_create(net.ctx, pkg.LAYER_KINDS["feedforward_identity"], net.layer("lstm_3").handle, 10, 1.0, 0, 0, C.byref(ff)) == 0
        assert lib.cn_layer_set_residual(ff, 1) == 0
        post = C.c_void_p()
        assert lib.cn_layer_create(net.ctx, pkg.LAYER_KINDS["sse"], ff, 10, 0.0, 0, 0, C.byref(post)) == BAD_ARG
        assert b"post output layer directly after a residual layer" in lib.cn_last_error(net.ctx)
        assert lib.cn_layer_set_residual(ff, 0) == 0
        assert lib.cn_layer_create(net.ctx, pkg.LAYER_KINDS["sse"], ff, 10, 0.0, 0, 0, C.byref(post)) == 0
        assert lib.cn_layer_set_residual(ff, 1) == BAD_ARG
        assert b"in front of a post output layer" in lib.cn_last_error(net.ctx)
    with small.net(pkg, "PREC_F32", marked=("blstm_1",)) as net:
        # the refused calls changed nothing; an unmarked layer has no branch to report; unmarking takes a layer off the path again
        forward_backward(net, small.frac)
        assert net.layer("blstm_1").residual and not net.layer("lstm_3").residual
        net.layer("blstm_1").residual_branch()
        for name in ("lstm_0", "feedforward_tanh_2", "lstm_3", "output"):
            with pytest.raises(pkg.CurrenntHipError) as ei:
                net.layer(name).residual_branch()
            assert ei.value.code == STATE, name
        net.layer("blstm_1").set_residual(False)
        forward_backward(net, small.frac)
        with pytest.raises(pkg.CurrenntHipError) as ei:
            net.layer("blstm_1").residual_branch()
        assert ei.value.code == STATE
    # the Python mirror refuses a description as the C++ driver does (tests/test_driver_residual.py), with the same texts
    for name, text in (("input", "only lstm, blstm and feedforward"), ("output", "only lstm, blstm and feedforward"),
                       ("postoutput", "only lstm, blstm and feedforward"), ("lstm_0", "size 10 differs from the preceding layer's size 7")):
        with pytest.raises(RuntimeError, match="Invalid value 'residual' in layer '%s': .*%s" % (name, text)):
            small.net(pkg, "PREC_F32", marked=(name,))
    layers = net_desc(7, [("lstm", 7)], 7, post="sse")
    layers[2]["residual"] = True                     # (the output layer of an sse net is feedforward_identity)
    with pytest.raises(RuntimeError, match="Invalid value 'residual' in layer 'output': a post output layer cannot follow a residual layer directly"):
        pkg.NeuralNetwork(layers, None, 2, 4, seed=1)
