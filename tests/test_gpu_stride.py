"""-m gpu: strided context layers (include/currennt_hip.h, section Strided context layers).  The gather, the derived time axis and
the fold are held bit for bit to the restated rule (tests/stride_reference.py), a strided layer behind the input layer to what
input splicing with a frame skip produces, a stride of 1 to the plain context layer, the step through the nets to the fp64
autograd stack with rate changes; then fractions of different lengths in sequence with a prefetch hit between them, the armed
updates, the other input features behind a strided layer, the ctc, sse and multiclass post layers on the reduced axis, and the
errors."""
import copy
import ctypes as C

import numpy as np
import pytest

import context_reference as cref
import post_reference as pr
from ctc_reference import ctc_fraction
from dropout_reference import bf16_round, keep, scale
from helpers import random_weights
from stride_reference import (Case, derived_pattern_types, derived_targets, stack_results, stride_net_desc, strided_backward,
                              strided_forward, unread_frames)
from test_gpu_ctc import bound as ctc_bound
from test_gpu_dropout import TOL

pytestmark = pytest.mark.gpu

PRECS = ["PREC_F32", "PREC_BF16X3", "PREC_BF16"]
STATE, BAD_ARG, SHAPE = -4, -1, -2


@pytest.fixture(scope="module")
def case_of(pkg):
    cache = {}

    def get(which, **kw):
        key = (which, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in cache:
            cache[key] = Case(pkg, which, **kw)
        return cache[key]
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


def strided_layers(net):
    return [l for l in net.layers if l.type == "context"]


def members(lay):
    return lay.context() + (lay.stride(),)


# ---- 1. the gather and the derived axis ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide", "from_input"])
def test_forward_and_axis_bit_for_bit(pkg, case_of, prec, which):
    case = case_of(which)
    tc = case.frac["targetClasses"].reshape(case.T, case.PS)
    with case.net(pkg, prec) as net:
        net.load_sequences(case.frac)
        net.compute_forward_pass()
        assert len(strided_layers(net)) == sum(t == "context" for t, _ in case.hidden)
        pads = set()
        for lay in strided_layers(net):
            L, R, D, S = members(lay)
            assert (L, R, D, S) == tuple(lay.desc[k] for k in ("left", "right", "dilation", "stride")) and S > 1
            Tp, lens_p, rate_p = case.axes[lay.prev.name]
            Tn, lens_n, rate_n = case.axes[lay.name]
            assert lay.time() == (Tn, -(-case.frac["Tmin"] // rate_n), rate_n) and rate_n == rate_p * S
            assert list(net.lengths(lay)[:len(case.lens)]) == lens_n
            x = lay.prev.outputs()
            assert x.shape == (Tp, case.PS, lay.prev.size)
            if prec == "PREC_BF16":
                x = bf16_round(x)      # (a feed-forward predecessor reports its fp32 outputs; its operand copy is their bf16 rounding)
            want = strided_forward(x, lens_p, L, R, D, S)
            got = lay.outputs()
            assert got.shape == want.shape == (Tn, case.PS, lay.size)
            assert np.array_equal(bits(got), bits(want)), (prec, lay.name, int((bits(got) != bits(want)).sum()))
            real = case.real(lay.name)
            assert (~real).any() and np.all(bits(got.reshape(Tn * case.PS, -1)[~real]) == 0) and np.abs(got).max() > 0     # rows behind n_s
            # the pad columns (size .. Lp - 1) and the pad slots of the padded rows, which outputs() does not return
            assert lay.pad_bits() == 0
            pads.add(lay.size % 32 != 0)
            # the axis as the device holds it: pattern types, classes, lengths; pad slots NONE / -1 / 0
            pat, cls, ln = net.axis(lay)
            PSp = pat.shape[1]
            assert PSp % 4 == 0 and PSp >= case.PS and pat.shape == (Tn, PSp)
            assert np.array_equal(pat[:, :case.PS], derived_pattern_types(case.lens, case.T, case.PS, rate_n))
            assert np.array_equal(cls[:, :case.PS], derived_targets(tc, case.lens, rate_n))
            assert np.all(pat[:, case.PS:] == 0) and np.all(cls[:, case.PS:] == -1)
            assert list(ln[:len(case.lens)]) == lens_n and not ln[len(case.lens):].any()
            # a follower's rows: as many as the axis has
            assert net.layers[net.layers.index(lay) + 1].outputs().shape[0] == Tn
        assert (True in pads) == (which != "wide")                                            # (small and from_input have layers with pad columns)


# ---- 2. the fold ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_backward_bit_for_bit(pkg, case_of, prec, which):
    case = case_of(which)
    rng = np.random.RandomState(6)
    with case.net(pkg, prec) as net:
        net.load_sequences(case.frac)
        net.compute_forward_pass()
        n_unread = 0
        for lay in strided_layers(net):
            L, R, D, S = members(lay)
            Tp, lens_p, _ = case.axes[lay.prev.name]
            Tn, _, _ = case.axes[lay.name]
            e = (rng.randn(Tn, case.PS, lay.size) + 0.5).astype(np.float32)
            assert np.all(e != 0)                                                              # (non-zero on dummy rows: they are not read)
            lay.write_output_errors(e)
            lay.backward()
            want = strided_backward(e, lens_p, Tp, L, R, D, S)
            got = lay.prev.output_errors()
            assert got.shape == want.shape
            assert np.array_equal(bits(got), bits(want)), (prec, lay.name, int((bits(got) != bits(want)).sum()), float(np.abs(got - want).max()))
            unread = unread_frames(lens_p, Tp, case.PS, L, R, D, S)
            real = case.real(lay.prev.name).reshape(Tp, case.PS)
            assert np.all(bits(got[unread]) == 0) and np.all(bits(got[~real]) == 0) and np.all(got[real & ~unread] != 0)
            n_unread += int(unread.sum())
        assert which != "wide" or n_unread > 0


# ---- 3. behind the input layer: input splicing with a frame skip ----------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_behind_the_input_layer_is_input_splicing_with_a_skip(pkg, case_of, prec):
    case = case_of("from_input")
    t_post, t_err, t_grad = TOL[prec]
    real = case.real("output")
    spliced = copy.deepcopy([d for d in case.layers if d["type"] != "context"])
    spliced[0]["size"] = 6 * case.P
    with case.net(pkg, prec) as net, pkg.NeuralNetwork(spliced, case.weights, case.PS, case.T, precision=getattr(pkg, prec)) as ref:
        ref.set_input_splice(context=(2, 3), frame_skip=2)
        e, e_ref = forward_backward(net, case.frac), forward_backward(ref, case.frac)
        got, want = net.layer("context_0").outputs(), ref.input_layer().outputs()
        assert got.shape == want.shape == (4, case.PS, 6 * case.P) and np.array_equal(bits(got), bits(want)) and np.abs(want).max() > 0
        d = {"post": float(np.abs(net.outputs().reshape(-1, case.C)[real] - ref.outputs().reshape(-1, case.C)[real]).max()),
             "error": abs(e - e_ref) / max(1.0, abs(e_ref))}
        for lay in net.trainable_layers():
            d["grad/" + lay.name] = rel(lay.weight_updates(), ref.layer(lay.name).weight_updates())
    print(prec, d)
    assert d["post"] < t_post and d["error"] <= t_err and all(v < t_grad for k, v in d.items() if k.startswith("grad")), d


# ---- 4. a stride of 1 is the plain context layer -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_stride_one_is_the_plain_layer(pkg, prec):
    case = cref.Case(pkg, "small")
    with_member = copy.deepcopy(case.layers)
    for d in with_member:
        if d["type"] == "context":
            d["stride"] = 1
    runs = []
    for layers in (case.layers, with_member):
        with case.net(pkg, prec, layers=layers, deterministic=True) as net:
            out = {}
            for step in range(3):
                forward_backward(net, case.frac)
                if step == 0:
                    out.update({"out/" + l.name: l.outputs() for l in net.layers[:-1]})
                    out.update({"err/" + l.name: l.output_errors() for l in net.layers[1:-1]})
                    out.update({"grad/" + l.name: l.weight_updates() for l in net.trainable_layers()})
                net.update_weights_fused(1e-2, 0.9)
            out.update({"w/" + l.name: l.weights() for l in net.trainable_layers()})
            names = (net.recurrent_kernel(False), net.recurrent_kernel(True))
            assert all(l.stride() == 1 and l.time() == (case.T, case.frac["Tmin"], 1) for l in net.layers if l.type == "context")
            runs.append((out, names))
    assert runs[0][1] == runs[1][1] and all(runs[0][1])
    for k, v in runs[0][0].items():
        assert np.array_equal(bits(v), bits(runs[1][0][k])) and np.abs(v).max() > 0, (prec, k)


# ---- 5. the step through the nets ----------------------------------------------------------------------------------------------------------
def distances(net, case, want):
    loss, post, grads, errs = want
    e = forward_backward(net, case.frac)
    real = case.real("output")
    d = {"post": float(np.abs(net.outputs().reshape(-1, case.C)[real] - post).max()), "error": abs(e - loss) / max(1.0, abs(loss))}
    for lay in net.layers[1:-2]:
        if lay.trainable:
            d["grad/" + lay.name] = rel(lay.weight_updates(), grads[lay.name])
        if lay.trainable or lay.prev.type != "input":                                      # (a context layer behind the input layer takes no errors)
            d["err/" + lay.name] = rel(lay.output_errors().reshape(-1, lay.size)[case.real(lay.name)], errs[lay.name])
    d["grad/output"] = rel(net.output_layer().weight_updates(), grads["output"])
    return d


def assert_inside(d, prec):
    t_post, t_err, t_grad = TOL[prec]
    assert d["post"] < t_post and d["error"] <= t_err, d
    assert all(v < t_grad for k, v in d.items() if k[:4] in ("grad", "err/")), d


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_parity_through_the_net(pkg, case_of, prec, which):
    """Loss, posteriors on the output axis's real frames, every gradient and the errors handed to every layer against the fp64
    autograd stack, within the project's table for a step through a small net (TOL of tests/test_gpu_dropout.py)."""
    case = case_of(which)
    with case.net(pkg, prec) as net:
        d = distances(net, case, case.reference())
    print(which, prec, {k: float("%.2g" % v) for k, v in d.items()})
    assert sum(k.startswith("err/") for k in d) == len(case.hidden)
    assert_inside(d, prec)


# ---- 6. fractions in sequence ---------------------------------------------------------------------------------------------------------------
def one_pass(net, case, prefetch=None):
    net.load_sequences(case.frac)
    net.compute_forward_pass()
    e, c = net.error_and_correct()
    if prefetch is not None:
        net.prefetch_sequences(prefetch.frac)
    net.compute_backward_pass()
    out = {"error": np.float32(e), "correct": np.float32(c)}
    out.update({"out/" + l.name: l.outputs() for l in net.layers[:-1]})
    out.update({"err/" + l.name: l.output_errors() for l in net.layers[1:-1] if l.trainable or l.prev.type != "input"})
    out.update({"grad/" + l.name: l.weight_updates() for l in net.trainable_layers()})
    out["time"] = [l.time() for l in net.layers]
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_long_short_long_with_a_prefetch_hit(pkg, case_of, prec):
    long_, short = case_of("small"), case_of("small", lens=[5, 2, 4], seed=77)
    assert short.T < long_.T and short.axes["output"][0] < long_.axes["output"][0]
    with long_.net(pkg, prec, deterministic=True) as net:
        got = [one_pass(net, long_, prefetch=short), one_pass(net, short), one_pass(net, long_)]
        assert net.prefetch_hits() == 1
    for case, g in zip((long_, short, long_), got):
        with long_.net(pkg, prec, deterministic=True) as fresh:
            want = one_pass(fresh, case)
        assert g["time"] == want["time"] == [(case.axes[d["name"]][0], -(-case.frac["Tmin"] // case.axes[d["name"]][2]), case.axes[d["name"]][2])
                                             for d in case.layers]
        for k, v in want.items():
            if k != "time":
                assert np.shape(g[k]) == np.shape(v) and np.array_equal(bits(g[k]), bits(v)), (prec, case.lens, k)


# ---- 7. armed updates; the other input features ------------------------------------------------------------------------------------------------
LR, MOM = 1e-2, 0.9


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rule", ["momentum", "adam"])
def test_armed_updates_run_twice_give_the_same_weights(pkg, case_of, rule, prec):
    fracs = [case_of("small"), case_of("small", lens=[5, 2, 4], seed=77)]

    def run():
        with fracs[0].net(pkg, prec, deterministic=True) as net:
            for step in range(3):
                net.load_sequences(fracs[step % 2].frac)
                net.compute_forward_pass()
                if step + 1 < 3:
                    net.prefetch_sequences(fracs[(step + 1) % 2].frac)
                if rule == "adam":
                    net.arm_adam(LR, step=step + 1)
                else:
                    net.arm_update(LR, MOM)
                net.compute_backward_pass()
                if rule == "adam":
                    net.update_weights_adam(LR, step=step + 1)
                else:
                    net.update_weights_fused(LR, MOM)
            assert net.prefetch_hits() == 2
            return {l.name: l.weights() for l in net.trainable_layers()}
    a, b = run(), run()
    w0 = cref.flat_weights(fracs[0].weights)
    for name, w in a.items():
        assert np.array_equal(bits(w), bits(b[name])), (rule, prec, name)
        assert np.abs(w - w0[name]).max() > 1e-4 and np.isfinite(w).all()


SEED, PASS = 0x2468ACE, 3


@pytest.mark.parametrize("prec", PRECS)
def test_follower_drops_normalises_and_is_residual(pkg, case_of, prec):
    """blstm 6 -> context(1, 1, x1, /2) -> feedforward_tanh 18 with dropout 0.2, layer_norm and residual: the masks are keyed by the
    follower's own frame index n = j * PS + ps of the reduced axis."""
    case = case_of("features")
    name, rate = "feedforward_tanh_2", 0.2
    desc = copy.deepcopy(case.layers)
    idx = [d["name"] for d in desc].index(name)
    desc[idx].update({"dropout": rate, "layer_norm": True, "residual": True})
    assert desc[idx - 1]["type"] == "context" and desc[idx - 1]["stride"] == 2 and desc[idx - 1]["size"] == desc[idx]["size"] == 18
    Tn = case.axes[name][0]
    mask = keep(SEED, idx, PASS, Tn * case.PS, 18, rate)
    want = stack_results(case.layers, case.weights, case.frac, case.lens, normed=(name,), marked=(name,), drop={name: (mask, scale(rate))})
    with case.net(pkg, prec, layers=desc) as net:
        net.set_dropout_pass(1, SEED, PASS)
        d = distances(net, case, want)
        lay = net.layer(name)
        assert lay.residual and lay.layer_norm and lay.dropout_input().shape == (Tn, case.PS, 18)
        assert np.all(lay.dropout_input().reshape(Tn * case.PS, -1)[~mask] == 0)
    print(prec, {k: float("%.2g" % v) for k, v in d.items()})
    assert_inside(d, prec)


# ---- 8. ctc on the reduced axis -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_ctc_on_the_reduced_axis(pkg, case_of, prec):
    case = case_of("small")
    layers = copy.deepcopy(case.layers)
    layers[-1]["type"] = "ctc"
    Tn, lens_n, rate = case.axes["output"]
    assert lens_n == [3, 1, 1]
    labels = [[1, 2], [0], [3, 3]]                                      # the last: 2 labels + 1 repeat = 3 frames needed, 1 there
    frac = pkg.make_fraction(case.xs, None, case.PS, labels=labels)
    with case.net(pkg, prec, layers=layers) as net:
        net.load_sequences(frac)
        net.compute_forward_pass()
        err, count = net.error_and_correct()
        y = net.outputs()
        assert y.shape == (Tn, case.PS, case.C)
        pat = derived_pattern_types(case.lens, case.T, case.PS, rate)
        l64, g64, ok = ctc_fraction(y, pat, labels, np.float64)
        l32, g32, _ = ctc_fraction(y, pat, labels, np.float32)
        assert list(ok) == [True, True, False] and count == 2
        d_ref = abs(float(l32.sum()) - l64.sum()) / l64.sum()
        print("%s: error %.8g model %.8g rel %.3g ref %.3g" % (prec, err, l64.sum(), abs(err - l64.sum()) / l64.sum(), d_ref))
        assert abs(err - l64.sum()) / l64.sum() <= ctc_bound(d_ref)
        net.post_output_layer().backward()
        oe = net.output_layer().output_errors()
        y64 = y.astype(np.float64)
        d_gpu, d_ref = np.abs(y64 * oe - y64 * g64).max(), np.abs(y64 * g32 - y64 * g64).max()
        print("%s: y*dL/dy gpu %.3g ref %.3g" % (prec, d_gpu, d_ref))
        assert d_gpu <= ctc_bound(d_ref)
        assert not oe[pat == 0].any() and not oe[:, 2].any() and oe[:, :2].any()      # the over-long sequence contributes 0
        net.compute_backward_pass()
        assert all(np.isfinite(l.weight_updates()).all() and np.abs(l.weight_updates()).max() > 0 for l in net.trainable_layers())


# ---- 9. sse and multiclass on the reduced axis ----------------------------------------------------------------------------------------------------
def inside(tag, got, want, bound):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    slack = np.abs(got - want) - bound
    assert np.all(slack <= 0), (tag, float(np.max(slack)), float(np.max(np.abs(got - want))))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("post", ["sse", "multiclass_classification"])
def test_post_layers_count_the_reduced_frames(pkg, case_of, post, prec):
    """The error, #correct and the injected errors against tests/post_reference.py at the outputs as read, with the targets and
    pattern types of the reduced axis (derived_targets, derived_pattern_types): five frames, not the input's twenty."""
    case = case_of("small")
    Tn, lens_n, rate = case.axes["output"]
    rng = np.random.RandomState(9)
    if post == "sse":
        layers = stride_net_desc(case.P, case.hidden, case.C, post="sse", out_type="feedforward_identity")
        ts = [rng.uniform(-1, 1, (n, case.C)).astype(np.float32) for n in case.lens]
        frac = pkg.make_fraction(case.xs, ts, case.PS, classification=False)
        tg = derived_targets(frac["targets"].reshape(case.T, case.PS, case.C), case.lens, rate).reshape(Tn * case.PS, case.C)
        weights = random_weights(layers, np.random.RandomState(3), 0.3)
    else:
        layers, weights, frac = case.layers, case.weights, case.frac
        tg = derived_targets(frac["targetClasses"].reshape(case.T, case.PS), case.lens, rate).reshape(-1)
    pat = derived_pattern_types(case.lens, case.T, case.PS, rate).reshape(-1)
    assert int((pat != 0).sum()) == sum(lens_n) == 5
    with case.net(pkg, prec, layers=layers, weights=weights) as net:
        net.load_sequences(frac)
        net.compute_forward_pass()
        y = net.outputs().reshape(Tn * case.PS, case.C)
        e, c = net.error_and_correct()
        want, bound = pr.error(post, y, tg, pat, depth=pr.loss_depth(case.C, Tn * 4))
        inside(post + " error", e, want, bound)
        assert c == pr.correct(post, y, tg, pat) and want > 0
        # the running sums count the same frames
        net.loss_accumulate()
        e2, c2 = net.loss_read()
        inside(post + " accumulated", e2, want, bound)
        assert c2 == max(c, 0) or post == "sse"
        net.post_output_layer().backward()
        if post == "sse":
            inj = net.output_layer().output_errors().reshape(-1, case.C)
            wi, bi = pr.inject(post, y, tg, pat)
            inside(post + " injected", inj, wi, bi)
            assert np.all(inj[pat == 0] == 0) and np.all(inj[pat != 0] != 0)
        net.compute_backward_pass()
        oe = net.output_layer().output_errors().reshape(-1, case.C)
        assert np.all(oe[pat == 0] == 0) and np.abs(oe[pat != 0]).max() > 0


# ---- 10. errors -------------------------------------------------------------------------------------------------------------------------------------
def test_axis_hook_without_slot_lengths_is_refused(pkg):
    """cn_dbg_layer_axis asked for the slot lengths of a net without a context layer (the context then has no such table): refused
    with CN_ERR_STATE in front of the length pass; the pattern types and classes of the base axis are there all the same."""
    layers = [{"name": "in", "type": "input", "size": 3}, {"name": "l", "type": "lstm", "size": 4, "bias": 1.0},
              {"name": "out", "type": "softmax", "size": 3, "bias": 1.0}, {"name": "post", "type": "multiclass_classification", "size": 3}]
    rng = np.random.RandomState(2)
    lens = [4, 2]
    frac = pkg.make_fraction([rng.randn(n, 3).astype(np.float32) for n in lens], [rng.randint(0, 3, n).astype(np.int32) for n in lens], 2)
    with pkg.NeuralNetwork(layers, None, 2, 4, seed=1) as net:
        net.load_sequences(frac)
        ln = np.full(64, -7, np.int32)
        assert net.lib.cn_dbg_layer_axis(net.layer("l").handle, None, None, ln.ctypes.data_as(C.c_void_p), 0, None) == STATE
        assert b"no slot lengths" in net.lib.cn_last_error(net.ctx) and np.all(ln == -7)
        pat, cls, none = net.axis("l")
        assert none is None and np.array_equal(pat[:, :2], frac["patTypes"].reshape(4, 2)) and np.all(pat[:, 2:] == 0)
        assert np.array_equal(cls[:, :2], frac["targetClasses"].reshape(4, 2))
        net.compute_forward_pass()
        assert np.isfinite(net.calculate_error())
        assert list(net.lengths()) == lens and net.layer("out").time() == (4, 2, 1)


@pytest.mark.parametrize("prec", PRECS)
def test_errors(pkg, case_of, prec):
    case = case_of("small")
    with case.net(pkg, prec) as net:
        lib, prev = net.lib, net.layer("lstm_0")
        h = C.c_void_p()
        for stride in (0, 9, -1):
            assert lib.cn_layer_create_context_strided(net.ctx, prev.handle, 1, 1, 1, stride, C.byref(h)) == BAD_ARG and not h.value, stride
            assert b"stride must lie in 1..8" in lib.cn_last_error(net.ctx)
        s = C.c_int()
        assert lib.cn_layer_context_stride(prev.handle, C.byref(s)) == BAD_ARG
        assert lib.cn_layer_context_stride(net.layer("context_3").handle, C.byref(s)) == 0 and s.value == 3
        t = C.c_int()
        assert lib.cn_layer_time(net.layer("output").handle, C.byref(t), None, None) == STATE          # before a load
        with pytest.raises(pkg.CurrenntHipError) as ei:
            prev.stride()
        assert ei.value.code == BAD_ARG
        # a downstream forward pass before the strided layer's of this fraction
        net.load_sequences(case.frac)
        assert net.layer("output").time() == (3, 1, 6)                                               # (host arithmetic: no forward pass needed)
        net.layer("lstm_0").forward()
        with pytest.raises(pkg.CurrenntHipError) as ei:
            net.layer("blstm_2").forward()
        assert ei.value.code == STATE and "strided context layer" in str(ei.value)
        for call in (net.layer("blstm_2").outputs, net.layer("blstm_2").backward, net.error_and_correct, net.loss_accumulate):
            with pytest.raises(pkg.CurrenntHipError) as ei:
                call()
            assert ei.value.code == STATE, call
        net.compute_forward_pass()
        net.error_and_correct()
        # a new load makes the axes stale again
        net.load_sequences(case.frac)
        with pytest.raises(pkg.CurrenntHipError) as ei:
            net.layer("output").forward()
        assert ei.value.code == STATE
        net.compute_forward_pass()
        # a read-back or errors with the parent's row count
        lay = net.layer("blstm_2")
        buf = np.zeros(case.T * case.PS * lay.size, np.float32)
        assert lib.cn_layer_read(lay.handle, pkg.binding.BUF["outputs"], 0, buf.ctypes.data_as(C.c_void_p), buf.size) == SHAPE
        assert lib.cn_layer_write_output_errors(lay.handle, buf.ctypes.data_as(C.c_void_p), buf.size) == SHAPE
        n = case.axes["blstm_2"][0] * case.PS * lay.size
        assert lib.cn_layer_read(lay.handle, pkg.binding.BUF["outputs"], 0, buf.ctypes.data_as(C.c_void_p), n) == 0
    # the mirror: a stride out of range comes back with the library's code, a stride that is no integer with the driver's text
    for value in (0, 9):
        desc = copy.deepcopy(case.layers)
        desc[2]["stride"] = value
        with pytest.raises(pkg.CurrenntHipError) as ei:
            case.net(pkg, prec, layers=desc)
        assert ei.value.code == BAD_ARG, value
    for value in (2.5, True):
        desc = copy.deepcopy(case.layers)
        desc[2]["stride"] = value
        with pytest.raises(RuntimeError, match="Invalid value 'stride' in layer 'context_1': an integer expected"):
            case.net(pkg, prec, layers=desc)
    # a post output layer directly behind a strided layer stays refused
    layers = [{"name": "in", "type": "input", "size": 3}, {"name": "l", "type": "lstm", "size": 4, "bias": 1.0},
              {"name": "c", "type": "context", "size": 4, "stride": 2}, {"name": "post", "type": "sse", "size": 4}]
    with pytest.raises(pkg.CurrenntHipError) as ei:
        pkg.NeuralNetwork(layers, None, 2, 4, seed=1)
    assert ei.value.code == BAD_ARG and "trainable preceding layer" in str(ei.value)
