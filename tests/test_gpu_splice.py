"""-m gpu: input splicing and frame skipping on the device (cn_ctx_set_input_splice) against the host path of the same rule: a net
that loads the source-rate fraction with the setting on and a net with the same weights that loads the network-rate fraction the
numpy restatement (tests/splice_reference.py) builds must leave the same bytes everywhere.  Every comparison is bit equality; the
one bounded comparison (noise under a skip) uses the bound tests/augment_reference.py derives.

The shapes are the smallest at which the gather can go wrong: 5 features per frame, 5 slots (padded to more on the device) holding
sequences of 12, 8, 2 and 1 frames and an empty one, 12 source steps, contexts (0, 0), (1, 2), (2, 0) and skips 1, 2, 3 in front
of lstm 7 -> softmax 4: a length the skip divides, ragged last groups where the gather clamps at the last frame, one network frame
from 2 frames and from 1, K > B (frames never read) and K < B."""
import numpy as np
import pytest

import augment_reference as AR
import splice_reference as SR
from helpers import net_desc, random_sequences, random_weights

pytestmark = pytest.mark.gpu
PRECS = ["PREC_F32", "PREC_BF16", "PREC_BF16X3"]
P0, C, PS, T = 5, 4, 5, 12
LENGTHS = [12, 8, 2, 1]
SHORTER = [5, 7, 1]
CONTEXTS = [(0, 0), (1, 2), (2, 0)]
SKIPS = [1, 2, 3]
SEED = 0x0123456789ABCDEF
LR, MOM = 1e-2, 0.9
BAD_ARG, SHAPE = -1, -2


def layers_of(context, post="multiclass_classification"):
    return net_desc(P0 * (context[0] + context[1] + 1), [("lstm", 7)], C, post=post)


def network(pkg, prec="PREC_F32", context=(0, 0), options=None, post="multiclass_classification", max_seq_length=T):
    layers = layers_of(context, post)
    return pkg.NeuralNetwork(layers, random_weights(layers, np.random.RandomState(77), 0.3), PS, max_seq_length, precision=getattr(pkg, prec),
                             deterministic=True, options=options)


def contiguous(fr):
    """the arrays a prefetch and its load both hand over (a hint is matched by address)"""
    fr["inputs"] = np.ascontiguousarray(fr["inputs"], np.float32); fr["patTypes"] = np.ascontiguousarray(fr["patTypes"], np.int8)
    if "targetClasses" in fr:
        fr["targetClasses"] = np.ascontiguousarray(fr["targetClasses"], np.int32)
    return fr


def source(pkg, k=0, lengths=LENGTHS, classes=True):
    """source-rate fraction k, built without context"""
    xs, ts = random_sequences(np.random.RandomState(3000 + k), lengths, P0, C=C) if classes else \
        random_sequences(np.random.RandomState(3000 + k), lengths, P0, L=C)
    return contiguous(pkg.make_fraction(xs, ts, PS, classification=classes))


def resident(torch, fr):
    """the fraction in HBM: (descriptor for load_sequences_resident, the tensors that own the memory)"""
    dev = {k: torch.from_numpy(fr[k]).cuda() for k in ("inputs", "patTypes", "targetClasses")}
    d = {"T": fr["T"], "Tmin": fr["Tmin"], "numSeqs": fr["numSeqs"], "inputPatternSize": fr["inputs"].shape[-1], "outputPatternSize": C}
    d.update({k: v.data_ptr() for k, v in dev.items()})
    return d, dev


def forward_state(net):
    """what a load and a forward pass leave, as bytes"""
    net.compute_forward_pass()
    return {"T": (net.T, net.Tmin), "inputs": net.input_layer().outputs().tobytes(), "posteriors": net.outputs().tobytes(),
            "error": net.error_and_correct(), "rows": net.row_map_counts()}


def train_state(net):
    net.compute_backward_pass()
    out = {"updates " + l.name: l.weight_updates().tobytes() for l in net.trainable_layers()}
    net.update_weights(LR, MOM)
    out.update({"weights " + l.name: l.weights().tobytes() for l in net.trainable_layers()})
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], (what, k)


@pytest.mark.parametrize("context", CONTEXTS)
@pytest.mark.parametrize("prec", PRECS)
def test_forward_loss_and_one_update_equal_the_host_path(pkg, prec, context):
    """every skip, on two fractions loaded one after the other into the same two nets"""
    for k in SKIPS:
        with network(pkg, prec, context) as a, network(pkg, prec, context) as b:
            a.set_input_splice(context, k)
            for n, lengths in enumerate((LENGTHS, SHORTER)):
                src = source(pkg, n, lengths)
                want = SR.network_fraction(src, context, k)
                a.load_sequences(src); b.load_sequences(want)
                fa, fb = forward_state(a), forward_state(b)
                assert fa["T"] == (want["T"], want["Tmin"]) and a.input_layer().outputs().shape == (want["T"], PS, P0 * sum(context) + P0)
                assert fb["inputs"] == (AR.bf16_round(want["inputs"]) if prec == "PREC_BF16" else want["inputs"]).tobytes()
                assert_same(fa, fb, (k, n))
                assert_same(train_state(a), train_state(b), (k, n))


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
def test_every_load_path_gives_the_same_bytes(pkg, prec):
    """context (1, 2), K = 2: staged host load, resident load, option overlap = 0, and a host and a resident prefetch whose load
    is a hit"""
    import torch
    context, k = (1, 2), 2
    src, other = source(pkg, 0), source(pkg, 1, [7, 12, 3, 5])
    d, keep = resident(torch, src)
    d_other, keep_other = resident(torch, other)
    with network(pkg, prec, context) as net:
        net.load_sequences(contiguous(SR.network_fraction(src, context, k)))
        want = forward_state(net)
    got = {}
    with network(pkg, prec, context) as net:
        net.set_input_splice(context, k)
        net.load_sequences(src)
        got["host"] = forward_state(net)
        net.load_sequences_resident(d)
        got["resident"] = forward_state(net)
    with network(pkg, prec, context, options={"overlap": 0}) as net:
        net.set_input_splice(context, k)
        net.load_sequences(src)
        got["overlap = 0"] = forward_state(net)
    for kind in ("host", "resident"):
        with network(pkg, prec, context) as net:
            net.set_input_splice(context, k)
            if kind == "host":
                net.load_sequences(other); net.compute_forward_pass(); net.prefetch_sequences(src)
            else:
                net.load_sequences_resident(d_other); net.compute_forward_pass(); net.prefetch_sequences_resident(d)
            net.compute_backward_pass()
            assert net.prefetch_hits() == 0
            net.load_sequences(src) if kind == "host" else net.load_sequences_resident(d)
            assert net.prefetch_hits() == 1, kind
            got[kind + " prefetch"] = forward_state(net)
    for name, v in got.items():
        assert_same(v, want, name)


@pytest.mark.parametrize("kind", ["host", "resident"])
def test_a_prefetch_under_another_splice_setting_is_a_miss(pkg, kind):
    """the prefetch records the setting in force when it is announced; a load under another one discards it and leaves what its
    own setting prescribes"""
    import torch
    src, other = source(pkg, 0), source(pkg, 1, [7, 12, 3, 5])
    d, keep = resident(torch, src)
    d_other, keep_other = resident(torch, other)
    at_prefetch = ((1, 2), 2)
    for at_load in (((1, 2), 3), ((2, 1), 2)):
        with network(pkg, context=(1, 2)) as net:
            net.load_sequences(contiguous(SR.network_fraction(src, *at_load)))
            want = forward_state(net)
        with network(pkg, context=(1, 2)) as net:
            net.set_input_splice(*at_prefetch)
            if kind == "host":
                net.load_sequences(other); net.compute_forward_pass(); net.prefetch_sequences(src)
            else:
                net.load_sequences_resident(d_other); net.compute_forward_pass(); net.prefetch_sequences_resident(d)
            net.compute_backward_pass()
            net.set_input_splice(*at_load)
            net.load_sequences(src) if kind == "host" else net.load_sequences_resident(d)
            assert net.prefetch_hits() == 0
            assert_same(forward_state(net), want, at_load)


@pytest.mark.parametrize("k", SKIPS)
def test_an_sse_layer_takes_the_target_rows_of_source_row_k_j(pkg, k):
    src = source(pkg, 0, classes=False)
    want = SR.network_fraction(src, (1, 2), k)
    assert want["targets"].tobytes() == src["targets"].reshape(T, PS, C)[::k].tobytes() and want["targets"].any()
    states = []
    for spliced in (True, False):
        with network(pkg, context=(1, 2), post="sse") as net:
            if spliced:
                net.set_input_splice((1, 2), k)
            net.load_sequences(src if spliced else want)
            st = forward_state(net)
            net.compute_backward_pass()
            st["output errors"] = net.output_layer().output_errors().tobytes()
            states.append(st)
    assert_same(states[0], states[1], k)


def test_a_ctc_net_at_a_skip_of_two_gives_the_host_path_s_loss_and_errors(pkg):
    rng = np.random.RandomState(11)
    layers = [{"name": "input", "type": "input", "size": 3 * P0}, {"name": "blstm", "type": "blstm", "size": 8, "bias": 1.0},
              {"name": "output", "type": "softmax", "size": 5, "bias": 1.0}, {"name": "postoutput", "type": "ctc", "size": 5}]
    weights = random_weights(layers, rng, 0.4)
    xs = [rng.randn(n, P0).astype(np.float32) for n in LENGTHS]
    labels = [[1, 0, 3], [2, 2], [0], []]                     # 2U - 1 repeats included: 3, 3, 1, 0 frames needed of 6, 4, 1, 1
    src = contiguous(pkg.make_fraction(xs, None, PS, labels=labels))
    want = SR.network_fraction(src, (1, 1), 2)
    assert want["seqLengths"] == [6, 4, 1, 1] and want["labels"] is src["labels"]
    states = []
    for spliced in (True, False):
        with pkg.NeuralNetwork(layers, weights, PS, T, deterministic=True) as net:
            if spliced:
                net.set_input_splice((1, 1), 2)
            net.load_sequences(src if spliced else want)
            st = forward_state(net)
            net.compute_backward_pass()
            st["output errors"] = net.output_layer().output_errors().tobytes()
            states.append(st)
    assert states[0]["error"][0] > 0 and np.frombuffer(states[0]["output errors"], np.float32).any()
    assert_same(states[0], states[1], "ctc")


MASKS = dict(freq_masks=3, freq_width=3, time_masks=3, time_width=4, time_max_permille=500, seed=SEED)


def first_pass(condition, settings):
    """the smallest pass >= 0 under which the restatement meets `condition`"""
    for p in range(1000):
        st = dict(settings, pass_=p)
        if condition(st):
            return st
    raise AssertionError("no pass below 1000 meets the precondition")


def time_masks_cover_a_frame_read_and_a_frame_skipped(st, k=3):
    """some time mask covers a source frame that a skip of k reads (context (0, 0): frames k * j) and one that it skips"""
    _, time = AR.mask_table(st, np.array(LENGTHS + [0]), P0)
    covered = {t for t0, w in time.reshape(-1, 2) for t in range(t0, t0 + w)}
    return any(t % k == 0 for t in covered) and any(t % k != 0 for t in covered)


@pytest.mark.parametrize("prec", PRECS)
def test_with_augmentation_a_skip_of_one_is_the_host_spliced_load(pkg, prec):
    st = first_pass(time_masks_cover_a_frame_read_and_a_frame_skipped, dict(MASKS, noise_sigma=0.6, context=(1, 2)))
    src = source(pkg)
    with network(pkg, prec, (1, 2)) as net:
        net.set_input_augment(**st)
        net.load_sequences(SR.network_fraction(src, (1, 2), 1))
        want = net.input_layer().outputs()
    with network(pkg, prec, (1, 2)) as net:
        net.set_input_augment(**st)
        net.set_input_splice((1, 2), 1)
        net.load_sequences(src)
        got = net.input_layer().outputs()
    assert want.tobytes() != SR.network_fraction(src, (1, 2), 1)["inputs"].tobytes()
    assert got.tobytes() == want.tobytes()


def test_with_augmentation_a_skip_of_three_gathers_the_augmented_source(pkg):
    """context (0, 0), K = 3: the read-back is rows 3 j of the restatement's augmentation of the SOURCE fraction: masks and noise
    are functions of the source element, the time masks count source frames"""
    st = first_pass(time_masks_cover_a_frame_read_and_a_frame_skipped, dict(MASKS, noise_sigma=0.6))
    src = source(pkg)
    x, pat = src["inputs"].reshape(T, PS, P0), src["patTypes"].reshape(T, PS)
    lens = SR.source_lengths(src)
    ref, bound, masked = AR.apply(x, pat, st)
    ref, bound, masked = (SR.gather(v, lens, (0, 0), 3) for v in (ref, bound, masked))
    real = np.broadcast_to((SR.network_fraction(src, (0, 0), 3)["patTypes"].reshape(4, PS) != 0)[:, :, None], ref.shape)
    assert masked.any() and not masked[real].all() and np.all(bound[real & ~masked] > 0) and not bound[~real].any()      # the restatement alone
    got = {}
    for prec in ("PREC_F32", "PREC_BF16X3"):
        with network(pkg, prec) as net:
            net.set_input_augment(**st)
            net.set_input_splice((0, 0), 3)
            net.load_sequences(src)
            got[prec] = net.input_layer().outputs()
    g = got["PREC_F32"]
    assert g.shape == ref.shape
    err = np.abs(g.astype(np.float64) - ref.astype(np.float64))
    print("largest |device - reference| = %.3f of the bound" % float((err[bound > 0] / bound[bound > 0]).max()))
    assert np.all(err <= bound)
    assert not g[masked].any() and not np.signbit(g[masked]).any() and not g[~real].any()
    assert got["PREC_BF16X3"].tobytes() == g.tobytes()


def test_off_and_the_identity(pkg):
    """set_input_splice(None) after use restores the plain load; {0, 0, 1} is on and equals the plain load"""
    src = source(pkg)
    with network(pkg) as net:
        net.load_sequences(src)
        plain = dict(forward_state(net), **train_state(net))
    with network(pkg) as net:
        net.set_input_splice((0, 0), 3)
        net.load_sequences(src)
        assert net.T == 4 and forward_state(net)["inputs"] != plain["inputs"]
        net.set_input_splice(None)
        net.load_sequences(src)
        assert_same(dict(forward_state(net), **train_state(net)), plain, "off")
    with network(pkg) as net:
        net.set_input_splice((0, 0), 1)
        net.load_sequences(src)
        assert_same(dict(forward_state(net), **train_state(net)), plain, "identity")


@pytest.mark.parametrize("context,k,word", [((-1, 0), 1, "context"), ((0, -1), 1, "context"), ((33, 0), 1, "context"), ((0, 33), 1, "context"),
                                            ((0, 0), 0, "frame_skip"), ((0, 0), 17, "frame_skip")])
def test_bad_settings_are_refused(pkg, context, k, word):
    src = source(pkg)
    with network(pkg) as net:
        with pytest.raises(pkg.CurrenntHipError) as e:
            net.set_input_splice(context, k)
        assert e.value.code == BAD_ARG and "cn_ctx_set_input_splice" in str(e.value) and word in str(e.value)
        net.load_sequences(src)                                      # ... and the context is still off and usable
        assert net.T == T and net.input_layer().outputs().tobytes() == src["inputs"].tobytes()
        net.set_input_splice((32, 32), 16)                          # the largest values are accepted (the load would find the shape)
        net.set_input_splice(None)


def test_shape_errors_are_found_at_the_load(pkg):
    src = source(pkg)
    spliced = SR.network_fraction(src, (1, 2), 1)

    def refused(net, fr, *words):
        with pytest.raises(pkg.CurrenntHipError) as e:
            net.load_sequences(fr)
        assert e.value.code == SHAPE and all(w in str(e.value) for w in words), str(e.value)

    with network(pkg) as net:                                        # input layer of 5: two frames do not divide it
        net.set_input_splice((1, 0), 1)
        refused(net, src, "no multiple")
        net.set_input_splice((0, 0), 2)
        net.load_sequences(src)
        assert net.T == 6
    with network(pkg, context=(1, 2)) as net:                        # input layer of 20 = 4 x 5: the fraction must bring 5
        net.set_input_splice((1, 2), 2)
        refused(net, spliced, "Input layer size of 20", "5", "data input pattern size of 20")
        net.set_input_augment(0.1, context=(2, 1))                   # the augmentation's context must be the splice's
        refused(net, src, "augmentation", "(2, 1)", "(1, 2)")
        net.set_input_augment(None)
        net.load_sequences(src)
        assert net.T == 6 and net.input_layer().outputs().tobytes() == SR.network_fraction(src, (1, 2), 2)["inputs"].tobytes()
    with network(pkg, max_seq_length=5) as net:                      # ceil(12 / 2) = 6 steps do not fit layers of 5, ceil(12 / 3) = 4 do
        net.set_input_splice((0, 0), 2)
        refused(net, src, "max_seq_length", "6")
        net.set_input_splice((0, 0), 3)
        net.load_sequences(src)
        assert net.T == 4 and net.input_layer().outputs().tobytes() == SR.network_fraction(src, (0, 0), 3)["inputs"].tobytes()
