"""-m gpu: input augmentation on the device (cn_ctx_set_input_augment) against its numpy restatement (tests/augment_reference.py):
the noise values, the masks, splicing, every load path, the prefetch record, that the kernels train on what is read back, off,
the keys and the errors.

The shapes are the smallest at which the re-layout can go wrong: 5 features per frame (no multiple of four: the Philox groups
straddle frames), four slots holding sequences of 12, 8 and 1 frames and an empty one (padded to more slots on the device),
12 time steps, contexts (0, 0) and (1, 2) -- the latter an input layer of 20 -- in front of lstm 7 -> softmax 4.  Before any
device call each test asserts that the restatement alone meets the test's precondition."""
import numpy as np
import pytest

import augment_reference as AR
from helpers import net_desc, random_sequences, random_weights

pytestmark = pytest.mark.gpu
PRECS = ["PREC_F32", "PREC_BF16", "PREC_BF16X3"]
P0, C, PS, T = 5, 4, 4, 12
LENGTHS = [12, 8, 1]
SEED = 0x0123456789ABCDEF
NOISE = dict(noise_sigma=0.6, seed=SEED, pass_=5)
MASKS = dict(freq_masks=3, freq_width=3, time_masks=3, time_width=4, time_max_permille=500, seed=SEED)
LR, MOM = 1e-2, 0.9
BAD_ARG, SHAPE = -1, -2


def layers_of(context):
    return net_desc(P0 * (context[0] + context[1] + 1), [("lstm", 7)], C)


def network(pkg, prec="PREC_F32", context=(0, 0), options=None):
    layers = layers_of(context)
    return pkg.NeuralNetwork(layers, random_weights(layers, np.random.RandomState(77), 0.3), PS, T, precision=getattr(pkg, prec),
                             deterministic=True, options=options)


def fraction(pkg, k=0, context=(0, 0), lengths=LENGTHS, order=None):
    """fraction k; its arrays are the contiguous ones a prefetch and its load both hand over (a hint is matched by address)"""
    xs, ts = random_sequences(np.random.RandomState(1000 + k), lengths, P0, C=C)
    if order is not None:
        xs, ts = [xs[i] for i in order], [ts[i] for i in order]
    fr = pkg.make_fraction(xs, ts, PS, context_left=context[0], context_right=context[1])
    fr["inputs"] = np.ascontiguousarray(fr["inputs"], np.float32); fr["patTypes"] = np.ascontiguousarray(fr["patTypes"], np.int8)
    fr["targetClasses"] = np.ascontiguousarray(fr["targetClasses"], np.int32)
    return fr


def arrays(fr):
    """(x [T][PS][P], pat [T][PS]) of a fraction"""
    return fr["inputs"].reshape(fr["T"], PS, -1), fr["patTypes"].reshape(fr["T"], PS)


def read_back(net):
    return net.input_layer().outputs()


def loaded(net, fr, settings):
    net.set_input_augment(**settings)
    net.load_sequences(fr)
    return read_back(net)


def first_pass(condition, settings):
    """the smallest pass >= 0 under which the restatement meets `condition`"""
    for p in range(1000):
        st = dict(settings, pass_=p)
        if condition(st):
            return st
    raise AssertionError("no pass below 1000 meets the precondition")


def masks_cover_every_case(st):
    freq, time = AR.mask_table(st, np.array(LENGTHS + [0]), P0)
    widths = np.concatenate([freq[:3, :, 1].reshape(-1), time[:3, :, 1].reshape(-1)])
    return all(freq[s, :, 1].max() >= 1 and time[s, :, 1].max() >= 1 for s in (0, 1)) and (widths == 0).any()


def resident(torch, fr):
    """the fraction in HBM: (descriptor for load_sequences_resident, the tensors that own the memory)"""
    dev = {k: torch.from_numpy(fr[k]).cuda() for k in ("inputs", "patTypes", "targetClasses")}
    d = {"T": fr["T"], "Tmin": fr["Tmin"], "numSeqs": fr["numSeqs"], "inputPatternSize": fr["inputs"].shape[-1], "outputPatternSize": C}
    d.update({k: v.data_ptr() for k, v in dev.items()})
    return d, dev


def train_step(net):
    net.compute_forward_pass(); net.compute_backward_pass()
    updates = {l.name: l.weight_updates() for l in net.trainable_layers()}
    net.update_weights(LR, MOM)
    return {l.name: (l.weights(), updates[l.name]) for l in net.trainable_layers()}


def assert_same_step(a, b, what):
    for name in a:
        for k, part in enumerate(("weights", "weight updates")):
            assert a[name][k].tobytes() == b[name][k].tobytes(), (what, name, part, float(np.abs(a[name][k] - b[name][k]).max()))


@pytest.fixture(scope="module")
def f32_noisy(pkg):
    """the f32-mode read-back of fraction 0 under NOISE, formed once"""
    with network(pkg) as net:
        return loaded(net, fraction(pkg), NOISE)


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16X3"])
def test_noise_values_keep_to_the_restatement(pkg, prec, f32_noisy):
    """the input layer's read-back = float32(x + float32(sigma z_ref)) within sigma 2^-24 (A r + B |z|) plus one ulp of the sum
    (A = 2, B = 5: tests/noise_reference.py); NONE frames, the empty slot and the pad stay what they were.  The largest error
    observed, as a share of that bound, is printed."""
    fr = fraction(pkg)
    x, pat = arrays(fr)
    ref, bound, masked = AR.apply(x, pat, NOISE)
    real = np.broadcast_to((pat != 0)[:, :, None], x.shape)
    assert AR.A + AR.B <= 16 and not masked.any()
    assert np.all(bound[real] > 0) and not bound[~real].any() and np.mean(ref[real] != x[real]) > 0.99       # the reference alone
    with network(pkg, prec) as net:
        got = loaded(net, fr, NOISE)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    share = float((err[real] / bound[real]).max())
    print("%s: largest |device - reference| = %.3f of the bound (%d elements)" % (prec, share, int(real.sum())))
    assert np.all(err <= bound), (share, int(np.argmax(err / np.maximum(bound, 1e-300))))
    assert got[~real].tobytes() == x[~real].tobytes()
    if prec == "PREC_BF16X3":                                     # the noise does not depend on the precision mode
        assert got.tobytes() == f32_noisy.tobytes()


def test_bf16_noise_values_are_the_rounded_f32_values(pkg, f32_noisy):
    """CN_PREC_BF16 rounds the sum once to the operand type: the read-back is the bf16 rounding of the f32-mode read-back"""
    want = AR.bf16_round(f32_noisy)
    moved = f32_noisy != 0
    assert np.mean(want[moved] != f32_noisy[moved]) > 0.9         # the rounding is not a no-op on these values
    with network(pkg, "PREC_BF16") as net:
        got = loaded(net, fraction(pkg), NOISE)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("prec", PRECS)
def test_masks_equal_the_restatement_bit_for_bit(pkg, prec):
    """sigma 0: masked elements are +0.0, every other element is the loaded value (after bf16 rounding in bf16); NONE frames, the
    empty slot and the pad stay zero"""
    st = first_pass(masks_cover_every_case, MASKS)
    fr = fraction(pkg)
    x, pat = arrays(fr)
    ref, bound, masked = AR.apply(x, pat, st, bf16=prec == "PREC_BF16")
    assert not bound.any() and masked[:, 0].any() and masked[:, 1].any() and not masked[:, 3].any() and not masked[8:, 1].any()
    assert np.array_equal(ref[~masked], (AR.bf16_round(x) if prec == "PREC_BF16" else x)[~masked])
    with network(pkg, prec) as net:
        got = loaded(net, fr, st)
    assert got.tobytes() == ref.tobytes(), (st["pass_"], int((got != ref).sum()))
    assert not got[masked].any() and not np.signbit(got[masked]).any()
    assert not got[8:, 1].any() and not got[1:, 2].any() and not got[:, 3].any()


@pytest.mark.parametrize("prec", PRECS)
def test_noise_and_masks_commute_with_splicing(pkg, prec):
    """context (1, 2): the device read-back equals the host splice of the device read-back of the unspliced fraction (context
    (0, 0), input size 5), bit for bit: every context copy of a frame carries the same noise and the same masks"""
    st = first_pass(masks_cover_every_case, dict(MASKS, noise_sigma=0.6))
    lens = np.array(LENGTHS + [0])
    x, pat = arrays(fraction(pkg))
    plain_ref, _, masked = AR.apply(x, pat, st)
    spliced_ref, _, _ = AR.apply(AR.splice(x, lens, 1, 2), pat, dict(st, context=(1, 2)))
    assert spliced_ref.tobytes() == AR.splice(plain_ref, lens, 1, 2).tobytes() and masked.any() and not masked[pat != 0].all()
    with network(pkg, prec) as net:
        plain = loaded(net, fraction(pkg), st)
    with network(pkg, prec, context=(1, 2)) as net:
        fr = fraction(pkg, context=(1, 2))
        assert fr["inputs"].tobytes() == AR.splice(x, lens, 1, 2).tobytes()
        spliced = loaded(net, fr, dict(st, context=(1, 2)))
    assert spliced.shape == (T, PS, 20)
    assert spliced.tobytes() == AR.splice(plain, lens, 1, 2).tobytes()


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
def test_every_load_path_gives_the_same_bits(pkg, prec):
    """host load (staged upload), resident load, a host prefetch and a resident prefetch that their loads take over
    (prefetch_hits advances), and the strided copies of option overlap = 0"""
    import torch
    st = first_pass(masks_cover_every_case, dict(MASKS, noise_sigma=0.6, context=(1, 2)))
    fr, other = fraction(pkg, 0, (1, 2)), fraction(pkg, 1, (1, 2), lengths=[7, 12, 3, 5])
    x, pat = arrays(fr)
    ref, bound, masked = AR.apply(x, pat, st)
    assert masked.any() and bound.any()
    got = {}
    with network(pkg, prec, (1, 2)) as net:
        got["host"] = loaded(net, fr, st)
    with network(pkg, prec, (1, 2), options={"overlap": 0}) as net:
        got["strided"] = loaded(net, fr, st)
    d, keep = resident(torch, fr)
    d_other, keep_other = resident(torch, other)
    with network(pkg, prec, (1, 2)) as net:
        net.set_input_augment(**st)
        net.load_sequences_resident(d)
        got["resident"] = read_back(net)
    for kind in ("host", "resident"):
        with network(pkg, prec, (1, 2)) as net:
            net.set_input_augment(**st)
            if kind == "host":
                net.load_sequences(other); net.compute_forward_pass(); net.prefetch_sequences(fr)
            else:
                net.load_sequences_resident(d_other); net.compute_forward_pass(); net.prefetch_sequences_resident(d)
            net.compute_backward_pass()
            assert net.prefetch_hits() == 0
            net.load_sequences(fr) if kind == "host" else net.load_sequences_resident(d)
            assert net.prefetch_hits() == 1, kind
            got[kind + " prefetch"] = read_back(net)
    if prec == "PREC_F32":
        assert np.all(np.abs(got["host"].astype(np.float64) - ref) <= bound)
    for name, v in got.items():
        assert v.tobytes() == got["host"].tobytes(), (name, int((v != got["host"]).sum()))


@pytest.mark.parametrize("kind", ["host", "resident"])
def test_a_prefetch_under_other_settings_is_not_a_hit(pkg, kind):
    """the prefetch records the settings in force when it is announced; a load under other settings discards it
    (prefetch_hits unchanged) and leaves what its own settings give"""
    import torch
    fr, other = fraction(pkg, 0), fraction(pkg, 1, lengths=[7, 12, 3, 5])
    d, keep = resident(torch, fr)
    d_other, keep_other = resident(torch, other)
    at_prefetch, at_load = dict(NOISE, pass_=1), dict(NOISE, pass_=2)
    x, pat = arrays(fr)
    assert AR.apply(x, pat, at_prefetch)[0].tobytes() != AR.apply(x, pat, at_load)[0].tobytes()
    with network(pkg) as net:
        want = loaded(net, fr, at_load)
        clean = loaded(net, fr, {})
    assert clean.tobytes() == x.tobytes()
    for load_settings, expect in ((at_load, want), (None, clean)):
        with network(pkg) as net:
            net.set_input_augment(**at_prefetch)
            if kind == "host":
                net.load_sequences(other); net.compute_forward_pass(); net.prefetch_sequences(fr)
            else:
                net.load_sequences_resident(d_other); net.compute_forward_pass(); net.prefetch_sequences_resident(d)
            net.compute_backward_pass()
            if load_settings is None:
                net.set_input_augment(None)
            else:
                net.set_input_augment(**load_settings)
            net.load_sequences(fr) if kind == "host" else net.load_sequences_resident(d)
            assert net.prefetch_hits() == 0
            assert read_back(net).tobytes() == expect.tobytes()
            # ... and the very same settings again are a hit
            net.compute_forward_pass()
            net.prefetch_sequences(fr) if kind == "host" else net.prefetch_sequences_resident(d)
            net.compute_backward_pass()
            net.load_sequences(fr) if kind == "host" else net.load_sequences_resident(d)
            assert net.prefetch_hits() == 1
            assert read_back(net).tobytes() == expect.tobytes()


@pytest.mark.parametrize("prec", PRECS)
def test_the_kernels_train_on_what_was_read_back(pkg, prec):
    """deterministic mode: one forward / backward / update under augmentation is bit-equal to the same step with augmentation
    off on a fraction whose inputs are the read-back (in bf16 the read-back is representable, so it loads unchanged)"""
    st = first_pass(masks_cover_every_case, dict(MASKS, noise_sigma=0.6))
    fr = fraction(pkg)
    with network(pkg, prec) as net:
        seen = loaded(net, fr, st)
        augmented = train_step(net)
    assert seen.tobytes() != arrays(fr)[0].tobytes()
    fed = dict(fr, inputs=np.ascontiguousarray(seen.reshape(T * PS, P0)))
    with network(pkg, prec) as net:
        net.load_sequences(fed)
        assert read_back(net).tobytes() == seen.tobytes()
        plain = train_step(net)
    assert_same_step(augmented, plain, prec)


def test_off_is_off(pkg):
    """set, then clear -- with NULL and with the all-zero struct: a training step is bit-equal to that of a context that never
    made the call"""
    fr = fraction(pkg)
    steps = {}
    for how in ("never", "null", "zero"):
        with network(pkg) as net:
            if how != "never":
                net.set_input_augment(**dict(MASKS, noise_sigma=0.6))
                net.set_input_augment(None) if how == "null" else net.set_input_augment(0.0, time_max_permille=0)
            net.load_sequences(fr)
            assert read_back(net).tobytes() == arrays(fr)[0].tobytes(), how
            steps[how] = train_step(net)
    assert_same_step(steps["never"], steps["null"], "null")
    assert_same_step(steps["never"], steps["zero"], "zero")


def test_keys(pkg):
    """the same settings twice give the same bits; another pass, another seed, or the same sequence in another slot do not"""
    st = dict(MASKS, noise_sigma=0.6, pass_=3)
    fr, swapped = fraction(pkg), fraction(pkg, order=[1, 0, 2])
    x, pat = arrays(fr)
    assert np.array_equal(arrays(swapped)[0][:8, 0], x[:8, 1])
    a = AR.apply(x, pat, st)[0]
    assert a.tobytes() != AR.apply(x, pat, dict(st, pass_=4))[0].tobytes() and a.tobytes() != AR.apply(x, pat, dict(st, seed=SEED + 1))[0].tobytes()
    assert AR.apply(*arrays(swapped), NOISE)[0][:8, 0].tobytes() != AR.apply(x, pat, NOISE)[0][:8, 1].tobytes()
    with network(pkg) as net:
        first = loaded(net, fr, st)
        assert loaded(net, fraction(pkg, 1, lengths=[7, 12, 3, 5]), st).tobytes() != first.tobytes()
        assert loaded(net, fr, st).tobytes() == first.tobytes()
        assert loaded(net, fr, dict(st, pass_=4)).tobytes() != first.tobytes()
        assert loaded(net, fr, dict(st, seed=SEED + 1)).tobytes() != first.tobytes()
        assert loaded(net, fr, dict(st, seed=SEED + 2 ** 32)).tobytes() != first.tobytes()           # the high word is part of the key
        noisy = loaded(net, fr, NOISE)
        noisy_swapped = loaded(net, swapped, NOISE)
    assert noisy_swapped[:8, 0].tobytes() != noisy[:8, 1].tobytes()
    assert np.abs(noisy_swapped[:8, 0] - noisy[:8, 1]).max() > 0.1


@pytest.mark.parametrize("bad,word", [
    (dict(noise_sigma=-0.1), "noise_sigma"), (dict(noise_sigma=float("nan")), "noise_sigma"), (dict(noise_sigma=float("inf")), "noise_sigma"),
    (dict(noise_sigma=0.1, context=(-1, 0)), "context"), (dict(noise_sigma=0.1, context=(0, -2)), "context"),
    (dict(freq_masks=-1), "freq_masks"), (dict(time_masks=-1), "time_masks"), (dict(freq_masks=9), "0..8"), (dict(time_masks=9), "0..8"),
    (dict(freq_masks=1, freq_width=-1), "freq_width"), (dict(time_masks=1, time_width=-3), "time_width"),
    (dict(time_masks=1, time_max_permille=-1), "time_max_permille"), (dict(time_masks=1, time_max_permille=1001), "time_max_permille"),
])
def test_bad_settings_are_refused(pkg, bad, word):
    with network(pkg) as net:
        with pytest.raises(pkg.CurrenntHipError) as e:
            net.set_input_augment(**bad)
        assert e.value.code == BAD_ARG and "cn_ctx_set_input_augment" in str(e.value) and word in str(e.value)
        # ... and the context is still off
        fr = fraction(pkg)
        net.load_sequences(fr)
        assert read_back(net).tobytes() == arrays(fr)[0].tobytes()


def test_an_input_size_that_the_context_does_not_divide_fails_at_the_load(pkg):
    fr = fraction(pkg)
    with network(pkg) as net:
        net.set_input_augment(0.1, context=(1, 0))                # accepted: the input layer's size is known at the load
        with pytest.raises(pkg.CurrenntHipError, match="no multiple") as e:
            net.load_sequences(fr)
        assert e.value.code == SHAPE
        net.set_input_augment(0.1, context=(2, 2))                # 5 = 1 * 5
        net.load_sequences(fr)
        assert read_back(net)[pat_real(fr)].tobytes() != arrays(fr)[0][pat_real(fr)].tobytes()


def pat_real(fr):
    return arrays(fr)[1] != 0
