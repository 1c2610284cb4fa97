"""Input augmentation without a GPU: the numpy restatement the GPU tests compare against (tests/augment_reference.py) keeps the
properties include/currennt_hip.h states -- masks inside their range and under their caps, splicing commutes with the
augmentation, a stream apart from the weight noise and the dropout masks, a standard normal -- and the new symbol is declared."""
import os
import re

import numpy as np

import augment_reference as AR
import dropout_reference as DR
import noise_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0, PS, T = 5, 4, 12
LENGTHS = [12, 8, 1]                     # the fourth slot is empty
SEED = 0x0123456789ABCDEF


def patterns():
    pat = np.zeros((T, PS), np.int8)
    for s, n in enumerate(LENGTHS):
        pat[:n, s] = 2
    return pat


def test_lengths_count_the_frames_that_are_not_none():
    assert AR.lengths(patterns(), T, PS).tolist() == LENGTHS + [0]


def test_masks_stay_in_range_and_under_their_caps():
    lens = np.array(LENGTHS + [0])
    widths_seen = set()
    for pass_ in range(200):
        for F, W, permille in ((3, 4, 1000), (9, 30, 1000), (2, 6, 400), (0, 0, 1000), (5, 12, 0)):
            st = dict(freq_masks=8, freq_width=F, time_masks=8, time_width=W, time_max_permille=permille, seed=SEED, pass_=pass_)
            freq, time = AR.mask_table(st, lens, P0)
            assert freq.shape == (PS, 8, 2) and time.shape == (PS, 8, 2)
            for s, n in enumerate(lens):
                f0, fw = freq[s, :, 0], freq[s, :, 1]
                t0, tw = time[s, :, 0], time[s, :, 1]
                if n == 0:
                    assert not freq[s].any() and not time[s].any()
                    continue
                assert np.all(fw <= min(F, P0)) and np.all(f0 >= 0) and np.all(f0 + fw <= P0)
                assert np.all(tw <= min(W, n * permille // 1000)) and np.all(t0 >= 0) and np.all(t0 + tw <= n)
                widths_seen.update(fw.tolist())
            # a one-frame sequence under a cap below the whole: the integer division leaves no room
            if permille < 1000:
                assert not time[2, :, 1].any()
    assert widths_seen == set(range(P0 + 1))                     # every width 0 .. P0 occurs (F = 9 is cut to P0)


def test_a_mask_does_not_depend_on_the_number_of_the_other_kind():
    lens = np.array(LENGTHS + [0])
    a = AR.mask_table(dict(freq_masks=2, freq_width=3, time_masks=2, time_width=4, seed=SEED, pass_=3), lens, P0)
    b = AR.mask_table(dict(freq_masks=5, freq_width=3, time_masks=1, time_width=4, seed=SEED, pass_=3), lens, P0)
    assert np.array_equal(a[0], b[0][:, :2]) and np.array_equal(a[1][:, :1], b[1])


def test_splicing_commutes_with_the_augmentation():
    """the restatement on spliced data = the splice of the restatement on unspliced data, bit for bit: noise and masks belong to
    the source element, so every context copy of a frame carries the same ones"""
    rng = np.random.RandomState(5)
    pat = patterns()
    lens = AR.lengths(pat, T, PS)
    x = rng.randn(T, PS, P0).astype(np.float32) * (pat != 0)[:, :, None]
    hit = False
    for pass_ in range(4):
        st = dict(noise_sigma=0.6, freq_masks=2, freq_width=3, time_masks=2, time_width=4, seed=SEED, pass_=pass_)
        plain, _, masked = AR.apply(x, pat, dict(st, context=(0, 0)))
        for left, right in ((1, 2), (0, 3), (2, 0)):
            spliced, _, _ = AR.apply(AR.splice(x, lens, left, right), pat, dict(st, context=(left, right)))
            assert spliced.tobytes() == AR.splice(plain, lens, left, right).tobytes(), (pass_, left, right)
        hit = hit or (masked.any() and not masked.all())
        assert np.all(plain[masked] == 0) and not np.signbit(plain[masked]).any()
        assert np.array_equal(plain[:, 3], x[:, 3]) and np.array_equal(plain[8:, 1], x[8:, 1])      # empty slot, NONE frames
    assert hit


def test_the_noise_stream_is_apart_from_weight_noise_and_dropout():
    count = 4096
    st = AR.complete(dict(seed=SEED, pass_=9))
    mine = AR._words(st, AR.KEY_NOISE, np.arange(count // 4), 0)
    masks = AR._words(st, AR.KEY_MASK, np.arange(count // 4), 0)
    weight = NR.words(SEED, 0, 9, count)                        # same counters: (g, 0, pass); key word 1 differs
    ctr = np.zeros((count // 4, 4), np.uint32)
    ctr[:, 0] = np.arange(count // 4); ctr[:, 2] = 9
    drop = DR.philox4x32_10(ctr, (SEED & DR.MASK32, SEED >> 32))
    for other in (weight, drop, masks):
        assert other.shape == mine.shape and not (other == mine).all(axis=1).any()
        assert (other == mine).mean() < 1e-3


def test_the_noise_is_standard_normal():
    """over n >= 2 * 10^5 samples the sample mean is within 5 / sqrt(n) and the sample variance within 5 * sqrt(2 / n) of 1"""
    z = np.concatenate([AR.gauss(dict(seed=SEED, pass_=p), s, np.arange(30000))[0] for p in range(2) for s in range(4)])
    n = z.size
    assert n >= 200000
    assert abs(z.mean()) <= 5 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n), z.var()
    # the cosine and the sine branch of a pair are both used: neighbours are uncorrelated
    assert abs(np.corrcoef(z[0:30000:2], z[1:30000:2])[0, 1]) <= 5 / np.sqrt(15000)


def test_no_noise_and_no_masks_is_the_identity():
    rng = np.random.RandomState(6)
    pat = patterns()
    x = rng.randn(T, PS, P0).astype(np.float32)
    x[0, 0, 0] = -0.0
    out, bound, masked = AR.apply(x, pat, dict(freq_masks=3, freq_width=0, time_masks=2, time_width=0, seed=SEED))
    assert out.tobytes() == x.tobytes() and not bound.any() and not masked.any()


def test_the_symbol_the_struct_and_the_method_are_declared(pkg):
    header = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    assert re.search(r"int\s+cn_ctx_set_input_augment\(cn_ctx \*ctx, const cn_input_augment \*a\);", header)
    assert "0x696E7074" in header and "0x6D61736B" in header
    assert "cn_ctx_set_input_augment" in pkg.binding.EXPORTS
    import ctypes
    fields = [f[0] for f in pkg.binding.InputAugment._fields_]
    assert fields == ["noise_sigma", "context_left", "context_right", "freq_masks", "freq_width", "time_masks", "time_width",
                      "time_max_permille", "seed", "pass_"]
    assert ctypes.sizeof(pkg.binding.InputAugment) == 48         # 8 x 4 bytes, then two aligned 64-bit words
    assert hasattr(pkg.NeuralNetwork, "set_input_augment")


def test_the_library_exports_the_symbol(hiplib):
    assert hasattr(hiplib, "cn_ctx_set_input_augment")
