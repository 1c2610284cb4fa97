"""CPU checks of the numpy restatement of the weight noise (tests/noise_reference.py) that the GPU is held to
(tests/test_gpu_noise.py): the ends of the uniforms, the pair and cos / sin assignment, the separation of the streams, the first
two moments, the error budget, and the declarations."""
import os
import re

import numpy as np

import noise_reference as NR
from dropout_reference import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cn_ctx_set_weight_noise", "cn_dbg_noisy_weights")


def test_uniform_ends():
    """word 0 gives u1 = 2^-24 and word 0xFFFFFFFF gives u1 = 1 - 2^-24: never 0 (log) and never 1; both exact in fp32"""
    u1, t = NR.uniforms_of_words([0, 0xFFFFFFFF], [0, 0xFFFFFFFF])
    assert u1[0] == 2.0 ** -24 and u1[1] == 1.0 - 2.0 ** -24
    assert t[0] == 2.0 ** -23 and t[1] == 2.0 - 2.0 ** -23
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(t.astype(np.float32).astype(np.float64), t)
    # the low nine bits of a word do not count
    assert NR.uniforms_of_words([0x1FF], [0x1FF])[0][0] == 2.0 ** -24
    assert NR.uniforms_of_words([0x200], [0x200])[0][0] == 3 * 2.0 ** -24


def test_pair_and_branch_assignment():
    """k & 3 = 0, 1 share words (0, 1) -- cosine, sine; k & 3 = 2, 3 share words (2, 3) -- cosine, sine"""
    seed, ordinal, pass_ = 0x1234567, 2, 5
    w = NR.words(seed, ordinal, pass_, 8)
    z, r = NR.gauss(seed, ordinal, pass_, 8)
    for k in range(8):
        p = (k & 3) >> 1
        u1, t = NR.uniforms_of_words(w[k >> 2, 2 * p], w[k >> 2, 2 * p + 1])
        rr = np.sqrt(-2.0 * np.log(u1))
        want = rr * (np.sin(np.pi * t) if k & 1 else np.cos(np.pi * t))
        assert abs(r[k] - rr) <= 1e-14 * rr and abs(z[k] - want) <= 1e-14 * rr, k     # (array and scalar libm paths may differ in the last bit)
    assert r[0] == r[1] and r[2] == r[3] and r[0] != r[2]
    # the two outputs of a pair lie on one circle
    assert abs(z[0] ** 2 + z[1] ** 2 - r[0] ** 2) < 1e-12
    # a count that is no multiple of four takes the first entries of the last group
    assert np.array_equal(NR.gauss(seed, ordinal, pass_, 7)[0], z[:7])


def test_stream_is_apart_from_dropout_and_differs_across_keys():
    seed, ordinal, pass_ = 0x89ABCDEF01234567, 3, (7 << 32) | 11
    w = NR.words(seed, ordinal, pass_, 64)
    # the dropout words of the same seed, ordinal and pass at frame 0: the same counters under the key without the XOR
    ctr = np.zeros((16, 4), np.uint32)
    ctr[:, 0] = np.arange(16)
    ctr[:, 2] = pass_ & 0xFFFFFFFF
    ctr[:, 3] = pass_ >> 32
    drop = philox4x32_10(ctr, (((seed & 0xFFFFFFFF) + ordinal) & 0xFFFFFFFF, seed >> 32))
    assert not np.any(w == drop)
    assert NR.key(seed, ordinal) == (((seed & 0xFFFFFFFF) + ordinal) & 0xFFFFFFFF, (seed >> 32) ^ 0x6E6F6973)
    z = NR.gauss(seed, ordinal, pass_, 64)[0]
    for other in (NR.gauss(seed, ordinal + 1, pass_, 64)[0], NR.gauss(seed, ordinal, pass_ + 1, 64)[0],
                  NR.gauss(seed, ordinal, pass_ + (1 << 32), 64)[0], NR.gauss(seed + 1, ordinal, pass_, 64)[0],
                  NR.gauss(seed + (1 << 32), ordinal, pass_, 64)[0]):
        assert not np.any(z == other)
    # the key's low word wraps: seed_lo + ordinal mod 2^32
    assert np.array_equal(NR.gauss(0xFFFFFFFF, 1, 5, 16)[0], NR.gauss(0, 0, 5, 16)[0])


def test_first_two_moments():
    """n = 2^20 samples of a standard normal: the mean has standard deviation 1/sqrt(n), the sample variance sqrt(2/n); five of
    those each (one in 1.7 million for a true normal) -- for a fixed key, a fixed fact that holds or does not."""
    n = 1 << 20
    z = NR.gauss(0x1234567, 1, 5, n)[0]
    assert abs(z.mean()) <= 5.0 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n), z.var()
    # the quantisation of u1 bounds the tail: r <= sqrt(-2 ln 2^-24)
    assert np.abs(z).max() <= np.sqrt(48 * np.log(2.0))


def test_error_budget():
    """every step of the device's evaluation contributes a few ulp at the most: a looser budget would mean a wrong formula"""
    assert NR.A + NR.B <= 16
    assert NR.A == 2 * NR.ULP_TRIG and NR.B == NR.ULP_LOG + 4
    w = np.linspace(-1, 1, 917).astype(np.float32)
    ref, bound = NR.noisy(w, 0.1, 7, 2, 3)
    z, r = NR.gauss(7, 2, 3, 917)
    assert ref.dtype == np.float32 and np.array_equal(ref, (w.astype(np.float64) + (float(np.float32(0.1)) * z).astype(np.float32)).astype(np.float32))
    assert np.all(bound >= np.spacing(np.abs(ref))) and np.all(bound <= np.spacing(np.abs(ref)) + 0.1 * 2.0 ** -24 * 16 * r.max())


def test_bias_slices():
    assert NR.bias_slice("blstm", 12, 5) == slice(240, 288)
    assert NR.bias_slice("lstm", 7, 12) == slice(336, 364)
    assert NR.bias_slice("softmax", 4, 6) == slice(24, 28)


def test_new_symbols_are_declared_and_bound(pkg):
    headers = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("currennt_hip.h", "currennt_hip_debug.h"))
    for sym in NEW_SYMBOLS:
        assert sym in pkg.binding.EXPORTS
        assert re.search(r"\bint\s+%s\(" % sym, headers), sym
    assert hasattr(pkg.NeuralNetwork, "set_weight_noise")
    assert hasattr(pkg.network.Layer, "noisy_weights")
