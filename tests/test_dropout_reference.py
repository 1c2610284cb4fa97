"""CPU checks of the numpy restatement of the dropout mask (tests/dropout_reference.py) that the GPU is held to bit for bit
(tests/test_gpu_dropout.py): Philox4x32-10 known answers, the threshold's ends, the kept share, and the declarations."""
import os
import re

import numpy as np
import pytest

from dropout_reference import apply, bf16_round, keep, philox4x32_10, scale, threshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cn_layer_set_dropout", "cn_ctx_set_dropout_pass", "cn_dbg_dropout_input")

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    got = philox4x32_10(np.array(counter, np.uint32), key)
    assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]


def test_philox_is_vectorised_like_it_is_scalar():
    ctr = np.array([c for c, _, _ in KNOWN_ANSWERS], np.uint32)
    for k, (c, key, want) in enumerate(KNOWN_ANSWERS):
        assert tuple(int(w) for w in philox4x32_10(ctr, key)[k]) == want


def test_threshold_and_scale():
    assert threshold(0.0) == 0 and keep(1, 2, 3, 5, 7, 0.0).all()              # rate 0 keeps everything
    assert threshold(0.5) == 2 ** 31 and threshold(0.25) == 2 ** 30 and threshold(0.125) == 2 ** 29
    assert threshold(np.nextafter(np.float32(1.0), np.float32(0.0))) == 2 ** 32 - 2 ** 8 < 2 ** 32    # the largest rate fits a uint32
    assert scale(0.5) == np.float32(2.0) and scale(0.2) == np.float32(1.0 / (1.0 - float(np.float32(0.2))))
    assert scale(0.2).dtype == np.float32


def test_mask_is_a_function_of_frame_and_unit_alone():
    """keep(n, i) does not depend on how many frames or units are asked for, and differs between ordinals, passes and seeds."""
    a = keep(0x1234567, 2, 5, 27, 10, 0.25)
    assert np.array_equal(a[:9, :7], keep(0x1234567, 2, 5, 9, 7, 0.25))
    assert a.dtype == bool and a.shape == (27, 10)
    for other in (keep(0x1234567, 3, 5, 27, 10, 0.25), keep(0x1234567, 2, 6, 27, 10, 0.25), keep(0x1234568, 2, 5, 27, 10, 0.25),
                  keep(0x1234567 + (1 << 32), 2, 5, 27, 10, 0.25), keep(0x1234567, 2, 5 + (1 << 32), 27, 10, 0.25)):
        assert not np.array_equal(a, other)
    # the key's low word wraps: seed_lo + ordinal mod 2^32
    assert np.array_equal(keep(0xFFFFFFFF, 1, 5, 4, 8, 0.5), keep(0, 0, 5, 4, 8, 0.5))


@pytest.mark.parametrize("rate", [0.1, 0.25, 0.5])
def test_kept_share(rate):
    """2^16 elements: the kept count is binomial(n, 1 - p) with p = thr / 2^32, so it lies within 4 sigma = 4 sqrt(n p (1 - p))
    of n (1 - p) except with probability 6e-5 -- for a fixed key, a fixed fact that holds or does not."""
    n = 1 << 16
    m = keep(0x1234567, 1, 5, 256, 256, rate)
    p = threshold(rate) / 2.0 ** 32
    assert abs(int(m.sum()) - n * (1 - p)) <= 4 * np.sqrt(n * p * (1 - p)), (int(m.sum()), n * (1 - p))


def test_apply_and_bf16_rounding():
    x = np.array([1.0, -3.0, 0.1, 1.00390625, 1.01171875, -0.0], np.float32)      # 1 + 2^-8 and 1 + 3 * 2^-8: ties to even
    assert np.array_equal(bf16_round(x).view(np.uint32) >> 16, [0x3F80, 0xC040, 0x3DCD, 0x3F80, 0x3F82, 0x8000])
    m = np.array([True, False, True, True, False, True])
    y = apply(x, m, 0.5)
    assert np.array_equal(y, [2.0, 0.0, np.float32(0.1) * np.float32(2.0), 2.0078125, 0.0, -0.0])
    assert not np.signbit(y[1]) and not np.signbit(y[4]) and np.signbit(y[5])       # dropped: +0; a kept -0 stays -0
    assert np.array_equal(apply(x, m, 0.5, bf16=True), bf16_round(y))


def test_new_symbols_are_declared_and_bound(pkg):
    headers = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("currennt_hip.h", "currennt_hip_debug.h"))
    for sym in NEW_SYMBOLS:
        assert sym in pkg.binding.EXPORTS
        assert re.search(r"\bint\s+%s\(" % sym, headers), sym
    assert hasattr(pkg.NeuralNetwork, "set_dropout_pass")
    for name in ("dropout_input", "set_dropout"):
        assert hasattr(pkg.network.Layer, name)
