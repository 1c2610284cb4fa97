"""numpy restatement of the input augmentation of include/currennt_hip.h (section Input augmentation): sequence lengths, the
mask table, the noise and their application to a fraction's inputs.

`settings` is a dict with the keywords of NeuralNetwork.set_input_augment: noise_sigma, context = (left, right), freq_masks,
freq_width, time_masks, time_width, time_max_permille, seed, pass_ (missing ones take that method's defaults).

    P0 = P / (left + right + 1);  column c of slot s at time t:  b = c // P0, j = c % P0, ts = clip(t + b - left, 0, len_s - 1)
    noise   e = ts*P0 + j;  words = Philox(counter = (e >> 2, s, pass_lo, pass_hi), key = (seed_lo, seed_hi ^ "inpt"))
            and from there the Box-Muller step of tests/noise_reference.py (float64 here, fp32 on the device)
    masks   (w0, w1, ., .) = Philox(counter = (m, s, pass_lo, pass_hi), key = (seed_lo, seed_hi ^ "mask"));
            frequency mask i is m = i, time mask i is m = 16 + i;  w = w0 % (cap + 1), start = w1 % (range - w + 1)

The device may be off the noisy values by the bound tests/noise_reference.py derives (A = 2, B = 5) plus one ulp of the sum;
masked elements (+0.0), elements without noise (sigma 0), NONE frames, empty slots and padding are exact."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dropout_reference import MASK32, bf16_round, philox4x32_10          # noqa: E402,F401
from noise_reference import A, B, uniforms_of_words                       # noqa: E402,F401

KEY_NOISE = 0x696E7074                   # "inpt"
KEY_MASK = 0x6D61736B                    # "mask"
DEFAULTS = dict(noise_sigma=0.0, context=(0, 0), freq_masks=0, freq_width=0, time_masks=0, time_width=0,
                time_max_permille=1000, seed=0, pass_=0)


def complete(settings):
    s = dict(DEFAULTS)
    s.update(settings)
    s["seed"] = int(s["seed"]) & (2 ** 64 - 1)
    s["pass_"] = int(s["pass_"]) & (2 ** 64 - 1)
    return s


def lengths(pat, T, PS):
    """len_s: the frames of slot s whose pattern type is not NONE"""
    return (np.asarray(pat).reshape(T, PS) != 0).sum(axis=0).astype(np.int64)


def _words(s, key_xor, word0, slot):
    """Philox words for counter word 0 = word0 (array), word 1 = slot (scalar or array)"""
    word0 = np.asarray(word0, np.uint64)
    ctr = np.zeros(word0.shape + (4,), np.uint32)
    ctr[..., 0] = (word0 & np.uint64(MASK32)).astype(np.uint32)
    ctr[..., 1] = np.asarray(slot, np.uint32)
    ctr[..., 2] = s["pass_"] & MASK32
    ctr[..., 3] = s["pass_"] >> 32
    return philox4x32_10(ctr, (s["seed"] & MASK32, (s["seed"] >> 32) ^ key_xor))


def mask_table(settings, lens, P0):
    """(freq, time): int arrays [PS][freq_masks][2] and [PS][time_masks][2] of (start, width); zeros for a slot with len 0"""
    s = complete(settings)
    PS = len(lens)
    freq = np.zeros((PS, s["freq_masks"], 2), np.int64)
    time = np.zeros((PS, s["time_masks"], 2), np.int64)
    for slot, n in enumerate(int(v) for v in lens):
        if n < 1:
            continue
        for i in range(s["freq_masks"]):
            w = _words(s, KEY_MASK, i, slot)
            width = int(w[0]) % (min(s["freq_width"], P0) + 1)
            freq[slot, i] = (int(w[1]) % (P0 - width + 1), width)
        for i in range(s["time_masks"]):
            w = _words(s, KEY_MASK, 16 + i, slot)
            width = int(w[0]) % (min(s["time_width"], n * s["time_max_permille"] // 1000) + 1)
            time[slot, i] = (int(w[1]) % (n - width + 1), width)
    return freq, time


def gauss(settings, slot, e):
    """(z, r), float64, of the source elements e (int array) of slot `slot`"""
    s = complete(settings)
    e = np.asarray(e, np.int64)
    w = _words(s, KEY_NOISE, e >> 2, slot)
    pair = (e & 3) >> 1
    a = np.take_along_axis(w, (2 * pair)[..., None], axis=-1)[..., 0]
    b = np.take_along_axis(w, (2 * pair + 1)[..., None], axis=-1)[..., 0]
    u1, t = uniforms_of_words(a, b)
    r = np.sqrt(-2.0 * np.log(u1))
    z = r * np.where(e & 1, np.sin(np.pi * t), np.cos(np.pi * t))
    return z, r


def apply(x, pat, settings, bf16=False):
    """x: the fraction's inputs [T][PS][P] (float32, spliced by the caller as settings['context'] says), pat [T][PS].
    Returns (x', bound, masked): the augmented inputs as float32 (rounded to bf16 when `bf16`), the distance the device's fp32
    value may keep from them (float64; 0 where the value is exact) and which elements a mask covers."""
    s = complete(settings)
    x = np.asarray(x, np.float32)
    T, PS, P = x.shape
    pat = np.asarray(pat).reshape(T, PS)
    left, right = s["context"]
    blocks = left + right + 1
    if P % blocks:
        raise ValueError("input size %d is no multiple of the context's %d frames" % (P, blocks))
    P0 = P // blocks
    lens = lengths(pat, T, PS)
    freq, time = mask_table(s, lens, P0)
    sigma = np.float32(s["noise_sigma"])
    out = x.copy()
    bound = np.zeros(x.shape, np.float64)
    masked = np.zeros(x.shape, bool)
    c = np.arange(P)
    b, j = c // P0, c % P0
    for slot in range(PS):
        n = int(lens[slot])
        if n < 1:
            continue
        ts = np.clip(np.arange(T)[:, None] + b[None, :] - left, 0, n - 1)                     # [T][P]
        jj = np.broadcast_to(j[None, :], ts.shape)
        m = np.zeros(ts.shape, bool)
        for f0, w in freq[slot]:
            m |= (jj >= f0) & (jj < f0 + w)
        for t0, w in time[slot]:
            m |= (ts >= t0) & (ts < t0 + w)
        real = np.broadcast_to((pat[:, slot] != 0)[:, None], ts.shape)
        m &= real
        v = x[:, slot, :]
        if sigma > 0:
            z, r = gauss(s, slot, ts * P0 + jj)
            n32 = (float(sigma) * z).astype(np.float32)
            noisy = (v.astype(np.float64) + n32.astype(np.float64)).astype(np.float32)
            bd = float(sigma) * 2.0 ** -24 * (A * r + B * np.abs(z)) + np.spacing(np.abs(noisy)).astype(np.float64)
            v = np.where(real, noisy, v)
            bound[:, slot, :] = np.where(real & ~m, bd, 0.0)
        out[:, slot, :] = np.where(m, np.float32(0.0), v)
        masked[:, slot, :] = m
    return (bf16_round(out) if bf16 else out), bound, masked


def splice(x, lens, left, right):
    """[T][PS][P0] -> [T][PS][P0 * (left + right + 1)]: block k of frame t is frame clip(t + k - left, 0, len - 1) (fraction.py);
    frames behind a sequence's end are zero"""
    x = np.asarray(x, np.float32)
    T, PS, P0 = x.shape
    out = np.zeros((T, PS, P0 * (left + right + 1)), np.float32)
    for slot, n in enumerate(int(v) for v in lens):
        for k, off in enumerate(range(-left, right + 1)):
            if n >= 1:
                out[:n, slot, k * P0:(k + 1) * P0] = x[np.clip(np.arange(n) + off, 0, n - 1), slot]
    return out
