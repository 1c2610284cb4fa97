"""numpy restatement, in float64, of the weight noise of include/currennt_hip.h (section Weight noise).

For the layer with creation index `ordinal` and flat weight index k:

    (w0,w1,w2,w3) = Philox4x32-10(counter = (k >> 2, 0, pass_lo, pass_hi),
                                  key = ((seed_lo + ordinal) mod 2^32, seed_hi ^ 0x6E6F6973))
    pair p = (k & 3) >> 1 uses words (w[2p], w[2p+1]) = (a, b)
    u1 = (2*(a >> 9) + 1) * 2^-24          t = (2*(b >> 9) + 1) * 2^-23
    r  = sqrt(-2 ln u1)                    z = r * (sin(pi t) if k & 1 else cos(pi t))
    n  = sigma * z                         w' = w + n

u1 and t are exact in fp32 and in float64; everything behind them is float64 here and fp32 on the device.

How far the device may be from this (the bound the GPU test uses)
-----------------------------------------------------------------
u = 2^-24 is the unit roundoff of fp32: a correctly rounded operation is off by at most u times its result, and one ulp of a
result x is at most 2u|x|.  The HIP math API documents a maximum error of 1 ulp for logf, 1 ulp for sinpif and 1 ulp for cospif
in single precision (ULP_LOG, ULP_TRIG below); the square root and the multiplications are correctly rounded.

    L~ = logf(u1)            = L (1 + e1),          |e1| <= 2u ULP_LOG
    m  = mul_rn(-2, L~)      exact (a power of two)
    r~ = sqrt_rn(m)          = r sqrt(1 + e1) (1 + e2), |e2| <= u      ->  r~ = r (1 + rho), |rho| <= (ULP_LOG + 1) u
    c~ = sinpif / cospif(t)  = c + dc,              |dc| <= ULP_TRIG ulp(c) <= 2u ULP_TRIG     (|c| <= 1; t is exact)
    z~ = mul_rn(r~, c~)      = (r c + r c rho + r dc)(1 + e3),  |e3| <= u
    n~ = mul_rn(sigma, z~)   = sigma z~ (1 + e4),               |e4| <= u

so, to first order in u,   |n~ - sigma z| <= sigma u ( 2 ULP_TRIG r + (ULP_LOG + 1 + 1 + 1) |z| ).
The test compares against float32(sigma z), which is itself within u |sigma z| of sigma z: one more unit on |z|.  Hence

    |n~ - float32(sigma z)| <= sigma 2^-24 (A r + B |z|),     A = 2 ULP_TRIG = 2,   B = ULP_LOG + 4 = 5,   A + B = 7

(the second-order terms are below 2^-20 of this).  The two sums w + n~ and w + float32(sigma z) are each rounded once more,
which can move them apart by one further ulp of the sum."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dropout_reference import MASK32, bf16_round, philox4x32_10          # noqa: E402,F401

KEY_XOR = 0x6E6F6973                     # "nois": keeps the stream apart from the dropout masks of the same seed
ULP_LOG, ULP_TRIG = 1, 1                 # documented maximum ulp errors of logf and of sinpif / cospif (HIP math API, single precision)
A = 2 * ULP_TRIG
B = ULP_LOG + 4


def key(seed, ordinal):
    seed = int(seed) & (2 ** 64 - 1)
    return ((seed & MASK32) + int(ordinal)) & MASK32, (seed >> 32) ^ KEY_XOR


def words(seed, ordinal, pass_, count):
    """uint32 [ceil(count / 4)][4]: the Philox words of the flat indices 4g .. 4g + 3."""
    pass_ = int(pass_) & (2 ** 64 - 1)
    groups = (int(count) + 3) // 4
    ctr = np.zeros((groups, 4), np.uint32)
    ctr[:, 0] = np.arange(groups, dtype=np.uint32)
    ctr[:, 2] = pass_ & MASK32
    ctr[:, 3] = pass_ >> 32
    return philox4x32_10(ctr, key(seed, ordinal))


def uniforms_of_words(a, b):
    """u1 in (0, 1) and t = 2 u2 in (0, 2) from the two words of a pair; float64, exact."""
    a = np.asarray(a, np.uint32).astype(np.uint64)
    b = np.asarray(b, np.uint32).astype(np.uint64)
    u1 = (2 * (a >> np.uint64(9)) + 1).astype(np.float64) * 2.0 ** -24
    t = (2 * (b >> np.uint64(9)) + 1).astype(np.float64) * 2.0 ** -23
    return u1, t


def uniforms(seed, ordinal, pass_, count):
    """(u1, t) per flat index k < count: index k takes pair (k & 3) >> 1 of its group's words."""
    w = words(seed, ordinal, pass_, count)
    k = np.arange(count)
    pair = (k & 3) >> 1
    return uniforms_of_words(w[k >> 2, 2 * pair], w[k >> 2, 2 * pair + 1])


def gauss(seed, ordinal, pass_, count):
    """(z, r) per flat index, float64: Box-Muller, even k the cosine branch and odd k the sine branch of their pair."""
    u1, t = uniforms(seed, ordinal, pass_, count)
    r = np.sqrt(-2.0 * np.log(u1))
    k = np.arange(count)
    z = r * np.where(k & 1, np.sin(np.pi * t), np.cos(np.pi * t))
    return z, r


def noisy(w, sigma, seed, ordinal, pass_):
    """float32(w + float32(sigma z)), with the bound the device's value must keep to: (w', bound), float32 / float64 arrays."""
    w = np.asarray(w, np.float32)
    sigma = np.float32(sigma)
    z, r = gauss(seed, ordinal, pass_, w.size)
    n32 = (float(sigma) * z).astype(np.float32)
    ref = (w.astype(np.float64) + n32.astype(np.float64)).astype(np.float32)
    bound = float(sigma) * 2.0 ** -24 * (A * r + B * np.abs(z)) + np.spacing(np.abs(ref)).astype(np.float64)
    return ref, bound


def bias_slice(kind, size, prev_size):
    """Where the bias weights lie in a layer's flat vector (LstmLayer.hpp:36-55, FeedForwardLayer.cu:148,160): no backward pass
    reads them, so they never carry noise."""
    if kind in ("lstm", "blstm"):
        return slice(4 * size * prev_size, 4 * size * prev_size + 4 * size)
    return slice(size * prev_size, size * prev_size + size)
