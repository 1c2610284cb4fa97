"""numpy restatement of the dropout mask of include/currennt_hip.h (section Dropout): Philox4x32-10 and keep(n, i).

    (w0,w1,w2,w3) = Philox4x32-10(counter = (i >> 2, n, pass_lo, pass_hi), key = ((seed_lo + ordinal) mod 2^32, seed_hi))
    keep(n, i)    = w[i & 3] >= thr          thr   = (uint32) floor((double)rate * 2^32)
    x'(n, i)      = keep ? x(n, i) * scale : 0    scale = (float)(1.0 / (1.0 - (double)rate))

n = t * PS + ps is the frame and i the unit of the preceding layer, both in the reference layout."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: uint32 array [..., 4]; key: two uint32 words (scalars or arrays that broadcast) -> uint32 array [..., 4]."""
    c = [np.asarray(counter)[..., k].astype(np.uint64) for k in range(4)]
    k0 = np.asarray(key[0], np.uint64) & np.uint64(MASK32)
    k1 = np.asarray(key[1], np.uint64) & np.uint64(MASK32)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & m32, (p0 >> s32) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + np.uint64(W0)) & m32
        k1 = (k1 + np.uint64(W1)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(rate):
    return int(np.floor(float(np.float32(rate)) * 4294967296.0))


def scale(rate):
    return np.float32(1.0 / (1.0 - float(np.float32(rate))))


def keep(seed, ordinal, pass_, N, P, rate):
    """Boolean [N][P]: which (frame, unit) pairs the layer with creation index `ordinal` keeps."""
    seed, pass_ = int(seed) & (2 ** 64 - 1), int(pass_) & (2 ** 64 - 1)
    groups = (P + 3) // 4
    ctr = np.zeros((N, groups, 4), np.uint32)
    ctr[..., 0] = np.arange(groups, dtype=np.uint32)[None, :]
    ctr[..., 1] = np.arange(N, dtype=np.uint32)[:, None]
    ctr[..., 2] = pass_ & MASK32
    ctr[..., 3] = pass_ >> 32
    words = philox4x32_10(ctr, (((seed & MASK32) + int(ordinal)) & MASK32, seed >> 32))
    return words.reshape(N, groups * 4)[:, :P] >= np.uint32(threshold(rate))


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16) << np.uint64(16)
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def apply(x, mask, rate, bf16=False):
    """x' of the header: one fp32 multiplication where the mask keeps (rounded to bf16 in that mode), +0 elsewhere."""
    y = np.where(mask, np.asarray(x, np.float32) * scale(rate), np.float32(0.0)).astype(np.float32)
    return bf16_round(y) if bf16 else y
