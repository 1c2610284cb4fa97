"""CPU: the numpy restatement of decoupled weight decay (tests/decay_reference.py) against torch's optimizers in float64, and its
own invariants in float32: exempt and pad entries keep their bits, decay 0 is the plain step."""
import os
import re

import numpy as np
import torch

import adam_reference as AR
import clip_reference as CR
import decay_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cn_ctx_set_weight_decay", "cn_ctx_get_weight_decay")
L_, P_ = 6, 5                    # a small lstm layer: 6 units, 5 inputs -> 120 | 24 | 144 + 18 = 306 weights
LR, WD, MOM = 1e-2, 0.1, 0.9
# Largest relative difference |ours - torch| / max(|torch|, 1e-300) seen over the 5 steps in float64 (this file, torch 2.x CPU):
MEASURED_ADAMW = 2.46e-15
MEASURED_SGD = 3.85e-15


def lstm_vector(rng, dtype):
    n = DR.weight_count("lstm", L_, P_)
    assert n == 306
    mask = DR.decay_mask(n, DR.decayed_ranges("lstm", L_, P_))
    return dtype(rng.uniform(-0.5, 0.5, n)), mask


def rel_diff(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def torch_groups(w, mask):
    """two parameters: the entries that decay, and the bias / peephole entries in a group with weight_decay = 0"""
    pd = torch.tensor(w[mask], dtype=torch.float64, requires_grad=True)
    pe = torch.tensor(w[~mask], dtype=torch.float64, requires_grad=True)
    return pd, pe


def test_ranges_table():
    assert DR.decayed_ranges("lstm", 8, 39) == [(0, 1248), (1280, 1536)]                    # 4*8*39 | 32 bias | 4*8*8 | 24 peepholes
    assert DR.decayed_ranges("blstm", 12, 8) == [(0, 384), (432, 720)]                      # H = 6: 4*12*6 recurrent weights
    assert DR.decayed_ranges("softmax", 5, 12) == [(0, 60)]
    assert DR.decayed_ranges("feedforward_tanh", 6, 8) == [(0, 48)]
    assert DR.weight_count("lstm", 8, 39) == 1560 and DR.weight_count("blstm", 12, 8) == 756 and DR.weight_count("softmax", 5, 12) == 65
    m = DR.decay_mask(1560, DR.decayed_ranges("lstm", 8, 39))
    assert m.sum() == 1248 + 256 and not m[1248:1280].any() and not m[1536:].any()


def test_float64_mode_agrees_with_torch_adamw():
    """5 steps on a small lstm layer's vector in float64 against torch.optim.AdamW (bias and peephole entries in a group with
    weight_decay = 0).  Largest relative difference measured: 2.46e-15 (MEASURED_ADAMW); the bound asserted is ten times that."""
    rng = np.random.RandomState(41)
    w, mask = lstm_vector(rng, np.float64)
    pd, pe = torch_groups(w, mask)
    opt = torch.optim.AdamW([{"params": [pd], "weight_decay": WD}, {"params": [pe], "weight_decay": 0.0}], lr=LR, betas=(0.9, 0.999), eps=1e-8)
    m, v = np.zeros_like(w), np.zeros_like(w)
    worst = 0.0
    for step in range(1, 6):
        g = rng.uniform(-1, 1, w.size)
        pd.grad = torch.tensor(g[mask]); pe.grad = torch.tensor(g[~mask])
        opt.step()
        w, m, v = DR.decay_adam_step(w, g, m, v, [(0, w.size, LR)], WD, mask, step=step, dtype=np.float64)
        worst = max(worst, rel_diff(w[mask], pd.detach().numpy()), rel_diff(w[~mask], pe.detach().numpy()))
    print("largest relative difference against torch.optim.AdamW: %.3g" % worst)
    assert worst <= 10 * MEASURED_ADAMW, worst


def test_float64_mode_agrees_with_torch_sgd_behind_the_shrink():
    """5 steps in float64 against p.mul_(1 - lr * wd) followed by torch.optim.SGD(momentum) (torch's momentum buffer b relates to
    the delta as d = -lr * b).  Largest relative difference measured: 3.85e-15 (MEASURED_SGD); the bound is ten times that."""
    rng = np.random.RandomState(42)
    w, mask = lstm_vector(rng, np.float64)
    pd, pe = torch_groups(w, mask)
    opt = torch.optim.SGD([pd, pe], lr=LR, momentum=MOM)
    d = np.zeros_like(w)
    worst = 0.0
    for step in range(1, 6):
        g = rng.uniform(-1, 1, w.size)
        pd.grad = torch.tensor(g[mask]); pe.grad = torch.tensor(g[~mask])
        with torch.no_grad():
            pd.mul_(1 - LR * WD)
        opt.step()
        w, d = DR.decay_sgd_step(w, g, d, LR, MOM, WD, mask, dtype=np.float64)
        worst = max(worst, rel_diff(w[mask], pd.detach().numpy()), rel_diff(w[~mask], pe.detach().numpy()))
    print("largest relative difference against torch.optim.SGD: %.3g" % worst)
    assert worst <= 10 * MEASURED_SGD, worst


def test_exempt_and_pad_entries_keep_their_bits():
    """fp32: with a zero gradient and no momentum the step is the decay part alone; bias, peephole and pad entries are bit-
    unchanged and every other entry is w - ld * w"""
    rng = np.random.RandomState(43)
    n = DR.weight_count("lstm", L_, P_)
    total = n + 2                                                         # two pad entries behind the layer
    mask = DR.decay_mask(total, DR.decayed_ranges("lstm", L_, P_))
    w = np.float32(rng.uniform(-0.5, 0.5, total))
    w[5] = np.float32(1e-42)                                              # a denormal stays one
    z = np.zeros(total, np.float32)
    w1, d1 = DR.decay_sgd_step(w, z, z, LR, 0.0, 0.5, mask)
    assert w1.dtype == np.float32
    assert w1[~mask].tobytes() == w[~mask].tobytes() and (~mask).sum() == 24 + 18 + 2
    ld = np.float32(float(np.float32(LR)) * 0.5)
    assert w1[mask].tobytes() == (w[mask] - ld * w[mask]).astype(np.float32).tobytes()
    assert np.all(w1[mask] != w[mask]) and w1[5] != 0
    w2, _, _ = DR.decay_adam_step(w, z, z, z, [(0, n, LR)], 0.5, mask)
    assert w2[~mask].tobytes() == w[~mask].tobytes() and w2[:n][mask[:n]].tobytes() == w1[mask].tobytes()


def test_decay_zero_is_the_plain_step_bit_for_bit():
    rng = np.random.RandomState(44)
    w, mask = lstm_vector(rng, np.float32)
    g = AR.test_gradients(rng, w.size)
    d = np.float32(rng.uniform(-1e-3, 1e-3, w.size))
    v = np.float32(rng.uniform(0, 1e-3, w.size))
    a = DR.decay_sgd_step(w, g, d, LR, MOM, 0.0, mask)
    b = CR.sgd_step(w, g, d, LR, MOM)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a = DR.decay_adam_step(w, g, d, v, [(0, w.size, LR)], 0.0, mask, step=3)
    b = AR.adam_step(w, g, d, v, LR, step=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a = DR.clip_decay_sgd_step(w, g, d, LR, MOM, 0.0, mask, 0.5)
    b = CR.clip_sgd_step(w, g, d, LR, MOM, 0.5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:2], b[:2])) and a[4] == b[4]
    a = DR.clip_decay_adam_step(w, g, d, v, [(0, w.size, LR)], 0.0, mask, 0.5, step=2)
    b = CR.clip_adam_step(w, g, d, v, [(0, w.size, LR)], 0.5, step=2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def test_clipping_scales_the_gradient_and_not_the_decay_term():
    rng = np.random.RandomState(45)
    w, mask = lstm_vector(rng, np.float32)
    g = AR.test_gradients(rng, w.size)
    z = np.zeros(w.size, np.float32)
    w1, d1, norm, scale, skip = DR.clip_decay_sgd_step(w, g, z, LR, 0.0, WD, mask, 0.25)
    assert not skip and scale is not None and scale < 1
    w0 = DR.decay_weights(w, mask, LR, WD)
    assert w1.tobytes() == (w0 - np.float32(LR) * (scale * g)).astype(np.float32).tobytes()
    g[3] = np.inf
    w2, d2, _, _, skip = DR.clip_decay_sgd_step(w, g, z, LR, 0.0, WD, mask, 0.25)
    assert skip and w2.tobytes() == w.tobytes() and d2.tobytes() == z.tobytes()          # a skipped step decays nothing


def test_new_symbols_are_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    assert "---- Weight decay" in header and "Loshchilov & Hutter 2019" in header
    assert header.index("---- Gradient clipping") < header.index("---- Weight decay")
    assert re.search(r"\bint\s+cn_ctx_set_weight_decay\(cn_ctx \*ctx, float decay\);", header)
    assert re.search(r"\bint\s+cn_ctx_get_weight_decay\(const cn_ctx \*ctx, float \*decay\);", header)
    for sym in NEW_SYMBOLS:
        assert sym in pkg.binding.EXPORTS
    assert max(pkg.binding.EXPORTS.index(s) for s in NEW_SYMBOLS) < pkg.binding.EXPORTS.index("cn_adam_update")
    for name in ("set_weight_decay", "weight_decay"):
        assert hasattr(pkg.NeuralNetwork, name)
