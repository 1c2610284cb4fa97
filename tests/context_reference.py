"""numpy / torch restatement of the context layers of include/currennt_hip.h (section Context layers).

With L, R, D the layer's members, B = L + R + 1, P the preceding layer's size and len_s the real frames of slot s:

    out[t][s][b * P + u] = x[clamp(t + (b - L) * D, 0, len_s - 1)][s][u]                       real frames; zeros elsewhere
    dx[ts][s][u]         = sum over b (ascending) of the sum over j (ascending) with clamp(j + (b - L) * D, 0, len_s - 1) == ts
                           of e[j][s][b * P + u]                                               single fp32 additions from +0.0

context_forward / context_backward say it with loops; autograd_context_stack is the fp64 autograd stack of
tests/layernorm_reference.py (its LSTM layer, normalisation, masks and residual sums, imported from there) with a context step
between the layers.  The test nets that tests/test_gpu_context.py uses are here too (CASES, Case)."""
import copy

import numpy as np
import torch

from helpers import random_sequences, random_weights, real_mask
from layernorm_reference import EPS, _ACT, lstm_layer, torch_layer_norm
from residual_reference import ff_delta, flat_weights


def pad_lens(lens, PS):
    return [int(n) for n in lens] + [0] * (PS - len(lens))


def context_forward(x, lens, L, R, D):
    """x: [T][PS][P] -> [T][PS][(L + R + 1) * P] of the same dtype, values copied; zeros on the rows that are no real frames."""
    x = np.asarray(x)
    T, PS, P = x.shape
    B = L + R + 1
    out = np.zeros((T, PS, B * P), x.dtype)
    for s, n in enumerate(pad_lens(lens, PS)):
        for t in range(n):
            for b in range(B):
                ts = min(max(t + (b - L) * D, 0), n - 1)
                out[t, s, b * P:(b + 1) * P] = x[ts, s]
    return out


def context_backward(e, lens, L, R, D):
    """e: [T][PS][(L + R + 1) * P] float32 -> dx [T][PS][P] float32: fp32 additions in the stated order; rows of e that are no real
    frames are never read, rows of dx that are none are zeros."""
    e = np.asarray(e, np.float32)
    T, PS, W = e.shape
    B = L + R + 1
    P = W // B
    assert P * B == W
    dx = np.zeros((T, PS, P), np.float32)
    for s, n in enumerate(pad_lens(lens, PS)):
        for ts in range(n):
            acc = np.zeros(P, np.float32)                      # +0.0f
            for b in range(B):
                for j in range(n):
                    if min(max(j + (b - L) * D, 0), n - 1) == ts:
                        acc = (acc + e[j, s, b * P:(b + 1) * P]).astype(np.float32)
            dx[ts, s] = acc
    return dx


def torch_context(h, lens, L, R, D):
    """The forward rule on a [T][PS][P] tensor, differentiable: index_select per slot and block."""
    T, PS, P = h.shape
    slots = []
    for s, n in enumerate(pad_lens(lens, PS)):
        real = torch.tensor((np.arange(T) < n).astype(np.float64)).reshape(T, 1)
        blocks = []
        for b in range(L + R + 1):
            idx = np.clip(np.arange(T) + (b - L) * D, 0, max(n - 1, 0))
            blocks.append(torch.index_select(h[:, s], 0, torch.tensor(idx, dtype=torch.int64)) * real)
        slots.append(torch.cat(blocks, dim=1))
    return torch.stack(slots, dim=1)


def autograd_context_stack(layers, flat_w, frac, lens, normed=(), marked=(), drop=None, branches=None):
    """The fp64 autograd stack of a network description `layers` (input; hidden lstm / blstm / feedforward_* / context layers;
    softmax; multiclass_classification) on one fraction.  normed / marked / drop as in layernorm_reference.autograd_stack: the
    weighted path of a normed layer reads LN(input) on real frames, then the mask {layer: (keep [N][P] bool, scale)}; a marked
    layer's output is its branch plus its un-normalised input on real frames.  -> loss, posteriors of the real frames, {layer:
    gradient}, {layer: dL/d(outputs) on the real frames} (context layers included)."""
    T, PS = frac["T"], frac["PS"]
    params = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in flat_w.items()}
    lens = pad_lens(lens, PS)
    real = real_mask(frac)
    realm = torch.tensor(real.reshape(T, PS, 1).astype(np.float64))
    drop = drop or {}

    def weighted_input(name, h):
        x = h
        if name in normed:
            x = torch_layer_norm(h, float(np.float32(EPS))) * realm
        if name in drop:
            keep, scale = drop[name]
            x = x * torch.tensor(np.asarray(keep).reshape(T, PS, -1).astype(np.float64) * float(scale))
        return x

    h = torch.tensor(frac["inputs"].reshape(T, PS, -1).astype(np.float64))
    prev, outs = layers[0]["size"], {}
    for d in layers[1:-2]:
        name, kind, size = d["name"], d["type"], d["size"]
        if kind == "context":
            h = torch_context(h, lens, d.get("left", 0), d.get("right", 0), d.get("dilation", 1))
            assert h.shape[2] == size
        else:
            w, x = params[name], weighted_input(name, h)
            if kind in ("lstm", "blstm"):
                b = lstm_layer(x, lens, w, prev, size, kind == "blstm", float(d["bias"]))
            else:
                b = _ACT[kind](x @ w[:size * prev].reshape(size, prev).T + float(d["bias"]) * w[size * prev:])
            if branches is not None:
                branches[name] = b.detach().numpy().reshape(T * PS, -1)[real]
            h = b + h * realm if name in marked else b
        h.retain_grad()
        outs[name] = h
        prev = size
    C, wo = layers[-2]["size"], params[layers[-2]["name"]]
    z = weighted_input(layers[-2]["name"], h) @ wo[:C * prev].reshape(C, prev).T + float(layers[-2]["bias"]) * wo[C * prev:]
    logp = torch.log_softmax(z, dim=2)
    tc = torch.tensor(frac["targetClasses"].reshape(T, PS).astype(np.int64))
    loss = -(logp.gather(2, tc.clamp(min=0).unsqueeze(2)).squeeze(2) * (tc >= 0)).sum()
    loss.backward()
    post = torch.exp(logp).detach().numpy().reshape(-1, C)[real]
    return (float(loss.detach()), post, {k: v.grad.numpy() for k, v in params.items()},
            {k: v.grad.numpy().reshape(T * PS, -1)[real] for k, v in outs.items()})


def stack_results(layers, weights, frac, lens, **kw):
    """autograd_context_stack with the propagated errors as the library's buffers hold them after the backward pass: a feed-forward
    layer's outputErrors are overwritten with act'(branch) * e (FeedForwardLayer.cu:72-79)."""
    branches = {}
    loss, post, grads, errs = autograd_context_stack(layers, flat_weights(weights), frac, lens, branches=branches, **kw)
    for d in layers:
        if d["type"].startswith("feedforward") and d["name"] in errs:
            errs[d["name"]] = ff_delta(d["type"], branches[d["name"]], errs[d["name"]])
    return loss, post, grads, errs


def context_net_desc(P, hidden, C, bias=1.0):
    """hidden: (type, size) tuples, or ("context", (left, right, dilation)) whose size follows from its predecessor."""
    layers = [{"name": "input", "type": "input", "size": P}]
    for i, (t, s) in enumerate(hidden):
        if t == "context":
            L, R, D = s
            layers.append({"name": "context_%d" % i, "type": "context", "size": (L + R + 1) * layers[-1]["size"], "left": L, "right": R, "dilation": D})
        else:
            layers.append({"name": "%s_%d" % (t, i), "type": t, "size": s, "bias": bias})
    layers.append({"name": "output", "type": "softmax", "size": C, "bias": bias})
    layers.append({"name": "postoutput", "type": "multiclass_classification", "size": C})
    return layers


# ---- the test nets: name -> (P, hidden, C, PS, lengths, weight scale, seed, the layers' bias)
CASES = {
    # dummy frames and a pad slot (PSp 4); H 5 against Hp 32: a split -> dense gather and a dense -> split fold; a feed-forward
    # predecessor (act(bias) on dummy rows); offsets of +-6 on sequences of 4 and 2 frames: both clamps hit one frame; L = 0
    "small": (7, [("lstm", 10), ("context", (2, 1, 1)), ("blstm", 10), ("context", (1, 2, 3)), ("feedforward_tanh", 12), ("context", (0, 1, 1)),
                  ("lstm", 6)], 5, 3, [9, 4, 2], 0.3, 51, 1.0),
    # the 16-byte paths, more than one workgroup per launch
    "wide": (13, [("blstm", 64), ("context", (2, 2, 1)), ("feedforward_tanh", 64), ("context", (1, 1, 2)), ("lstm", 64)], 9, 8,
             [17 - (i % 5) for i in range(8)], 0.2, 52, 0.7),
    # the predecessor is the input layer: what input splicing produces
    "from_input": (7, [("context", (2, 3, 1)), ("lstm", 10)], 5, 3, [7, 5, 2], 0.3, 53, 1.0),
    # a follower that drops, normalises and is residual: blstm 6 -> context(1, 1) -> feedforward_tanh 18
    "features": (7, [("blstm", 6), ("context", (1, 1, 1)), ("feedforward_tanh", 18), ("lstm", 8)], 5, 3, [9, 6, 4], 0.3, 54, 1.0),
}


class Case:
    def __init__(self, pkg, which):
        P, hidden, C, PS, lens, wscale, seed, bias = CASES[which]
        rng = np.random.RandomState(seed)
        self.which, self.P, self.hidden, self.C, self.PS, self.lens = which, P, hidden, C, PS, lens
        self.layers = context_net_desc(P, hidden, C, bias=bias)
        self.weights = random_weights(self.layers, rng, wscale)
        self.xs, self.ts = random_sequences(rng, lens, P, C=C)
        self.frac = pkg.make_fraction(self.xs, self.ts, PS)
        self.T, self.N = self.frac["T"], self.frac["T"] * PS
        self._ref = None

    def net(self, pkg, prec, layers=None, weights=None, **kw):
        return pkg.NeuralNetwork(copy.deepcopy(layers or self.layers), weights or self.weights, self.PS, self.T, precision=getattr(pkg, prec), **kw)

    def reference(self):
        """(loss, posteriors, gradients, errors) of the fp64 stack, computed once."""
        if self._ref is None:
            self._ref = stack_results(self.layers, self.weights, self.frac, self.lens)
        return self._ref
