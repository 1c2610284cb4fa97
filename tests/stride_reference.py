"""numpy / torch restatement of the strided context layers of include/currennt_hip.h (section Strided context layers).

With L, R, D, S the layer's members, B = L + R + 1, P the preceding layer's size, len_s the real frames of slot s in the parent
time axis and n_s = ceil(len_s / S) those of the layer's own:

    out[j][s][b * P + u] = x[clamp(S * j + (b - L) * D, 0, len_s - 1)][s][u]                  j < n_s; zeros elsewhere
    dx[ts][s][u]         = sum over b (ascending) of the sum over j < n_s (ascending) with clamp(S * j + (b - L) * D, 0, len_s - 1)
                           == ts of e[j][s][b * P + u]                                         single fp32 additions from +0.0

strided_forward / strided_backward say it with loops, derived_pattern_types / derived_targets state the new axis, and
autograd_stride_stack is the fp64 autograd stack of tests/context_reference.py (its LSTM layer, normalisation, masks and residual
sums, imported from there) in which a strided layer changes the number of steps of everything behind it.  The test nets that
tests/test_gpu_stride.py uses are here too (CASES, Case)."""
import copy

import numpy as np
import torch

from context_reference import pad_lens
from helpers import random_sequences, random_weights
from layernorm_reference import EPS, _ACT, lstm_layer, torch_layer_norm
from residual_reference import ff_delta, flat_weights

NONE, FIRST, NORMAL, LAST = 0, 1, 2, 3


def ceil_div(a, b):
    return -(-int(a) // int(b))


def strided_lengths(lens, S):
    return [ceil_div(n, S) for n in lens]


def strided_forward(x, lens, L, R, D, S):
    """x: [T][PS][P] -> [ceil(T / S)][PS][(L + R + 1) * P] of the same dtype, values copied; zeros on the rows j >= n_s."""
    x = np.asarray(x)
    T, PS, P = x.shape
    B = L + R + 1
    out = np.zeros((ceil_div(T, S), PS, B * P), x.dtype)
    for s, n in enumerate(pad_lens(lens, PS)):
        for j in range(ceil_div(n, S)):
            for b in range(B):
                ts = min(max(S * j + (b - L) * D, 0), n - 1)
                out[j, s, b * P:(b + 1) * P] = x[ts, s]
    return out


def strided_backward(e, lens, T, L, R, D, S):
    """e: [ceil(T / S)][PS][(L + R + 1) * P] float32 -> dx [T][PS][P] float32: fp32 additions in the stated order; rows of e that
    are no real frames are never read; a parent frame nobody reads and every row that is no real frame are +0.0."""
    e = np.asarray(e, np.float32)
    Tn, PS, W = e.shape
    assert Tn == ceil_div(T, S)
    B = L + R + 1
    P = W // B
    assert P * B == W
    dx = np.zeros((T, PS, P), np.float32)
    for s, n in enumerate(pad_lens(lens, PS)):
        for ts in range(n):
            acc = np.zeros(P, np.float32)                      # +0.0f
            for b in range(B):
                for j in range(ceil_div(n, S)):
                    if min(max(S * j + (b - L) * D, 0), n - 1) == ts:
                        acc = (acc + e[j, s, b * P:(b + 1) * P]).astype(np.float32)
            dx[ts, s] = acc
    return dx


def unread_frames(lens, T, PS, L, R, D, S):
    """Boolean [T][PS]: real parent frames that no (b, j) reads."""
    read = np.zeros((T, PS), bool)
    for s, n in enumerate(pad_lens(lens, PS)):
        for j in range(ceil_div(n, S)):
            for b in range(L + R + 1):
                read[min(max(S * j + (b - L) * D, 0), n - 1), s] = True
    real = np.arange(T)[:, None] < np.asarray(pad_lens(lens, PS))[None, :]
    return real & ~read


def derived_pattern_types(lens, T, PS, S):
    """[ceil(T / S)][PS] int8: FIRST for j = 0, LAST for j = n_s - 1 > 0, NORMAL between, NONE for j >= n_s and empty slots."""
    pat = np.full((ceil_div(T, S), PS), NONE, np.int8)
    for s, n in enumerate(pad_lens(lens, PS)):
        m = ceil_div(n, S)
        pat[:m, s] = NORMAL
        if m > 0:
            pat[0, s] = FIRST
        if m > 1:
            pat[m - 1, s] = LAST
    return pat


def derived_targets(t, lens, S):
    """t: [T][PS] classes or [T][PS][W] target rows of the parent axis -> those of parent row S * j for j < n_s; -1 (an integer
    array) / zero rows elsewhere."""
    t = np.asarray(t)
    T, PS = t.shape[:2]
    out = np.full((ceil_div(T, S),) + t.shape[1:], -1 if np.issubdtype(t.dtype, np.integer) else 0, t.dtype)
    for s, n in enumerate(pad_lens(lens, PS)):
        for j in range(ceil_div(n, S)):
            out[j, s] = t[S * j, s]
    return out


def torch_strided(h, lens, L, R, D, S):
    """The forward rule on a [T][PS][P] tensor, differentiable: index_select per slot and block."""
    T, PS, P = h.shape
    Tn = ceil_div(T, S)
    slots = []
    for s, n in enumerate(pad_lens(lens, PS)):
        real = torch.tensor((np.arange(Tn) < ceil_div(n, S)).astype(np.float64)).reshape(Tn, 1)
        blocks = []
        for b in range(L + R + 1):
            idx = np.clip(S * np.arange(Tn) + (b - L) * D, 0, max(n - 1, 0))
            blocks.append(torch.index_select(h[:, s], 0, torch.tensor(idx, dtype=torch.int64)) * real)
        slots.append(torch.cat(blocks, dim=1))
    return torch.stack(slots, dim=1)


def axes_of(layers, lens, T):
    """{layer name: (T, lens, rate)} of the time axis every layer's rows lie in."""
    out, rate = {}, 1
    for d in layers:
        if d["type"] == "context":
            rate *= d.get("stride", 1)
        out[d["name"]] = (ceil_div(T, rate), strided_lengths(lens, rate), rate)
    return out


def real_of(T, lens, PS):
    return (np.arange(T)[:, None] < np.asarray(pad_lens(lens, PS))[None, :]).reshape(-1)


def autograd_stride_stack(layers, flat_w, frac, lens, normed=(), marked=(), drop=None, branches=None, loss_fn=None):
    """The fp64 autograd stack of context_reference.autograd_context_stack with rate changes: a context layer with a "stride"
    hands every layer behind it ceil(T / S) steps and ceil(len_s / S) real frames per slot, and the loss is taken over the output
    layer's frames with the derived targets.  drop: {layer: (keep [N'][P] bool in the layer's own frame index, scale)}.
    loss_fn (default: the multiclass loss on the softmax of z): (z [T'][PS][C] tensor, T', lens', rate) -> (loss tensor, outputs).
    -> loss, outputs on the real frames of the output layer's axis, {layer: gradient}, {layer: dL/d(outputs) on the real frames of
    that layer's axis} (context layers included)."""
    T, PS = frac["T"], frac["PS"]
    params = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in flat_w.items()}
    lens = [int(n) for n in lens]
    drop = drop or {}
    rate = 1

    def realm():
        return torch.tensor(real_of(T, lens, PS).reshape(T, PS, 1).astype(np.float64))

    def weighted_input(name, h):
        x = h
        if name in normed:
            x = torch_layer_norm(h, float(np.float32(EPS))) * realm()
        if name in drop:
            keep, scale = drop[name]
            x = x * torch.tensor(np.asarray(keep).reshape(T, PS, -1).astype(np.float64) * float(scale))
        return x

    h = torch.tensor(frac["inputs"].reshape(T, PS, -1).astype(np.float64))
    prev, outs, reals = layers[0]["size"], {}, {}
    for d in layers[1:-2]:
        name, kind, size = d["name"], d["type"], d["size"]
        if kind == "context":
            S = d.get("stride", 1)
            h = torch_strided(h, lens, d.get("left", 0), d.get("right", 0), d.get("dilation", 1), S)
            T, lens, rate = ceil_div(T, S), strided_lengths(lens, S), rate * S
            assert h.shape[0] == T and h.shape[2] == size
        else:
            w, x = params[name], weighted_input(name, h)
            if kind in ("lstm", "blstm"):
                b = lstm_layer(x, pad_lens(lens, PS), w, prev, size, kind == "blstm", float(d["bias"]))
            else:
                b = _ACT[kind](x @ w[:size * prev].reshape(size, prev).T + float(d["bias"]) * w[size * prev:])
            if branches is not None:
                branches[name] = b.detach().numpy().reshape(T * PS, -1)[real_of(T, lens, PS)]
            h = b + h * realm() if name in marked else b
        if h.requires_grad:                  # (a context layer behind the input layer takes no errors)
            h.retain_grad()
            outs[name], reals[name] = h, real_of(T, lens, PS)
        prev = size
    C, wo = layers[-2]["size"], params[layers[-2]["name"]]
    z = weighted_input(layers[-2]["name"], h) @ wo[:C * prev].reshape(C, prev).T + float(layers[-2]["bias"]) * wo[C * prev:]
    real = real_of(T, lens, PS)
    if loss_fn is None:
        logp = torch.log_softmax(z, dim=2)
        tc = derived_targets(frac["targetClasses"].reshape(frac["T"], PS), [int(n) for n in frac["seqLengths"]], rate)
        tc = torch.tensor(tc.astype(np.int64))
        loss = -(logp.gather(2, tc.clamp(min=0).unsqueeze(2)).squeeze(2) * (tc >= 0)).sum()
        y = torch.exp(logp)
    else:
        loss, y = loss_fn(z, T, lens, rate)
    loss.backward()
    post = y.detach().numpy().reshape(-1, C)[real]
    return (float(loss.detach()), post, {k: v.grad.numpy() for k, v in params.items()},
            {k: v.grad.numpy().reshape(len(reals[k]), -1)[reals[k]] for k, v in outs.items()})


def stack_results(layers, weights, frac, lens, **kw):
    """autograd_stride_stack with the propagated errors as the library's buffers hold them after the backward pass: a feed-forward
    layer's outputErrors are overwritten with act'(branch) * e (FeedForwardLayer.cu:72-79)."""
    branches = {}
    loss, post, grads, errs = autograd_stride_stack(layers, flat_weights(weights), frac, lens, branches=branches, **kw)
    for d in layers:
        if d["type"].startswith("feedforward") and d["name"] in errs:
            errs[d["name"]] = ff_delta(d["type"], branches[d["name"]], errs[d["name"]])
    return loss, post, grads, errs


def stride_net_desc(P, hidden, C, bias=1.0, post="multiclass_classification", out_type="softmax"):
    """hidden: (type, size) tuples, or ("context", (left, right, dilation, stride)) whose size follows from its predecessor."""
    layers = [{"name": "input", "type": "input", "size": P}]
    for i, (t, s) in enumerate(hidden):
        if t == "context":
            L, R, D, S = s
            layers.append({"name": "context_%d" % i, "type": "context", "size": (L + R + 1) * layers[-1]["size"], "left": L, "right": R, "dilation": D,
                           "stride": S})
        else:
            layers.append({"name": "%s_%d" % (t, i), "type": t, "size": s, "bias": bias})
    layers.append({"name": "output", "type": out_type, "size": C, "bias": bias})
    layers.append({"name": "postoutput", "type": post, "size": C})
    return layers


# ---- the test nets: name -> (P, hidden, C, PS, lengths, weight scale, seed, the layers' bias)
CASES = {
    # PS 3 (PSp 4: a pad slot); /2 gives 7, 3, 1 frames and /3 behind it 3, 1, 1: a length that is a multiple of S and one that is
    # not, a one-frame sequence (FIRST only, both clamps on one frame), dummy rows in every axis; H 5 against Hp 32: the scalar
    # path, split -> dense and dense -> split
    "small": (7, [("lstm", 10), ("context", (1, 1, 1, 2)), ("blstm", 10), ("context", (0, 1, 1, 3)), ("feedforward_tanh", 12), ("lstm", 6)],
              5, 3, [13, 6, 1], 0.3, 61, 1.0),
    # the 16-byte paths, more than one workgroup per launch; both folds leave parent frames that no output frame reads
    "wide": (13, [("blstm", 64), ("context", (1, 1, 2, 2)), ("feedforward_tanh", 64), ("context", (0, 0, 1, 2)), ("lstm", 64)], 9, 8,
             [17 - (i % 5) for i in range(8)], 0.2, 62, 0.7),
    # the predecessor is the input layer: what input splicing with a frame skip produces
    "from_input": (7, [("context", (2, 3, 1, 2)), ("lstm", 10)], 5, 3, [7, 5, 2], 0.3, 63, 1.0),
    # a follower that drops, normalises and is residual (size B * P) behind a strided layer
    "features": (7, [("blstm", 6), ("context", (1, 1, 1, 2)), ("feedforward_tanh", 18), ("lstm", 8)], 5, 3, [9, 6, 4], 0.3, 64, 1.0),
}


class Case:
    def __init__(self, pkg, which, lens=None, seed=None):
        P, hidden, C, PS, lens0, wscale, seed0, bias = CASES[which]
        lens = lens0 if lens is None else lens
        self.which, self.P, self.hidden, self.C, self.PS, self.lens = which, P, hidden, C, PS, lens
        self.layers = stride_net_desc(P, hidden, C, bias=bias)
        self.weights = random_weights(self.layers, np.random.RandomState(seed0), wscale)     # (the same weights whatever the fraction)
        self.xs, self.ts = random_sequences(np.random.RandomState(seed0 + 1000 if seed is None else seed), lens, P, C=C)
        self.frac = pkg.make_fraction(self.xs, self.ts, PS)
        self.T, self.N = self.frac["T"], self.frac["T"] * PS
        self.maxT = max(lens0)
        self.axes = axes_of(self.layers, lens, self.T)
        self._ref = None

    def net(self, pkg, prec, layers=None, weights=None, **kw):
        return pkg.NeuralNetwork(copy.deepcopy(layers or self.layers), weights or self.weights, self.PS, self.maxT, precision=getattr(pkg, prec), **kw)

    def real(self, name):
        """Boolean [T' * PS] of the axis layer `name` runs on."""
        T, lens, _ = self.axes[name]
        return real_of(T, lens, self.PS)

    def reference(self):
        """(loss, posteriors, gradients, errors) of the fp64 stack, computed once."""
        if self._ref is None:
            self._ref = stack_results(self.layers, self.weights, self.frac, self.lens)
        return self._ref
