"""numpy / torch restatement of the layer normalization of include/currennt_hip.h (section Layer normalization).

    mean = (1/P) sum x_i      var = (1/P) sum (x_i - mean)^2      rstd = 1 / sqrt(var + eps)      xn_i = (x_i - mean) * rstd
    dx_i = rstd * (g_i - mean(g) - xn_i * mean(g * xn))

on real frames, zeros on every other row; no gain, no bias.  layer_norm_rule / layer_norm_backward say it in float64 numpy;
autograd_stack is the fp64 autograd stack of tests/residual_reference.py extended by `normed` (layer names): a normed layer's
weighted path reads LN(input) on real frames, then the dropout mask if one is given, and a residual layer's skip path takes the
un-normalised input.  With bf16=True the same stack models CN_PREC_BF16's operand roundings with straight-through bf16_round.  The
test nets that tests/test_layernorm_reference.py (CPU) and tests/test_gpu_layernorm.py share are here too (CASES, Case)."""
import copy

import numpy as np
import torch

from dropout_reference import bf16_round
from helpers import net_desc, random_sequences, random_weights, real_mask
from residual_reference import ff_delta, flat_weights
from test_oracle_autograd import tanh_, sig

EPS = 1e-5


def layer_norm_rule(x, real, eps=EPS):
    """x: [N][P] float32 operand values; real: bool [N] -> (xn, mean, rstd) in float64, xn = 0 on the rows that are not real."""
    x = np.asarray(x, np.float32).astype(np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    rho = 1.0 / np.sqrt(var + float(np.float32(eps)))
    xn = np.where(np.asarray(real, bool)[:, None], (x - mu) * rho, 0.0)
    return xn, mu, rho


def layer_norm_bound(xn, mu, rho, bf16=False):
    """|got - xn| may reach: three fp32 roundings on xn and one on the mean (which enters as |mean| * rstd * 2^-24), with a 4/3
    and a 4x margin; in bf16 half an ulp of the operand type with room for a near-tie."""
    b = 2.0 ** -22 * (np.abs(xn) + np.abs(mu) * rho) + 1e-30
    return b + 2.0 ** -8 * np.abs(xn) if bf16 else b


def layer_norm_backward(g, xn, rho):
    """dL/dx [N][P] from g = dL/d xn, the normalised rows and their rstd [N][1] (float64)."""
    g, xn = np.asarray(g, np.float64), np.asarray(xn, np.float64)
    return rho * (g - g.mean(axis=1, keepdims=True) - xn * (g * xn).mean(axis=1, keepdims=True))


def torch_layer_norm(h, eps=EPS):
    mu = h.mean(dim=-1, keepdim=True)
    var = ((h - mu) ** 2).mean(dim=-1, keepdim=True)
    return (h - mu) / torch.sqrt(var + eps)


def _clip1(t):
    """The value t; its gradient is clipped to [-1, 1] where it leaves t (limitedError.cuh:31-34)."""
    if t.requires_grad:
        t.register_hook(lambda g: g.clamp(-1.0, 1.0))
    return t


def lstm_layer(x, lens, w, P, L, bidir, bias):
    """lstm_layer of tests/test_oracle_autograd.py with the delta clip of the reference's backward pass (ComputeBlockErrorsFn,
    LstmLayer.cu:262-285; csrc/cn_lstm_device.h states it): the four gate deltas are clipped to [-1, 1] when stored, and the
    stored ones feed the weight gradients, the recurrent and input products and the carried input / forget gate terms; the
    cell state error is not clipped and takes the output gate's peephole term from the unclipped delta.  The plain stack leaves
    the clip out because nothing there reaches it; behind a normalisation the handed-back errors are 1 / std times larger and
    do.  x: [T][PS][P] float64 tensor; returns [T][PS][L]."""
    T, PS, _ = x.shape
    dirs = 2 if bidir else 1
    H = L // dirs
    Win = w[:4 * L * P].reshape(4, dirs, H, P)
    Wb = w[4 * L * P:4 * L * (P + 1)].reshape(4, dirs, H)
    Wr = w[4 * L * (P + 1):4 * L * (P + 1) + 4 * L * H].reshape(4, dirs, H, H)
    Wp = w[4 * L * (P + 1) + 4 * L * H:].reshape(3, dirs, H)
    outs = []
    for d in range(dirs):
        ys = [None] * T
        y_prev = torch.zeros(PS, H, dtype=torch.float64)
        c_prev = torch.zeros(PS, H, dtype=torch.float64)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            a = [x[t] @ Win[g, d].T + y_prev @ Wr[g, d].T + bias * Wb[g, d] for g in range(4)]
            n = tanh_(_clip1(a[0]))
            i = sig(_clip1(a[1] + Wp[0, d] * c_prev))
            f = sig(_clip1(a[2] + Wp[1, d] * c_prev))
            c = n * i + f * c_prev
            # the output gate's peephole term Wp c: the weight's gradient from the clipped delta, the cell state's from the unclipped
            peep = _clip1(Wp[2, d] * c.detach()) + (Wp[2, d].detach() * c - (Wp[2, d] * c).detach())
            o = sig(_clip1(a[3]) + peep)
            y = tanh_(c) * o
            m = torch.tensor([[1.0 if t < ln else 0.0] for ln in lens], dtype=torch.float64)
            y, c = y * m, c * m          # dummy slots: output 0, state 0
            ys[t] = y
            y_prev, c_prev = y, c
        outs.append(torch.stack(ys))
    return torch.cat(outs, dim=2)


def st_bf16(t):
    """bf16_round with a straight-through gradient."""
    r = torch.tensor(bf16_round(t.detach().numpy().astype(np.float32)).astype(np.float64))
    return t + (r - t).detach()


_ACT = {"feedforward_tanh": tanh_, "feedforward_logistic": sig, "feedforward_identity": lambda v: v}


def autograd_stack(layers, flat_w, frac, lens, normed=(), marked=(), eps=None, drop=None, affine=None, bf16=False, branches=None):
    """The fp64 autograd stack of a network description `layers` (input, hidden lstm / blstm / feedforward_* layers, softmax,
    multiclass_classification; every bias the description's) on one fraction.  normed: names of the layers whose weighted path
    reads LN(input) on real frames (the softmax layer may be one); marked: names of the residual layers (out = branch + the
    un-normalised input on real frames); eps: {layer: eps}, default 1e-5; drop: {layer: (keep [N][P] bool, scale)}, applied
    behind the normalisation; affine: {layer: (gamma [P], beta [P])}, a gain and bias on the normalised copy (the library has
    none: for the absorption identity).  bf16: straight-through bf16 rounding of the inputs, every weight, every layer output as
    its followers read it, every residual sum and every normalised copy.  -> loss, posteriors of the real frames, {layer:
    gradient}, {layer: dL/d(outputs) on the real frames}.  branches (a dict, optional) receives {layer: the branch output on the
    real frames}."""
    T, PS = frac["T"], frac["PS"]
    rnd = st_bf16 if bf16 else (lambda t: t)
    params = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in flat_w.items()}
    lens = list(lens) + [0] * (PS - len(lens))
    real = real_mask(frac)
    realm = torch.tensor(real.reshape(T, PS, 1).astype(np.float64))
    eps, drop, affine = eps or {}, drop or {}, affine or {}

    def weighted_input(name, h):
        x = h
        if name in normed:
            x = rnd(torch_layer_norm(h, float(np.float32(eps.get(name, EPS)))) * realm)
            if name in affine:
                x = (x * torch.tensor(affine[name][0]) + torch.tensor(affine[name][1])) * realm
        if name in drop:
            keep, scale = drop[name]
            x = rnd(x * torch.tensor(np.asarray(keep).reshape(T, PS, -1).astype(np.float64) * float(scale)))
        return x

    h = rnd(torch.tensor(frac["inputs"].reshape(T, PS, -1).astype(np.float64)))
    prev, outs = layers[0]["size"], {}
    for d in layers[1:-2]:
        name, kind, size, w = d["name"], d["type"], d["size"], rnd(params[d["name"]])
        x = weighted_input(name, h)
        if kind in ("lstm", "blstm"):
            b = lstm_layer(x, lens, w, prev, size, kind == "blstm", float(d["bias"]))
        else:
            b = _ACT[kind](x @ w[:size * prev].reshape(size, prev).T + float(d["bias"]) * w[size * prev:])
        if branches is not None:
            branches[name] = b.detach().numpy().reshape(T * PS, -1)[real]
        h = rnd(rnd(b) + h * realm) if name in marked else rnd(b)
        h.retain_grad()
        outs[name] = h
        prev = size
    C, wo = layers[-2]["size"], rnd(params[layers[-2]["name"]])
    z = weighted_input(layers[-2]["name"], h) @ wo[:C * prev].reshape(C, prev).T + float(layers[-2]["bias"]) * wo[C * prev:]
    logp = torch.log_softmax(z, dim=2)
    tc = torch.tensor(frac["targetClasses"].reshape(T, PS).astype(np.int64))
    loss = -(logp.gather(2, tc.clamp(min=0).unsqueeze(2)).squeeze(2) * (tc >= 0)).sum()
    loss.backward()
    post = torch.exp(logp).detach().numpy().reshape(-1, C)[real]
    return (float(loss.detach()), post, {k: v.grad.numpy() for k, v in params.items()},
            {k: v.grad.numpy().reshape(T * PS, -1)[real] for k, v in outs.items()})


def stack_results(layers, weights, frac, lens, **kw):
    """autograd_stack with the propagated errors as the library's buffers hold them after the backward pass: a feed-forward layer's
    outputErrors are overwritten with act'(branch) * e (FeedForwardLayer.cu:72-79)."""
    branches = {}
    loss, post, grads, errs = autograd_stack(layers, flat_weights(weights), frac, lens, branches=branches, **kw)
    for d in layers:
        if d["type"].startswith("feedforward") and d["name"] in errs:
            errs[d["name"]] = ff_delta(d["type"], branches[d["name"]], errs[d["name"]])
    return loss, post, grads, errs


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


# ---- the test nets: name -> (P, hidden, indices of the normed hidden layers, output layer normed, C, PS, lengths, weight scale, seed,
# the layers' bias)
CASES = {
    # a pad slot (PSp 4), dummy frames, H 5 against Hp 32, dense and split predecessors
    "small": (7, [("lstm", 10), ("blstm", 10), ("feedforward_tanh", 10), ("lstm", 10)], (1, 2, 3), True, 5, 3, [9, 6, 4], 0.3, 41, 1.0),
    # more than one workgroup per launch (the "wide" net of tests/test_gpu_residual.py, bias 0.7)
    "wide": (13, [("blstm", 64), ("feedforward_tanh", 64), ("lstm", 64)], (1, 2), True, 9, 8, [17 - (i % 5) for i in range(8)], 0.2, 42, 0.7),
    # P = 250 with H 125 / Hp 128: a row that is no multiple of 64 and straddles the direction pad
    "headline": (39, [("blstm", 250), ("blstm", 250)], (1,), True, 20, 4, [24, 24, 17, 9], 0.1, 43, 1.0),
    # the predecessor is the input layer
    "first": (7, [("lstm", 10), ("blstm", 10)], (0, 1), True, 5, 3, [9, 6, 4], 0.3, 45, 1.0),
    # more than one trip of the row loop (Pp 1120: five trips of 256 fp32 columns, three of 512 bf16 columns)
    "long row": (5, [("feedforward_tanh", 1100)], (), True, 3, 2, [3, 2], 0.1, 46, 1.0),
    # wider than the rows the kernels hold in registers (Pp 2112 > 2048): the path that reads the row again per pass
    "very long row": (5, [("feedforward_tanh", 2100)], (), True, 3, 2, [3, 2], 0.1, 47, 1.0),
}
BF16_THROUGH_NET = ("wide", "headline", "first")          # (tests/test_layernorm_reference.py, condition (d))


class Case:
    def __init__(self, pkg, which):
        P, hidden, normed, out_normed, C, PS, lens, wscale, seed, bias = CASES[which]
        rng = np.random.RandomState(seed)
        self.which, self.P, self.hidden, self.C, self.PS, self.lens = which, P, hidden, C, PS, lens
        self.layers = net_desc(P, hidden, C, bias=bias)
        self.normed = tuple("%s_%d" % (hidden[i][0], i) for i in normed) + (("output",) if out_normed else ())
        self.weights = random_weights(self.layers, rng, wscale)
        self.xs, self.ts = random_sequences(rng, lens, P, C=C)
        self.frac = pkg.make_fraction(self.xs, self.ts, PS)
        self.T, self.N = self.frac["T"], self.frac["T"] * PS
        self._ref = {}

    def desc(self, normed=None, member=False):
        """The description with "layer_norm": true on `normed` (default: the case's); member: and false on every other trainable
        layer."""
        out = copy.deepcopy(self.layers)
        for d in out:
            if d["name"] in (self.normed if normed is None else normed):
                d["layer_norm"] = True
            elif member and "bias" in d:
                d["layer_norm"] = False
        return out

    def net(self, pkg, prec, normed=None, weights=None, **kw):
        return pkg.NeuralNetwork(self.desc(normed), weights or self.weights, self.PS, self.T, precision=getattr(pkg, prec), **kw)

    def reference(self, bf16=False):
        """(loss, posteriors, gradients, errors) of the stack with the case's layers normed, computed once."""
        if bf16 not in self._ref:
            self._ref[bf16] = stack_results(self.layers, self.weights, self.frac, self.lens, normed=self.normed, bf16=bf16)
        return self._ref[bf16]
