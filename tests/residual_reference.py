"""numpy / torch restatement of the residual connections of include/currennt_hip.h (section Residual connections).

    out[n][u] = round_op( float(b_op[n][u]) + float(x_op[n][u]) )     real frames;   out = b_op on every other row

b_op: the marked layer's own output (its "branch"), x_op: what the preceding layer's followers read, both in the reference layout;
round_op: one rounding to the operand type.  And the fp64 autograd stack of tests/test_oracle_autograd.py with h = branch(h) + h on
the marked layers, feed-forward hidden layers included."""
import numpy as np
import torch

from dropout_reference import bf16_round
from helpers import real_mask
from test_oracle_autograd import lstm_layer, tanh_, sig


def residual_sum(branch, x, real, bf16=False):
    """branch, x: [N][L] float32 operand values (bf16 mode: already bf16 values); real: bool [N] -> out [N][L] float32."""
    branch, x = np.asarray(branch, np.float32), np.asarray(x, np.float32)
    s = (branch + x).astype(np.float32)          # one fp32 addition (exact for two bf16 values up to the rounding below)
    if bf16:
        s = bf16_round(s)
    return np.where(np.asarray(real, bool)[:, None], s, branch)


_ACT = {"feedforward_tanh": tanh_, "feedforward_logistic": sig, "feedforward_identity": lambda v: v}


def ff_delta(kind, branch, e):
    """What a feed-forward layer's outputErrors hold once its backward pass has run (FeedForwardLayer.cu:72-79 overwrites them in
    place): act'(branch output) * e."""
    d = {"feedforward_tanh": 1.0 - branch * branch, "feedforward_logistic": branch * (1.0 - branch), "feedforward_identity": 1.0}[kind]
    return d * e


def autograd_residual(layers, flat_weights, frac, lens, marked, hook=None, branches=None):
    """The fp64 autograd stack of a network description `layers` (input, hidden lstm / blstm / feedforward_* layers, softmax,
    multiclass_classification; every bias the description's) on one fraction, with out = branch + (input on real frames) on the
    layers named in `marked`.  flat_weights: {layer: flat float64 array in the oracle's layout}.  hook(name, out) may replace a
    hidden layer's output (finite differences).  -> loss, posteriors of the real frames, {layer: gradient}, {layer: dL/d(outputs)
    on the real frames}.  branches (a dict, optional) receives {layer: the branch output on the real frames}."""
    T, PS = frac["T"], frac["PS"]
    params = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in flat_weights.items()}
    lens = list(lens) + [0] * (PS - len(lens))
    realm = torch.tensor(real_mask(frac).reshape(T, PS, 1).astype(np.float64))
    h = torch.tensor(frac["inputs"].reshape(T, PS, -1).astype(np.float64))
    prev, outs = layers[0]["size"], {}
    for d in layers[1:-2]:
        name, kind, size, w = d["name"], d["type"], d["size"], params[d["name"]]
        if kind in ("lstm", "blstm"):
            b = lstm_layer(h, lens, w, prev, size, kind == "blstm", float(d["bias"]))
        else:
            b = _ACT[kind](h @ w[:size * prev].reshape(size, prev).T + float(d["bias"]) * w[size * prev:])
        if branches is not None:
            branches[name] = b.detach().numpy().reshape(T * PS, -1)[real_mask(frac)]
        h = b + h * realm if name in marked else b
        if hook is not None:
            h = hook(name, h)
        h.retain_grad()
        outs[name] = h
        prev = size
    C, wo = layers[-2]["size"], params[layers[-2]["name"]]
    z = h @ wo[:C * prev].reshape(C, prev).T + float(layers[-2]["bias"]) * wo[C * prev:]
    logp = torch.log_softmax(z, dim=2)
    tc = torch.tensor(frac["targetClasses"].reshape(T, PS).astype(np.int64))
    loss = -(logp.gather(2, tc.clamp(min=0).unsqueeze(2)).squeeze(2) * (tc >= 0)).sum()
    loss.backward()
    real = real_mask(frac)
    post = torch.exp(logp).detach().numpy().reshape(-1, C)[real]
    return (float(loss.detach()), post, {k: v.grad.numpy() for k, v in params.items()},
            {k: v.grad.numpy().reshape(T * PS, -1)[real] for k, v in outs.items()})


def flat_weights(weights):
    return {n: np.concatenate([np.asarray(w[k], np.float64).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in weights.items()}
