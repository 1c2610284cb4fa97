"""Shared helpers of the test suite: fixtures on disk, synthetic networks and fractions."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_kat0():
    """KAT-0 inputs: test1 network + first 10 sequences of val_1_speaker.nc."""
    z = np.load(os.path.join(GOLDEN, "kat0_test1.npz"))
    layers = json.loads(str(z["layers_json"]))
    weights = {}
    for k in z.files:
        if k.startswith("w/"):
            _, name, key = k.split("/")
            weights.setdefault(name, {})[key] = z[k]
    lens = z["seqLengths"]
    off = np.concatenate([[0], np.cumsum(lens)])
    xs = [z["inputs"][off[i]:off[i + 1]] for i in range(len(lens))]
    ts = [z["targetClasses"][off[i]:off[i + 1]] for i in range(len(lens))]
    return layers, weights, xs, ts


def lstm_weight_count(P, L, bidir):
    return L * (4 * (P + 1) + (2 if bidir else 4) * L + 3)


def random_weights(layers, rng, scale=0.1):
    """Explicit weights for every trainable layer, split like the JSON sections."""
    out = {}
    prev = None
    for d in layers:
        t, L = d["type"], int(d["size"])
        if t in ("lstm", "blstm"):
            P = int(prev["size"])
            H = L // (2 if t == "blstm" else 1)
            out[d["name"]] = {"input": rng.uniform(-scale, scale, 4 * L * P).astype(np.float32),
                              "bias": rng.uniform(-scale, scale, 4 * L).astype(np.float32),
                              "internal": rng.uniform(-scale, scale, 4 * L * H + 3 * L).astype(np.float32)}
        elif t == "softmax" or t.startswith("feedforward"):
            P = int(prev["size"])
            out[d["name"]] = {"input": rng.uniform(-scale, scale, L * P).astype(np.float32),
                              "bias": rng.uniform(-scale, scale, L).astype(np.float32),
                              "internal": np.zeros(0, np.float32)}
        prev = d
    return out


def net_desc(P, hidden, C, post="multiclass_classification", bias=1.0):
    """hidden: list of (type, size) tuples."""
    layers = [{"name": "input", "type": "input", "size": P}]
    for i, (t, s) in enumerate(hidden):
        layers.append({"name": "%s_%d" % (t, i), "type": t, "size": s, "bias": bias})
    layers.append({"name": "output", "type": "softmax" if post == "multiclass_classification" else "feedforward_identity",
                   "size": C, "bias": bias})
    layers.append({"name": "postoutput", "type": post, "size": C})
    return layers


def random_sequences(rng, lengths, P, C=None, L=None):
    xs = [rng.randn(n, P).astype(np.float32) for n in lengths]
    if C is not None:
        ts = [rng.randint(0, C, n).astype(np.int32) for n in lengths]
    else:
        ts = [rng.randn(n, L).astype(np.float32) for n in lengths]
    return xs, ts


def real_mask(frac):
    return np.asarray(frac["patTypes"]).reshape(-1) != 0


def load_ref_golden(name):
    """One case of tests/golden/ref_golden.npz (outputs of the reference's own compiled functors, made by
    tests/golden/make_ref_golden.py): (layers, weights, xs, ts, PS, expected dict)."""
    z = np.load(os.path.join(GOLDEN, "ref_golden.npz"))
    pre = name + "/"
    layers = json.loads(str(z[pre + "layers_json"]))
    weights, exp = {}, {}
    for k in z.files:
        if not k.startswith(pre):
            continue
        parts = k[len(pre):].split("/")
        if parts[0] == "w":
            weights.setdefault(parts[1], {})[parts[2]] = z[k]
        elif parts[0] not in ("layers_json", "PS", "seqLengths", "inputs", "targetClasses", "targets"):
            exp["/".join(parts)] = z[k]
    lens = z[pre + "seqLengths"]
    off = np.concatenate([[0], np.cumsum(lens)])
    xs = [z[pre + "inputs"][off[i]:off[i + 1]] for i in range(len(lens))]
    tkey = pre + ("targetClasses" if pre + "targetClasses" in z.files else "targets")      # real-valued targets: sse case
    ts = [z[tkey][off[i]:off[i + 1]] for i in range(len(lens))]
    return layers, weights, xs, ts, int(z[pre + "PS"]), exp


# ---- references for the fp64-relative bounds (tests/test_oracle_fp64.py, tests/test_gpu_long_fp64.py) ----------------------

def oracle_reference(ons, layers, weights, frac, PS, rounding=None):
    """One forward + backward pass of an oracle namespace (`orc` = fp32, `orc.real64()` = double), optionally under an operand
    rounding model, as a dict of float64 arrays in the layout the comparisons use: posteriors of the real frames `post`
    [frames][C], `error`, `correct`, `grad/<layer>`, `err/<layer>` (propagated errors into a trainable layer, real frames), and
    `ylast`: the last LSTM layer's outputs [T][PS][L]."""
    with ons.operand_rounding(rounding):
        ref = ons.OracleNetwork(layers, weights, PS, frac["T"])
        ref.load_sequences(frac); ref.compute_forward_pass()
        out = {"error": ref.calculate_error(), "correct": ref.count_correct_classifications()}
        ref.compute_backward_pass()
    real = real_mask(frac)
    C = layers[-1]["size"]
    out["post"] = ref.outputs().reshape(-1, C)[real].astype(np.float64)
    for lay in ref.trainable_layers():
        out["grad/" + lay.name] = lay.weightUpdates.astype(np.float64)
        if lay.prev.trainable:
            out["err/" + lay.prev.name] = lay.prev.outputErrors[:ref.N * lay.prev.size].reshape(-1, lay.prev.size)[real].astype(np.float64)
        if lay.type in ("lstm", "blstm"):
            out["ylast"] = lay.outputs[:ref.N * lay.size].reshape(ref.T, PS, lay.size).astype(np.float64)
    return out


def fp64_distances(got, r64, t_long, slot=0):
    """The compared quantities of `got` against the double oracle's `r64` (both as oracle_reference returns them):
    `post` posteriors max-abs; `grad/<layer>`, `err/<layer>` max-abs over the layer's max (rel_err of test_gpu_parity);
    `y_first` / `y_last`: the last LSTM layer's outputs at frame 0 and frame t_long - 1 of `slot` (the longest sequence:
    the backward direction has run all its steps at frame 0, the forward direction at the last frame), max-abs."""
    d = {"post": float(np.abs(got["post"] - r64["post"]).max())}
    for k in r64:
        if k.startswith("grad/") or k.startswith("err/"):
            d[k] = float(np.abs(got[k] - r64[k]).max() / max(1e-12, np.abs(r64[k]).max()))
    d["y_first"] = float(np.abs(got["ylast"][0, slot] - r64["ylast"][0, slot]).max())
    d["y_last"] = float(np.abs(got["ylast"][t_long - 1, slot] - r64["ylast"][t_long - 1, slot]).max())
    return d
