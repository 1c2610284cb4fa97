"""-m gpu: the JSON "layer_norm" member through the C++ driver (lstm-rnn_amd/currennt_hip) on a few sequences of
tests/golden/val_1_speaker.nc: a marked net trains, the member and its eps travel through trained_network.jsn and the autosave,
--continue resumes the same run, a forward pass (--ff_input_file) normalises too, and a description that cannot be normalised is
refused."""
import json
import os
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, net_desc, random_weights
from test_driver_dropout import first_sequences

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
NC = os.path.join(GOLDEN, "val_1_speaker.nc")
PS, ALL = 3, 102                             # (--train_fraction 0.06 of the file's 102 sequences: the first 6)
HIDDEN = [("lstm", 8), ("blstm", 8), ("feedforward_tanh", 8)]
MARKED = {"blstm_1": None, "output": 1e-3}  # layer -> "layer_norm_eps" (None: the member is absent, the default 1e-5 holds)


def write_network(path, marked, hidden=HIDDEN, value=True):
    rng = np.random.RandomState(30)
    layers = net_desc(39, hidden, 51)
    for d in layers:
        if d["name"] in marked:
            d["layer_norm"] = value
            if marked[d["name"]] is not None:
                d["layer_norm_eps"] = marked[d["name"]]
    weights = random_weights(layers, rng, 0.3)
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(path, "w"))


def weights_of(path):
    doc = json.load(open(path))
    return {n: np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in doc["weights"].items()}


def test_driver_layer_norm(pkg, tmp_path):
    net = str(tmp_path / "network.jsn")
    write_network(net, MARKED)
    common = [BIN, "--train", "true", "--stochastic", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net,
              "--parallel_sequences", str(PS), "--learning_rate", "1e-2", "--momentum", "0.9", "--precision", "f32", "--deterministic", "true",
              "--shuffle_fractions", "false", "--shuffle_sequences", "false", "--random_seed", "3", "--max_epochs", "2"]
    trained, prefix = str(tmp_path / "trained_network.jsn"), str(tmp_path / "run")
    out = subprocess.run(common + ["--save_network", trained, "--autosave", "true", "--autosave_prefix", prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # the layer listing names the marked layers
    listing = [l for l in out.stdout.splitlines() if l.startswith("(")]
    assert [", layer_norm]" in l for l in listing] == [False, False, True, False, True, False], listing
    # the member and its eps travel with the saved network and the autosave, on the marked layers only
    auto = prefix + "_epoch001.autosave"
    a = json.load(open(trained))
    for doc in (a, json.load(open(auto))):
        assert {d["name"]: d.get("layer_norm") for d in doc["layers"]} == {d["name"]: (True if d["name"] in MARKED else None) for d in doc["layers"]}
        eps = {d["name"]: d.get("layer_norm_eps") for d in doc["layers"]}
        assert all(eps[n] is None for n in eps if n not in MARKED)
        assert np.float32(eps["blstm_1"]) == np.float32(1e-5) and np.float32(eps["output"]) == np.float32(1e-3)
    # ... and it is part of the model: the same net without it trains other weights
    plain_net, plain = str(tmp_path / "plain_network.jsn"), str(tmp_path / "plain.jsn")
    write_network(plain_net, {})
    out = subprocess.run([plain_net if c == net else c for c in common] + ["--save_network", plain], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert all("layer_norm" not in d for d in json.load(open(plain))["layers"]) and ", layer_norm" not in out.stdout
    w, wp = weights_of(trained), weights_of(plain)
    assert all(not np.array_equal(w[n], wp[n]) for n in w)
    # --continue from the epoch-1 autosave ends in the uninterrupted run's weights, bit for bit
    resumed = str(tmp_path / "resumed.jsn")
    out = subprocess.run([BIN, "--continue", auto, "--max_epochs", "2", "--autosave", "false", "--save_network", resumed], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Restoring state from" in out.stdout
    wr = weights_of(resumed)
    for n in w:
        assert np.array_equal(w[n], wr[n]), (n, float(np.abs(w[n] - wr[n]).max()))
    # a forward pass of the saved network normalises too: the driver's output is the Python mirror's
    csv = str(tmp_path / "ff.csv")
    out = subprocess.run([BIN, "--train", "false", "--ff_input_file", NC, "--network", trained, "--parallel_sequences", str(PS),
                          "--precision", "f32", "--ff_output_file", csv, "--ff_output_format", "single_csv", "--revert_std", "false"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = open(csv).read().strip().split("\n")
    xs, ts = first_sequences(ALL)
    fracs = pkg.make_fractions(xs, ts, PS)                                       # forward pass: file order, no sort
    k = 0
    with pkg.NeuralNetwork(a["layers"], a["weights"], PS, max(f["T"] for f in fracs), precision=pkg.PREC_F32) as mirror:
        assert [l.layer_norm for l in mirror.layers] == [False, False, True, False, True, False]
        assert np.float32(mirror.layer("output").layer_norm_eps) == np.float32(1e-3)
        for f in fracs:
            mirror.load_sequences(f); mirror.compute_forward_pass()
            y = mirror.outputs()
            for i, n in enumerate(f["seqLengths"]):
                vals = np.array(rows[k].split(";")[1:], np.float64).reshape(n, -1)
                assert np.abs(vals - y[:n, i, :]).max() < 1e-6                  # posteriors <= 1, printed with 6 significant digits
                k += 1
    assert k == ALL == len(rows)


def run_refused(tmp_path, **kw):
    net = str(tmp_path / "network.jsn")
    write_network(net, **kw)
    out = subprocess.run([BIN, "--train", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net, "--parallel_sequences", str(PS),
                          "--max_epochs", "1", "--save_network", str(tmp_path / "never.jsn")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2, out.stdout + out.stderr
    assert "FAILED:" in out.stdout and not os.path.exists(str(tmp_path / "never.jsn"))
    return out.stdout


def test_driver_refuses_what_cannot_be_normalised(pkg, tmp_path):
    """The texts (the Python mirror refuses the same files with the same texts: tests/test_gpu_layernorm.py::test_errors)."""
    for name in ("input", "postoutput"):
        text = run_refused(tmp_path, marked={name: None})
        assert "Invalid value 'layer_norm' in layer '%s': only lstm, blstm, feedforward_* and softmax layers normalise their input" % name in text
    text = run_refused(tmp_path, marked={"blstm_1": None}, value=1)
    assert "Invalid value 'layer_norm' in layer 'blstm_1': true or false expected" in text
    text = run_refused(tmp_path, marked={"lstm_1": None}, hidden=[("lstm", 1), ("lstm", 8)])
    assert "Invalid value 'layer_norm' in layer 'lstm_1': the preceding layer's size 1 is below 2" in text
    text = run_refused(tmp_path, marked={"blstm_1": 0.0})
    assert "Invalid value 'layer_norm_eps' in layer 'blstm_1': a finite number above 0 expected" in text
