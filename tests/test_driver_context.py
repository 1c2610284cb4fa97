"""-m gpu: the "context" layer through the C++ driver (lstm-rnn_amd/currennt_hip) on a few sequences of
tests/golden/val_1_speaker.nc: the net trains, the layer and its members travel through trained_network.jsn and the autosave without
a weights entry, --continue resumes the same run, a forward pass (--ff_input_file) runs the layer too, and bad descriptions are
refused with a message that names the layer."""
import json
import os
import subprocess

import numpy as np
import pytest

from context_reference import context_net_desc
from helpers import GOLDEN, random_weights
from test_driver_dropout import first_sequences
from test_gpu_dropout import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
NC = os.path.join(GOLDEN, "val_1_speaker.nc")
PS, ALL = 3, 102                             # (--train_fraction 0.06 of the file's 102 sequences: the first 6)


def hidden(members):
    return [("lstm", 8), ("context", members), ("feedforward_tanh", 8), ("blstm", 8)]


def write_network(path, members=(1, 1, 2), edit=None, layers=None):
    rng = np.random.RandomState(61)
    layers = layers or context_net_desc(39, hidden(members), 51)
    weights = random_weights(layers, rng, 0.3)
    if edit:
        edit(layers)
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(path, "w"))


def weights_of(path):
    doc = json.load(open(path))
    return {n: np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in doc["weights"].items()}


def test_driver_context(pkg, tmp_path):
    net = str(tmp_path / "network.jsn")
    write_network(net)
    common = [BIN, "--train", "true", "--stochastic", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net,
              "--parallel_sequences", str(PS), "--learning_rate", "1e-2", "--momentum", "0.9", "--precision", "f32", "--deterministic", "true",
              "--shuffle_fractions", "false", "--shuffle_sequences", "false", "--random_seed", "3", "--max_epochs", "2"]
    trained, prefix = str(tmp_path / "trained_network.jsn"), str(tmp_path / "run")
    out = subprocess.run(common + ["--save_network", trained, "--autosave", "true", "--autosave_prefix", prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # the layer listing names the context layer
    listing = [l for l in out.stdout.splitlines() if l.startswith("(")]
    assert len(listing) == 7 and listing[2].startswith("(2) context [size: 24, context -1..+1 x2]"), listing
    assert sum("context" in l for l in listing) == 1
    # the layer travels with the saved network and the autosave: its members, and no entry in "weights"
    auto = prefix + "_epoch001.autosave"
    a = json.load(open(trained))
    for doc in (a, json.load(open(auto))):
        d = doc["layers"][2]
        assert (d["name"], d["type"], d["size"], d["left"], d["right"], d["dilation"]) == ("context_1", "context", 24, 1, 1, 2)
        assert "bias" not in d and "context_1" not in doc["weights"]
        assert sorted(doc["weights"]) == ["blstm_3", "feedforward_tanh_2", "lstm_0", "output"]
        assert all("left" not in x and "dilation" not in x for x in doc["layers"] if x["type"] != "context")
    assert len(a["weights"]["feedforward_tanh_2"]["input"]) == 8 * 24
    # ... and it is part of the model: context(0, 0) in its place is a net of another shape that trains other weights
    plain_net, plain = str(tmp_path / "plain_network.jsn"), str(tmp_path / "plain.jsn")
    write_network(plain_net, members=(0, 0, 1))
    out = subprocess.run([plain_net if c == net else c for c in common] + ["--save_network", plain], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "(2) context [size: 8, context -0..+0 x1]" in out.stdout
    p = json.load(open(plain))
    assert p["layers"][2]["size"] == 8 and len(p["weights"]["feedforward_tanh_2"]["input"]) == 8 * 8
    w, wp = weights_of(trained), weights_of(plain)
    assert w["feedforward_tanh_2"].size != wp["feedforward_tanh_2"].size
    assert all(not np.array_equal(w[n], wp[n]) for n in w if w[n].size == wp[n].size)
    # --continue from the epoch-1 autosave ends in the uninterrupted run's weights, bit for bit
    resumed = str(tmp_path / "resumed.jsn")
    out = subprocess.run([BIN, "--continue", auto, "--max_epochs", "2", "--autosave", "false", "--save_network", resumed], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Restoring state from" in out.stdout
    wr = weights_of(resumed)
    for n in w:
        assert np.array_equal(w[n], wr[n]), (n, float(np.abs(w[n] - wr[n]).max()))
    # a forward pass of the saved network runs the layer like training does: the driver's output is the Python mirror's
    csv = str(tmp_path / "ff.csv")
    out = subprocess.run([BIN, "--train", "false", "--ff_input_file", NC, "--network", trained, "--parallel_sequences", str(PS),
                          "--precision", "f32", "--ff_output_file", csv, "--ff_output_format", "single_csv", "--revert_std", "false"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = open(csv).read().strip().split("\n")
    xs, ts = first_sequences(ALL)
    fracs = pkg.make_fractions(xs, ts, PS)                                       # forward pass: file order, no sort
    k, worst = 0, 0.0
    with pkg.NeuralNetwork(a["layers"], a["weights"], PS, max(f["T"] for f in fracs), precision=pkg.PREC_F32) as mirror:
        assert mirror.layer("context_1").context() == (1, 1, 2)
        for f in fracs:
            mirror.load_sequences(f); mirror.compute_forward_pass()
            y = mirror.outputs()
            for i, n in enumerate(f["seqLengths"]):
                vals = np.array(rows[k].split(";")[1:], np.float64).reshape(n, -1)
                worst = max(worst, float(np.abs(vals - y[:n, i, :]).max()))
                k += 1
    assert k == ALL == len(rows)
    assert worst < TOL["PREC_F32"][0], worst


def run_refused(tmp_path, **kw):
    net = str(tmp_path / "network.jsn")
    write_network(net, **kw)
    out = subprocess.run([BIN, "--train", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net, "--parallel_sequences", str(PS),
                          "--max_epochs", "1", "--save_network", str(tmp_path / "never.jsn")], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0, out.stdout + out.stderr
    assert "FAILED:" in out.stdout and not os.path.exists(str(tmp_path / "never.jsn"))
    return out.stdout


def test_driver_refuses_bad_context_layers(pkg, tmp_path):
    def wrong_size(layers):
        layers[2]["size"] = 16

    def no_dilation(layers):
        layers[2]["dilation"] = 0
    text = run_refused(tmp_path, edit=wrong_size)
    assert "Size mismatch: 16 vs. 24 in layer 'context_1'" in text
    text = run_refused(tmp_path, edit=no_dilation)
    assert "Invalid value 'dilation' in layer 'context_1': an integer in 1..16 expected" in text
    # a context layer as the last hidden layer: no post output layer may follow it
    layers = [{"name": "input", "type": "input", "size": 39}, {"name": "lstm_0", "type": "lstm", "size": 17, "bias": 1.0},
              {"name": "context_1", "type": "context", "size": 51, "left": 1, "right": 1},
              {"name": "postoutput", "type": "multiclass_classification", "size": 51}]
    text = run_refused(tmp_path, layers=layers)
    assert "Cannot add post output layer after a non trainable layer (the context layer 'context_1')" in text
