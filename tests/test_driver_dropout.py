"""-m gpu: the JSON "dropout" member through the C++ driver (lstm-rnn_amd/currennt_hip) on a few sequences of
tests/golden/val_1_speaker.nc: training passes drop with masks derived from --random_seed, the epoch and the fraction's index;
validation does not drop; the member travels through trained_network.jsn and the autosave; a bad rate is refused."""
import json
import os
import subprocess

import numpy as np
import pytest
from scipy.io import netcdf_file

from helpers import GOLDEN, net_desc, random_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
NC = os.path.join(GOLDEN, "val_1_speaker.nc")
RATE, PS, SEQS = 0.2, 3, 6                   # --train_fraction / --val_fraction 0.06 of 102 sequences: the first 6


def write_network(path, rates):
    rng = np.random.RandomState(27)
    layers = net_desc(39, [("lstm", 8)], 51)
    for d in layers:
        if d["name"] in rates:
            d["dropout"] = rates[d["name"]]
    weights = random_weights(layers, rng, 0.3)
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(path, "w"))


def first_sequences(n):
    f = netcdf_file(NC, "r", mmap=False)
    lens = f.variables["seqLengths"][:n].astype(int)
    off = np.concatenate([[0], np.cumsum(lens)])
    x, t = f.variables["inputs"][:off[-1]].astype(np.float32), f.variables["targetClasses"][:off[-1]].astype(np.int32)
    f.close()
    return [x[off[i]:off[i + 1]] for i in range(n)], [t[off[i]:off[i + 1]] for i in range(n)]


def error_per_sequence(pkg, doc, xs, ts, drop):
    """The error column of the driver (summed error / number of sequences) for the network in `doc`, from Python."""
    fracs = pkg.make_fractions(xs, ts, PS)
    with pkg.NeuralNetwork(doc["layers"], doc["weights"], PS, max(f["T"] for f in fracs), precision=pkg.PREC_F32) as net:
        total = 0.0
        for k, f in enumerate(fracs):
            net.set_dropout_pass(1 if drop else 0, 3, k)
            net.load_sequences(f); net.compute_forward_pass()
            total += net.calculate_error()
    return total / len(xs)


def test_driver_dropout(pkg, tmp_path):
    net = str(tmp_path / "network.jsn")
    write_network(net, {"lstm_0": RATE, "output": RATE})
    common = [BIN, "--train", "true", "--stochastic", "true", "--train_file", NC, "--train_fraction", "0.06", "--val_file", NC, "--val_fraction", "0.06",
              "--network", net, "--parallel_sequences", str(PS), "--learning_rate", "1e-2", "--momentum", "0.9", "--precision", "f32",
              "--shuffle_fractions", "false", "--shuffle_sequences", "false", "--max_epochs", "2"]
    saved = {}
    for name, seed in (("a", "3"), ("b", "3"), ("other", "4")):
        saved[name] = str(tmp_path / (name + ".jsn"))
        extra = ["--autosave", "true", "--autosave_prefix", str(tmp_path / "run")] if name == "a" else []
        out = subprocess.run(common + ["--random_seed", seed, "--save_network", saved[name]] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        if name == "a":
            stdout = out.stdout
    # the same seed: the same masks, the same network byte for byte; another seed: other masks
    assert open(saved["a"], "rb").read() == open(saved["b"], "rb").read()
    a, other = json.load(open(saved["a"])), json.load(open(saved["other"]))
    assert any(a["weights"][n]["input"] != other["weights"][n]["input"] for n in a["weights"])
    # ... and other weights than training without dropout gives (the member is not merely carried along)
    plain_net, plain = str(tmp_path / "plain_network.jsn"), str(tmp_path / "plain.jsn")
    write_network(plain_net, {})
    cmd = [plain_net if c == net else c for c in common]
    out = subprocess.run(cmd + ["--random_seed", "3", "--save_network", plain], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    p = json.load(open(plain))
    assert any(a["weights"][n]["input"] != p["weights"][n]["input"] for n in a["weights"])
    # the member travels with the saved network and the autosave; files without it are written without it
    auto = json.load(open(str(tmp_path / "run_epoch001.autosave")))
    for doc in (a, auto):
        got = {d["name"]: d.get("dropout") for d in doc["layers"]}
        assert got["input"] is None and got["postoutput"] is None
        assert abs(got["lstm_0"] - RATE) < 1e-6 and abs(got["output"] - RATE) < 1e-6
    assert all("dropout" not in d for d in p["layers"])
    # evaluation does not drop: the validation error printed for epoch 1 is a plain forward pass of the epoch-1 weights.
    # Bound: the project's 1e-4 relative on an error (the autosave text carries ~7 digits of every weight)
    # plus half a unit of the third decimal the table prints.  The same pass WITH dropout lies outside of it.
    rows = [l.split("|") for l in stdout.splitlines() if l.strip()[:1].isdigit() and "|" in l]
    assert len(rows) == 2 and rows[0][0].strip() == "1"
    printed = float(rows[0][3].split("%")[1])
    xs, ts = first_sequences(SEQS)
    clean, dropped = error_per_sequence(pkg, auto, xs, ts, False), error_per_sequence(pkg, auto, xs, ts, True)
    print("validation error of epoch 1: printed %.3f, forward pass %.6f, with dropout %.6f" % (printed, clean, dropped))
    bound = 1e-4 * abs(clean) + 5e-4
    assert abs(printed - clean) <= bound, (printed, clean)
    assert abs(printed - dropped) > bound, (printed, dropped)          # (the check tells the two apart)


def test_driver_refuses_a_bad_rate(pkg, tmp_path):
    net = str(tmp_path / "network.jsn")
    write_network(net, {"output": 1.5})
    out = subprocess.run([BIN, "--train", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net, "--parallel_sequences", str(PS),
                          "--max_epochs", "1", "--save_network", str(tmp_path / "never.jsn")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2, out.stdout + out.stderr
    assert "FAILED:" in out.stdout and "'dropout'" in out.stdout and "'output'" in out.stdout
    assert not os.path.exists(str(tmp_path / "never.jsn"))
    # ... and a rate on a layer that cannot drop (the Python mirror refuses the same file: tests/test_gpu_dropout.py::test_errors)
    write_network(net, {"postoutput": 0.2})
    out = subprocess.run([BIN, "--train", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net, "--parallel_sequences", str(PS),
                          "--max_epochs", "1", "--save_network", str(tmp_path / "never.jsn")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2, out.stdout + out.stderr
    assert "FAILED:" in out.stdout and "'dropout'" in out.stdout and "'postoutput'" in out.stdout
    assert not os.path.exists(str(tmp_path / "never.jsn"))
