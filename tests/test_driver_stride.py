"""-m gpu: the "stride" member of a context layer through the C++ driver (lstm-rnn_amd/currennt_hip) on the first 6 sequences of
tests/golden/val_1_speaker.nc: the net trains, the listing shows the stride, trained_network.jsn and the autosave carry it (and
those of a stride-1 net do not), --continue resumes the same run, --ff_input_file writes ceil(len / 2) rows per sequence, the
classification error column is taken over the reduced frames, and a ctc net with a stride trains and prints a label error rate."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, random_weights
from stride_reference import stride_net_desc
from test_driver_dropout import first_sequences
from test_gpu_dropout import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
NC = os.path.join(GOLDEN, "val_1_speaker.nc")
PS, ALL, FIRST = 3, 102, 6                   # (--train_fraction 0.06 of the file's 102 sequences: the first 6)


def write_network(path, stride):
    rng = np.random.RandomState(71)
    layers = stride_net_desc(39, [("lstm", 10), ("context", (0, 1, 1, stride)), ("blstm", 8)], 51)
    if stride == 1:
        del layers[2]["stride"]
    weights = random_weights(layers, rng, 0.3)
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(path, "w"))


def weights_of(path):
    doc = json.load(open(path))
    return {n: np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in doc["weights"].items()}


def common_args(net, epochs=2, lr="1e-2", mom="0.9"):
    return [BIN, "--train", "true", "--stochastic", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net,
            "--parallel_sequences", str(PS), "--learning_rate", lr, "--momentum", mom, "--precision", "f32", "--deterministic", "true",
            "--shuffle_fractions", "false", "--shuffle_sequences", "false", "--random_seed", "3", "--max_epochs", str(epochs)]


def run(args, timeout=300):
    out = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_driver_stride(pkg, tmp_path):
    net = str(tmp_path / "network.jsn")
    write_network(net, 2)
    trained, prefix = str(tmp_path / "trained_network.jsn"), str(tmp_path / "run")
    text = run(common_args(net) + ["--save_network", trained, "--autosave", "true", "--autosave_prefix", prefix])
    listing = [l for l in text.splitlines() if l.startswith("(")]
    assert len(listing) == 6 and listing[2].startswith("(2) context [size: 20, context -0..+1 x1 /2]"), listing
    auto = prefix + "_epoch001.autosave"
    a = json.load(open(trained))
    for doc in (a, json.load(open(auto))):
        d = doc["layers"][2]
        assert (d["type"], d["size"], d["left"], d["right"], d["dilation"], d["stride"]) == ("context", 20, 0, 1, 1, 2)
        assert all("stride" not in x for x in doc["layers"] if x["type"] != "context")
    w = weights_of(trained)
    rows = [l for l in text.splitlines() if re.match(r"^\s+\d+ \|", l)]
    assert len(rows) == 2 and all(np.isfinite(float(re.search(r"%\s+([0-9.]+) \|", r).group(1))) for r in rows), text
    # a stride-1 net prints and saves as before: no such member
    plain_net, plain, plain_prefix = str(tmp_path / "plain_network.jsn"), str(tmp_path / "plain.jsn"), str(tmp_path / "plain")
    write_network(plain_net, 1)
    text = run(common_args(plain_net, epochs=1) + ["--save_network", plain, "--autosave", "true", "--autosave_prefix", plain_prefix])
    assert "(2) context [size: 20, context -0..+1 x1]" in text and "/1" not in text
    for path in (plain, plain_prefix + "_epoch001.autosave"):
        assert '"stride"' not in open(path).read() and all("stride" not in x for x in json.load(open(path))["layers"])
    # --continue from the epoch-1 autosave ends in the uninterrupted run's weights, bit for bit
    resumed = str(tmp_path / "resumed.jsn")
    text = run([BIN, "--continue", auto, "--max_epochs", "2", "--autosave", "false", "--save_network", resumed])
    assert "Restoring state from" in text and "x1 /2]" in text
    wr = weights_of(resumed)
    for n in w:
        assert np.array_equal(w[n], wr[n]), (n, float(np.abs(w[n] - wr[n]).max()))
    assert json.load(open(resumed))["layers"][2]["stride"] == 2
    # --ff_input_file: ceil(len / 2) rows per sequence, the Python mirror's values
    csv = str(tmp_path / "ff.csv")
    run([BIN, "--train", "false", "--ff_input_file", NC, "--network", trained, "--parallel_sequences", str(PS),
         "--precision", "f32", "--ff_output_file", csv, "--ff_output_format", "single_csv", "--revert_std", "false"])
    rows = open(csv).read().strip().split("\n")
    xs, ts = first_sequences(ALL)
    fracs = pkg.make_fractions(xs, ts, PS)                                       # forward pass: file order, no sort
    k, worst = 0, 0.0
    with pkg.NeuralNetwork(a["layers"], a["weights"], PS, max(f["T"] for f in fracs), precision=pkg.PREC_F32) as mirror:
        assert mirror.layer("context_1").stride() == 2
        for f in fracs:
            mirror.load_sequences(f); mirror.compute_forward_pass()
            y = mirror.outputs()
            assert list(mirror.lengths("output")[:len(f["seqLengths"])]) == [-(-n // 2) for n in f["seqLengths"]]
            for i, n in enumerate(f["seqLengths"]):
                m = -(-n // 2)
                vals = np.array(rows[k].split(";")[1:], np.float64)
                assert vals.size == m * 51, (k, n, vals.size)
                worst = max(worst, float(np.abs(vals.reshape(m, -1) - y[:m, i, :]).max()))
                k += 1
    assert k == ALL == len(rows)
    assert worst < TOL["PREC_F32"][0], worst


def test_error_column_counts_the_reduced_frames(pkg, tmp_path):
    """A learning rate of 0 keeps the weights: the training row is the evaluation of the network file, which the Python mirror
    repeats.  The classification error is (frames - correct) / frames with frames = the sum of ceil(len / 2)."""
    net = str(tmp_path / "network.jsn")
    write_network(net, 2)
    text = run(common_args(net, epochs=1, lr="0", mom="0") + ["--save_network", str(tmp_path / "out.jsn")])
    row = [l for l in text.splitlines() if re.match(r"^\s+1 \|", l)][0]
    m = re.search(r"\|\s*([0-9.]+)%\s+([0-9.]+) \|", row)
    percent, error = float(m.group(1)), float(m.group(2))
    doc = json.load(open(net))
    xs, ts = first_sequences(FIRST)
    fracs = pkg.make_fractions(xs, ts, PS, sort_by_length=True)
    total, correct = 0.0, 0
    with pkg.NeuralNetwork(doc["layers"], doc["weights"], PS, max(f["T"] for f in fracs), precision=pkg.PREC_F32) as mirror:
        for f in fracs:
            mirror.load_sequences(f); mirror.compute_forward_pass()
            e, c = mirror.error_and_correct()
            total, correct = total + e, correct + c
    reduced, full = sum(-(-len(x) // 2) for x in xs), sum(len(x) for x in xs)
    want = 100.0 * (reduced - correct) / reduced
    print(row, "| mirror: %.4f%% of %d frames (%d at the input's rate), error %.4f" % (want, reduced, full, total / FIRST))
    assert abs(percent - want) <= 0.0051 and abs(error - total / FIRST) <= 0.0006 + 1e-4 * total / FIRST
    assert abs(percent - 100.0 * (full - correct) / full) > 1.0           # (the input-rate count would show another figure)


def test_driver_trains_a_strided_ctc_net(tmp_path):
    from test_gpu_ctc import toy_set
    from test_host_dataset import write_nc
    rng = np.random.RandomState(12)
    files = {}
    for name, n_seq in (("train", 7), ("val", 4)):
        xs, labels = toy_set(rng, n_seq)
        ts = [np.argmax(np.round(x), axis=1).astype(np.int32) for x in xs]            # the frame's pattern is its class
        files[name] = str(tmp_path / (name + ".nc"))
        write_nc(files[name], xs, ts, 4, name[0])
    layers = [{"name": "input", "type": "input", "size": 6},
              {"name": "lstm", "type": "lstm", "size": 8, "bias": 1.0},
              {"name": "pyramid", "type": "context", "size": 16, "left": 0, "right": 1, "stride": 2},
              {"name": "output", "type": "softmax", "size": 5, "bias": 1.0},
              {"name": "postoutput", "type": "ctc", "size": 5}]
    weights = random_weights(layers, rng, 0.1)
    net = str(tmp_path / "ctc.jsn")
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    text = run([BIN, "--train", "true", "--train_file", files["train"], "--val_file", files["val"], "--network", net,
                "--parallel_sequences", "3", "--max_epochs", "3", "--max_epochs_no_best", "10", "--learning_rate", "1e-2", "--momentum", "0.9",
                "--optimizer", "steepest_descent", "--precision", "f32", "--shuffle_fractions", "false", "--shuffle_sequences", "false",
                "--save_network", str(tmp_path / "out.jsn")], timeout=120)
    assert "context -0..+1 x1 /2]" in text
    rows = [l for l in text.splitlines() if re.match(r"^\s+\d+ \|", l)]
    assert len(rows) == 3, text
    for r in rows:
        cols = [c.strip() for c in r.split("|")]
        assert re.fullmatch(r"-\s+[0-9]+\.[0-9]{3}", cols[2]), r
        m = re.fullmatch(r"([0-9]+\.[0-9]{2})%\s+([0-9]+\.[0-9]{3})", cols[3])
        assert m and np.isfinite(float(m.group(2))) and 0.0 <= float(m.group(1)), r
