"""-m gpu: --weight_average_decay / --weight_average_warmup in the C++ driver, on the set-up of test_driver_adam_autosave_continue:
a few sequences of tests/golden/val_1_speaker.nc, 39 -> lstm 8 -> softmax 51, PS 3, deterministic, no shuffling."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, net_desc, random_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
NC = os.path.join(GOLDEN, "val_1_speaker.nc")
NOTICE = "Weight averaging: the autosave file holds no average; it starts with the next update."


def weights_of(path):
    doc = json.load(open(path))
    return {n: np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in doc["weights"].items()}


def averages_of(state):
    """{layer name: float32 vector} of an autosave's weight_average: one array per layer, empty for layers without weights."""
    names = [l["name"] for l in state["layers"]]
    assert len(state["weight_average"]) == len(names)
    return {n: np.asarray(a, np.float32) for n, a in zip(names, state["weight_average"]) if len(a)}


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[n], b[n]) for n in a)


def epoch_rows(stdout):
    """The progress table's rows without their duration column."""
    rows = [l for l in stdout.splitlines() if re.match(r"^\s+\d+ \|", l)]
    return [[c for k, c in enumerate(r.split("|")) if k != 1] for r in rows]


@pytest.fixture()
def common(tmp_path):
    rng = np.random.RandomState(51)
    layers = net_desc(39, [("lstm", 8)], 51)
    weights = random_weights(layers, rng, 0.1)
    net = str(tmp_path / "network.jsn")
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    return [BIN, "--train", "true", "--stochastic", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net,
            "--parallel_sequences", "3", "--learning_rate", "1e-3", "--deterministic", "true", "--shuffle_fractions", "false",
            "--shuffle_sequences", "false", "--random_seed", "3", "--optimizer", "adam"]


def run(args):
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_driver_average_autosave_continue(pkg, tmp_path, common):
    """(a) No validation set, decay 0.9 without warm-up, 3 epochs: every epoch keeps the average as its best weights, so the trained
    network is the average; the autosave carries the average and the step count, and --continue from epoch 2 ends in the
    uninterrupted run's network bit for bit."""
    straight, prefix = str(tmp_path / "straight.jsn"), str(tmp_path / "run")
    out = run(common + ["--weight_average_decay", "0.9", "--weight_average_warmup", "false", "--max_epochs", "3", "--autosave", "true",
                        "--autosave_prefix", prefix, "--save_network", straight])
    assert "Weight averaging:          decay 0.9, warm-up off" in out
    auto = prefix + "_epoch002.autosave"
    state = json.load(open(auto))
    assert state["optimizer_cur_epoch"] == 2 and state["weight_average_steps"] == 4           # 6 sequences, 3 at a time, 2 epochs
    assert "weight_average_decay=0.9;" in state["configuration"] and "weight_average_warmup=false;" in state["configuration"]
    avg2 = averages_of(state)
    assert set(avg2) == set(state["weights"]) and all(np.abs(a).max() > 0 for a in avg2.values())
    assert not same(avg2, weights_of(auto))                        # (the average is not the raw weights it travels beside)
    resumed = str(tmp_path / "resumed.jsn")
    out = run([BIN, "--continue", auto, "--max_epochs", "3", "--autosave", "false", "--save_network", resumed])
    assert "Restoring state from" in out and "Weight averaging:          decay 0.9, warm-up off" in out and NOTICE not in out
    a, b = weights_of(straight), weights_of(resumed)
    for name in a:
        assert np.array_equal(a[name], b[name]), (name, float(np.abs(a[name] - b[name]).max()))
    last = averages_of(json.load(open(prefix + "_epoch003.autosave")))
    assert same(a, last)                                           # the trained network holds the averaged weights
    plain = str(tmp_path / "plain.jsn")
    out = run(common + ["--max_epochs", "3", "--save_network", plain])
    assert "Weight averaging" not in out
    assert not same(a, weights_of(plain))


def test_driver_average_with_a_validation_set(pkg, tmp_path, common):
    """(b) With a validation set.  Decay 1e-30 makes 1 - decay round to 1: the average is the raw weights, so every epoch's row
    and the final network equal the run without averaging -- the swap protocol around the validation pass does not disturb
    training.  With decay 0.9 the validation errors are another model's, and the .best.jsn file of --autosave_best holds the
    average of the epoch it was written for."""
    val = ["--val_file", NC, "--val_fraction", "0.04", "--max_epochs", "3"]
    plain, tiny = str(tmp_path / "plain.jsn"), str(tmp_path / "tiny.jsn")
    out_plain = run(common + val + ["--save_network", plain])
    out_tiny = run(common + val + ["--weight_average_decay", "1e-30", "--save_network", tiny])
    rows = epoch_rows(out_plain)
    assert len(rows) == 3 and all(r[2].strip() for r in rows)      # three epochs, each with a validation error
    assert epoch_rows(out_tiny) == rows
    assert same(weights_of(plain), weights_of(tiny))
    prefix = str(tmp_path / "best")
    out = run(common + ["--val_file", NC, "--val_fraction", "0.04", "--max_epochs", "2", "--weight_average_decay", "0.9", "--autosave", "true",
                        "--autosave_best", "true", "--autosave_prefix", prefix, "--save_network", str(tmp_path / "avg.jsn")])
    rows9 = epoch_rows(out)
    assert len(rows9) == 2 and [r[1] for r in rows9] == [r[1] for r in rows[:2]]             # the same training errors ...
    assert [r[2] for r in rows9] != [r[2] for r in rows[:2]]                                  # ... validated on the average
    best = [k + 1 for k, r in enumerate(rows9) if "yes" in r[-1]]
    assert best
    state = json.load(open(prefix + "_epoch%03d.autosave" % best[-1]))
    assert same(weights_of(prefix + ".best.jsn"), averages_of(state))


def test_driver_average_starts_late(pkg, tmp_path, common):
    """(c) --continue from an autosave written without averaging, with --weight_average_decay given: the run succeeds, says that
    the average starts fresh, and from then on autosaves carry it."""
    prefix = str(tmp_path / "run")
    run(common + ["--max_epochs", "2", "--autosave", "true", "--autosave_prefix", prefix, "--save_network", str(tmp_path / "one.jsn")])
    auto = prefix + "_epoch001.autosave"
    assert "weight_average" not in json.load(open(auto))
    late = str(tmp_path / "late")
    out = run([BIN, "--continue", auto, "--weight_average_decay", "0.9", "--max_epochs", "2", "--autosave_prefix", late,
               "--save_network", str(tmp_path / "two.jsn")])
    assert out.count(NOTICE) == 1 and "Weight averaging:          decay 0.9, warm-up on" in out
    state = json.load(open(late + "_epoch002.autosave"))
    assert state["weight_average_steps"] == 2 and same(averages_of(state), weights_of(str(tmp_path / "two.jsn")))
