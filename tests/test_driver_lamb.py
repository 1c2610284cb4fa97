"""-m gpu: `--optimizer lamb` in the C++ driver, on a few sequences of tests/golden/val_1_speaker.nc (39 -> lstm 8 -> softmax 51,
PS 3, deterministic, no shuffling; the command-line skeleton of test_driver_decay.py)."""
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
TRUST_LINE = re.compile(r"^\s+trust ratio: min (\S+) \((\w+)\), max (\S+) \((\w+)\)$", re.M)
NEW_LINES = ("Optimizer type: LAMB", "Trust ratio bounds:", "trust ratio:")


def _weights_of(path):
    doc = json.load(open(path))
    return {n: np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in doc["weights"].items()}


def _same(a, b):
    return all(np.array_equal(a[n], b[n]) for n in a)


def _training_errors(text):
    """the training error column of the epoch table's rows"""
    rows = [l for l in text.splitlines() if re.match(r"^\s+\d+ \|", l)]
    return [float(r.split("|")[2].split()[-1]) for r in rows]


class Runs:
    """runs of the driver by name, each made once"""

    def __init__(self, tmp):
        self.tmp = tmp
        self.nc = os.path.join(GOLDEN, "val_1_speaker.nc")
        rng = np.random.RandomState(71)
        layers = net_desc(39, [("lstm", 8)], 51)
        self.names = [d["name"] for d in layers[1:3]]
        self.initial = random_weights(layers, rng, 0.1)
        self.net = str(tmp / "network.jsn")
        json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in self.initial.items()}},
                  open(self.net, "w"))
        self.done = {}

    def common(self, optimizer="lamb", epochs="3", stochastic="true"):
        return [BIN, "--train", "true", "--stochastic", stochastic, "--train_file", self.nc, "--train_fraction", "0.06", "--network", self.net,
                "--parallel_sequences", "3", "--learning_rate", "1e-2", "--optimizer", optimizer, "--deterministic", "true",
                "--shuffle_fractions", "false", "--shuffle_sequences", "false", "--random_seed", "3", "--max_epochs", epochs]

    def run(self, name, args, expect_ok=True):
        if name not in self.done:
            saved = str(self.tmp / (name + ".jsn"))
            r = subprocess.run(args + ["--save_network", saved], capture_output=True, text=True, timeout=300)
            if expect_ok:
                assert r.returncode == 0, r.stdout + r.stderr
            self.done[name] = (r.stdout + r.stderr, _weights_of(saved) if os.path.exists(saved) else None, r.returncode)
        return self.done[name]

    def prefix(self, name):
        return str(self.tmp / ("auto_" + name))

    def autosaving(self, name):
        return ["--autosave", "true", "--autosave_prefix", self.prefix(name)]

    def three(self):
        """three epochs, an autosave behind each"""
        return self.run("three", self.common() + ["--weight_decay", "0.01", "--lamb_min_trust", "0.001", "--lamb_max_trust", "100"] + self.autosaving("three"))

    def adam(self):
        return self.run("adam", self.common("adam", epochs="2") + self.autosaving("adam"))

    def sgd(self):
        return self.run("sgd", self.common("steepest_descent", epochs="2") + self.autosaving("sgd"))

    def resume(self, name, of, extra=(), expect_ok=True):
        return self.run(name, [BIN, "--continue", self.prefix(of) + "_epoch002.autosave", "--max_epochs", "3", "--autosave", "false"] + list(extra), expect_ok)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("lamb"))


def test_lamb_trains_and_prints_its_lines(runs):
    out, w, _ = runs.three()
    assert "Optimizer type: LAMB" in out and re.search(r"^Trust ratio bounds:\s+0\.001 / 100$", out, re.M)
    assert re.search(r"^Weight decay:\s+0\.01 \(in LAMB's direction", out, re.M)
    errs = _training_errors(out)
    assert len(errs) == 3 and errs[2] < errs[0], errs
    lines = TRUST_LINE.findall(out)
    assert len(lines) == 3
    for lo, lo_name, hi, hi_name in lines:
        assert 0.001 <= float(lo) <= float(hi) <= 100 and lo_name in runs.names and hi_name in runs.names
    assert any(np.abs(w[n] - np.concatenate([runs.initial[n][k] for k in ("input", "bias", "internal")])).max() > 1e-3 for n in w)
    free = runs.run("unbounded", runs.common(epochs="1"))
    assert re.search(r"^Trust ratio bounds:\s+0 / unbounded$", free[0], re.M)


def test_two_runs_with_the_same_seed_save_the_same_bits(runs):
    again = runs.run("three_again", runs.common() + ["--weight_decay", "0.01", "--lamb_min_trust", "0.001", "--lamb_max_trust", "100"] + runs.autosaving("again"))
    assert _same(runs.three()[1], again[1])
    assert TRUST_LINE.findall(runs.three()[0]) == TRUST_LINE.findall(again[0])


def test_two_epochs_and_a_continued_third_equal_three(runs):
    """The two epochs are the first two of the three-epoch run, as its autosave of epoch 2 holds them: a run that ENDS at epoch 2
    saves optimizer_finished = true, and --continue resumes that too (Optimizer.cu:326-358), for every optimizer."""
    whole = runs.three()
    auto = json.load(open(runs.prefix("three") + "_epoch002.autosave"))
    assert auto["lamb_optimizer"] is True and auto["adam_optimizer_step"] == 4            # 6 sequences, 3 at a time, 2 epochs
    assert np.float32(auto["lamb_optimizer_min_trust"]) == np.float32(0.001) and np.float32(auto["lamb_optimizer_max_trust"]) == np.float32(100)
    for key in ("adam_optimizer_first_moments", "adam_optimizer_second_moments"):
        assert any(np.abs(np.asarray(a)).max() > 0 for a in auto[key] if len(a))
    assert "optimizer=lamb;" in auto["configuration"] and "steepest_descent_optimizer_weight_deltas" not in auto
    assert auto["optimizer_finished"] is False
    resumed = runs.resume("resumed", "three")
    assert "Restoring state from" in resumed[0] and "Optimizer type: LAMB" in resumed[0]
    assert re.search(r"^Trust ratio bounds:\s+0\.001 / 100$", resumed[0], re.M)
    for name, ref in whole[1].items():
        assert np.array_equal(ref, resumed[1][name]), (name, float(np.abs(ref - resumed[1][name]).max()))
    assert TRUST_LINE.findall(resumed[0]) == TRUST_LINE.findall(whole[0])[2:]


def test_batch_learning_runs(runs):
    out, w, _ = runs.run("batch", runs.common(stochastic="false") + ["--max_grad_norm", "100"])
    errs = _training_errors(out)
    assert len(errs) == 3 and errs[2] < errs[0], errs
    assert len(TRUST_LINE.findall(out)) == 3 and "gradient norm: max" in out
    assert not _same(w, runs.three()[1])


@pytest.mark.parametrize("of,optimizer", [("adam", "lamb"), ("three", "adam"), ("three", "steepest_descent"), ("adam", "steepest_descent"), ("sgd", "lamb")])
def test_cross_optimizer_continues_are_refused(runs, of, optimizer):
    getattr(runs, of)()
    writer = {"three": "lamb", "adam": "adam", "sgd": "steepest_descent"}[of]
    out, w, rc = runs.resume("refused_%s_%s" % (of, optimizer), of, ["--optimizer", optimizer], expect_ok=False)
    assert rc == 2 and w is None
    assert "FAILED: The autosave file was written by the %s optimizer and cannot be continued with %s" % (writer, optimizer) in out


def test_adam_prints_none_of_the_new_lines(runs):
    out = runs.adam()[0]
    assert "Optimizer type: Adam" in out and not any(s in out for s in NEW_LINES)
    assert "lamb_optimizer" not in json.load(open(runs.prefix("adam") + "_epoch002.autosave"))
