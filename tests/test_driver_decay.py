"""-m gpu: `--weight_decay` and the learning-rate schedule options in the C++ driver, on a few sequences of
tests/golden/val_1_speaker.nc (39 -> lstm 8 -> softmax 51, PS 3, deterministic, no shuffling; the command-line skeleton of
test_driver_clip.py)."""
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
LR_LINE = re.compile(r"^\s+learning rate: (\S+) \(scale (\S+), (\d+) updates\)$", re.M)
NEW_LINES = ("Weight decay:", "Learning rate schedule:", "learning rate:")


def _weights_of(path):
    doc = json.load(open(path))
    return {n: np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in ("input", "bias", "internal")]) for n, w in doc["weights"].items()}


def _same(a, b):
    return all(np.array_equal(a[n], b[n]) for n in a)


def _rows(text):
    """the epoch table's rows, durations aside"""
    return [re.sub(r"\|\s+[\d.]+ \|", "| D |", l, count=1) for l in text.splitlines() if re.match(r"^\s+\d+ \|", l)]


class Runs:
    """runs of the driver by name, each made once"""

    def __init__(self, tmp):
        self.tmp = tmp
        self.nc = os.path.join(GOLDEN, "val_1_speaker.nc")
        rng = np.random.RandomState(61)
        layers = net_desc(39, [("lstm", 8)], 51)
        self.initial = random_weights(layers, rng, 0.1)
        self.net = str(tmp / "network.jsn")
        json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in self.initial.items()}},
                  open(self.net, "w"))
        self.done = {}

    def common(self, fraction="0.06", epochs="3", rate="1e-3", momentum="0.9"):
        return [BIN, "--train", "true", "--stochastic", "true", "--train_file", self.nc, "--train_fraction", fraction, "--network", self.net,
                "--parallel_sequences", "3", "--learning_rate", rate, "--momentum", momentum, "--deterministic", "true",
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

    def resume(self, name, of, epochs):
        return self.run(name, [BIN, "--continue", self.prefix(of) + "_epoch002.autosave", "--max_epochs", epochs, "--autosave", "false"])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("decay"))


VAL = lambda runs: ["--val_file", runs.nc, "--val_fraction", "0.06", "--max_epochs_no_best", "10"]


# ---- defaults --------------------------------------------------------------------------------------------------------------
def test_options_at_their_defaults_change_nothing(runs):
    plain = runs.run("plain", runs.common())
    zero = runs.run("zero", runs.common() + ["--weight_decay", "0", "--learning_rate_warmup_updates", "0", "--learning_rate_decay", "1",
                                             "--learning_rate_decay_patience", "1", "--learning_rate_min", "0"])
    assert _same(plain[1], zero[1])
    assert _rows(plain[0]) == _rows(zero[0]) and len(_rows(plain[0])) == 3
    for out in (plain[0], zero[0]):
        assert not any(s in out for s in NEW_LINES)


# ---- --weight_decay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["steepest_descent", "adam"])
def test_weight_decay_trains_elsewhere_is_saved_and_resumes(runs, optimizer):
    opt = ["--optimizer", optimizer]
    plain = runs.run("plain_" + optimizer, runs.common() + opt) if optimizer == "adam" else runs.run("plain", runs.common())
    wd = runs.run("wd_" + optimizer, runs.common() + opt + ["--weight_decay", "0.1"] + runs.autosaving(optimizer))
    assert not _same(plain[1], wd[1])
    assert re.search(r"^Weight decay:\s+0\.1 ", wd[0], re.M) and "Weight decay:" not in plain[0]
    assert "Learning rate schedule:" not in wd[0] and not LR_LINE.findall(wd[0])
    auto = json.load(open(runs.prefix(optimizer) + "_epoch002.autosave"))
    assert "weight_decay=0.1;" in auto["configuration"]
    assert "learning_rate_scale" not in auto                     # (no schedule: no schedule state)
    resumed = runs.resume("resumed_" + optimizer, optimizer, "3")
    assert "Restoring state from" in resumed[0] and re.search(r"^Weight decay:\s+0\.1 ", resumed[0], re.M)
    for name, ref in wd[1].items():
        assert np.array_equal(ref, resumed[1][name]), (name, float(np.abs(ref - resumed[1][name]).max()))


@pytest.mark.parametrize("bad", ["-1", "nan", "inf"])
def test_a_bad_weight_decay_is_a_parse_error(runs, bad):
    out, w, rc = runs.run("bad_" + bad, runs.common() + ["--weight_decay", bad], expect_ok=False)
    assert rc != 0 and w is None
    assert "Error while parsing the command line and/or options file: --weight_decay must be finite and >= 0" in out


@pytest.mark.parametrize("option,bad", [("learning_rate_warmup_updates", "-1"), ("learning_rate_decay", "0"), ("learning_rate_decay", "1.5"),
                                        ("learning_rate_decay_patience", "0"), ("learning_rate_min", "-1")])
def test_bad_schedule_options_are_parse_errors(runs, option, bad):
    out, w, rc = runs.run("bad_%s_%s" % (option, bad), runs.common() + ["--" + option, bad], expect_ok=False)
    assert rc != 0 and w is None
    assert "Error while parsing the command line and/or options file: --" + option in out


# ---- warm-up ---------------------------------------------------------------------------------------------------------------
def test_warmup_of_two_updates_halves_the_first_rate(runs):
    """momentum 0, steepest descent, ONE update (3 sequences, PS 3, 1 epoch): --learning_rate 1e-3 with a warm-up of 2 updates
    runs its only update at factor 1/2 -- halving a float is exact, so it is the float 5e-4 -- and ends in the bits of
    --learning_rate 5e-4 without a schedule; a warm-up of 1 update is the plain run."""
    one = lambda rate: runs.common(fraction="0.035", epochs="1", rate=rate, momentum="0")
    assert np.float32(1e-3) / np.float32(2) == np.float32(5e-4)
    full = runs.run("one_full", one("1e-3"))
    half = runs.run("one_half", one("5e-4"))
    warm2 = runs.run("one_warm2", one("1e-3") + ["--learning_rate_warmup_updates", "2"])
    warm1 = runs.run("one_warm1", one("1e-3") + ["--learning_rate_warmup_updates", "1"])
    assert "Sequences:        3\n" in full[0]
    assert not _same(full[1], half[1])
    assert _same(warm2[1], half[1])
    assert _same(warm1[1], full[1])
    assert re.search(r"^Learning rate schedule:\s+warm-up 2 updates", warm2[0], re.M)
    lines = LR_LINE.findall(warm2[0])
    assert len(lines) == 1 and lines[0] == ("0.001", "1", "1")                # the next update would run at the full rate


# ---- plateau ---------------------------------------------------------------------------------------------------------------
def test_a_forced_plateau_decays_every_epoch_down_to_the_floor(runs):
    """a rate so small that no weight changes its bits: the validation error repeats, and an equal error is no improvement"""
    base = runs.common(epochs="4", rate="1e-30") + VAL(runs) + ["--learning_rate_decay", "0.5", "--learning_rate_decay_patience", "1"]
    free = runs.run("plateau", base)
    floor = runs.run("plateau_floor", base + ["--learning_rate_min", "2.5e-31"])
    for out, w, _ in (free, floor):
        for name, ref in runs.initial.items():
            assert np.array_equal(w[name], np.concatenate([ref[k] for k in ("input", "bias", "internal")])), name       # no weight changed
        assert len(_rows(out)) == 4
    assert [l[1] for l in LR_LINE.findall(free[0])] == ["1", "0.5", "0.25", "0.125"]
    assert [l[1] for l in LR_LINE.findall(floor[0])] == ["1", "0.5", "0.25", "0.25"]
    assert [l[2] for l in LR_LINE.findall(free[0])] == ["2", "4", "6", "8"]              # 6 sequences, 3 at a time
    assert [float(l[0]) for l in LR_LINE.findall(free[0])] == [1e-30, 5e-31, 2.5e-31, 1.25e-31]
    assert [float(l[0]) for l in LR_LINE.findall(floor[0])] == [1e-30, 5e-31, 2.5e-31, 2.5e-31]


# ---- a real decay, and its resume -------------------------------------------------------------------------------------------
def test_a_real_decay_resumes_bit_for_bit(runs):
    """Adam at a rate large enough (30, warmed up over 12 updates: epoch 1 runs at 2.5 and 5, epoch 2 at 7.5 and 10) that the
    validation error of epoch 2 is above epoch 1's: the scale is below 1 in the autosave of epoch 2, and --continue from it ends in
    the uninterrupted run's network and prints its last `learning rate:` line"""
    args = runs.common(epochs="4", rate="30") + ["--optimizer", "adam"] + VAL(runs) + ["--learning_rate_decay", "0.5", "--learning_rate_warmup_updates", "12"]
    whole = runs.run("real", args + runs.autosaving("real"))
    lines = LR_LINE.findall(whole[0])
    assert len(lines) == 4
    assert float(lines[1][1]) < 1, lines                         # one decay happened by the end of epoch 2
    auto = json.load(open(runs.prefix("real") + "_epoch002.autosave"))
    assert auto["optimizer_updates"] == 4 and float(auto["learning_rate_scale"]) == float(lines[1][1])
    assert "learning_rate_bad_epochs" in auto and float(auto["learning_rate_lowest_error"]) > 0
    assert "learning_rate_decay=0.5;" in auto["configuration"]
    resumed = runs.resume("real_resumed", "real", "4")
    assert "Restoring state from" in resumed[0] and "starts fresh" not in resumed[0]
    for name, ref in whole[1].items():
        assert np.array_equal(ref, resumed[1][name]), (name, float(np.abs(ref - resumed[1][name]).max()))
    again = LR_LINE.findall(resumed[0])
    assert len(again) == 2 and again[-1] == lines[-1] and again[0] == lines[2]


def test_an_autosave_without_schedule_state_starts_the_schedule_fresh(runs):
    runs.run("wd_adam", runs.common() + ["--optimizer", "adam", "--weight_decay", "0.1"] + runs.autosaving("adam"))
    out, w, rc = runs.run("fresh", [BIN, "--continue", runs.prefix("adam") + "_epoch002.autosave", "--max_epochs", "3", "--autosave", "false",
                                    "--learning_rate_decay", "0.5"])
    assert "Learning rate schedule: the autosave file holds no schedule state; it starts fresh." in out
    lines = LR_LINE.findall(out)
    assert len(lines) == 1 and lines[0][2] == "2"                # its own count: the two updates of epoch 3
