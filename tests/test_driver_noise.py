"""-m gpu: `--weight_noise_on_device` in the C++ driver, on the problem of test_host_driver.py (6 -> blstm 8 -> feedforward_tanh 5
-> softmax 4, seven sequences, three at a time): the noise never reaches the forward pass or the stored weights, one seed gives
one network, --continue resumes the same noise, and without the option the driver does what it did."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_host_driver import BIN, _table_rows, _weights_of, problem

pytestmark = pytest.mark.gpu
NOISE_LINE = re.compile(r"^Weight noise:\s+sigma (\S+), generated on the device$", re.M)


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _without_durations(text):
    """the driver's output with the one column that is a wall time blanked"""
    return [re.sub(r"^(\s+\d+ \|)\s+[\d.]+ \|", r"\1 D |", l) for l in text.splitlines()]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("noise")
    layers, weights, xs, ts, nc, net = problem(tmp)
    common = [BIN, "--train", "true", "--train_file", nc, "--network", net, "--parallel_sequences", "3", "--momentum", "0.9",
              "--random_seed", "3", "--precision", "f32", "--deterministic", "true"]
    out = {"weights": weights, "common": common, "tmp": tmp}

    def run(name, extra):
        path = str(tmp / (name + ".jsn"))
        text = _run(common + extra + ["--save_network", path])
        out[name] = (text, _weights_of(path), open(path, "rb").read())

    on = ["--weight_noise_on_device", "true"]
    for st in ("true", "false"):
        mode = ["--stochastic", st, "--max_epochs", "3"]
        run("clean0_" + st, mode + ["--learning_rate", "0"])
        run("noisy0_" + st, mode + ["--learning_rate", "0", "--weight_noise_sigma", "0.5"] + on)
    train = ["--stochastic", "true", "--learning_rate", "1e-2"]
    run("clean", train + ["--max_epochs", "4"])
    prefix = str(tmp / "auto")
    run("noisy", train + ["--max_epochs", "4", "--weight_noise_sigma", "0.1", "--autosave", "true", "--autosave_prefix", prefix] + on)
    run("noisy_again", train + ["--max_epochs", "4", "--weight_noise_sigma", "0.1"] + on)
    run("other_seed", train + ["--max_epochs", "4", "--weight_noise_sigma", "0.1", "--random_seed", "4"] + on)
    resumed = str(tmp / "resumed.jsn")
    text = _run([BIN, "--continue", prefix + "_epoch002.autosave", "--max_epochs", "4", "--autosave", "false", "--save_network", resumed])
    out["resumed"] = (text, _weights_of(resumed), None)
    out["autosave"] = json.load(open(prefix + "_epoch002.autosave"))
    # the host stream, with and without naming the default
    run("host", train + ["--max_epochs", "3", "--weight_noise_sigma", "0.1"])
    run("host_explicit", train + ["--max_epochs", "3", "--weight_noise_sigma", "0.1", "--weight_noise_on_device", "false"])
    return out


@pytest.mark.parametrize("stochastic", ["true", "false"])
def test_noise_never_reaches_the_forward_pass_or_the_stored_weights(runs, stochastic):
    """learning rate 0: the training error of every epoch is a forward-pass quantity of the clean weights -- not a digit of the
    table changes under sigma 0.5 -- and the saved weights are the initial ones"""
    clean, noisy = runs["clean0_" + stochastic], runs["noisy0_" + stochastic]
    rows = [r[1] for r in _table_rows(clean[0])]
    assert len(rows) == 3 and [r[1] for r in _table_rows(noisy[0])] == rows and len(set(rows)) == 1
    for n, w in noisy[1].items():
        w0 = np.concatenate([np.asarray(runs["weights"][n][k], np.float64).reshape(-1) for k in ("input", "bias", "internal")])
        assert np.abs(w - w0).max() < 1e-6, n                    # (the JSON text carries ~7 digits)
        assert np.array_equal(w, clean[1][n]), n


def test_one_seed_one_network(runs):
    assert runs["noisy"][2] == runs["noisy_again"][2]             # the saved files, byte for byte
    moved = max(np.abs(runs["noisy"][1][n] - runs["clean"][1][n]).max() for n in runs["clean"][1])
    assert moved > 1e-4                                           # the noisy backward passes led somewhere else
    other = max(np.abs(runs["noisy"][1][n] - runs["other_seed"][1][n]).max() for n in runs["clean"][1])
    assert other > 1e-5
    # the forward pass of epoch 1's first fraction saw the clean initial weights; the table moves from there
    assert [r[1] for r in _table_rows(runs["noisy"][0])] != [r[1] for r in _table_rows(runs["clean"][0])]


def test_the_optimizer_block_names_the_noise_only_with_the_option(runs):
    assert NOISE_LINE.findall(runs["noisy"][0]) == ["0.1"]
    assert NOISE_LINE.findall(runs["noisy0_true"][0]) == ["0.5"]
    for name in ("clean", "host", "host_explicit"):
        assert not NOISE_LINE.findall(runs[name][0]) and "Weight noise" not in runs[name][0], name


def test_continue_resumes_the_same_noise(runs):
    """the epoch-2 autosave of the 4-epoch run carries the option, and its continuation ends in the same weights (2e-6: the
    precision of the autosave's text, as in test_host_driver.py)"""
    assert "weight_noise_on_device=true;" in runs["autosave"]["configuration"]
    assert "weight_noise_sigma=0.1;" in runs["autosave"]["configuration"]
    text, w, _ = runs["resumed"]
    assert "Restoring state from" in text and NOISE_LINE.findall(text) == ["0.1"]
    for name, ref in runs["noisy"][1].items():
        assert np.abs(ref - w[name]).max() < 2e-6, (name, float(np.abs(ref - w[name]).max()))
    assert [r[1] for r in _table_rows(text)] == [r[1] for r in _table_rows(runs["noisy"][0])]


def test_the_default_is_the_host_stream(runs):
    """without the option, and with an explicit `false`, the driver prints and saves the same thing, byte for byte (durations
    aside)"""
    a, b = runs["host"], runs["host_explicit"]
    assert a[2] == b[2]
    assert _without_durations(a[0].replace("host.jsn", "X.jsn")) == _without_durations(b[0].replace("host_explicit.jsn", "X.jsn"))
    moved = max(np.abs(a[1][n] - runs["noisy"][1][n]).max() for n in a[1])
    assert moved > 1e-5                                            # (another stream of noise than the device's)
