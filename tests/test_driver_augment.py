"""`--input_noise_on_device` and `--spec_augment_*` in the C++ driver (lstm-rnn_amd/currennt_hip).  Without a GPU: the options
parse, bad values are refused with the reference's message and the usage text names them.  -m gpu, on a few sequences of
tests/golden/val_1_speaker.nc (39 -> lstm 8 -> softmax 51): one seed gives one network, another seed or no augmentation gives
another, --continue resumes the same augmentation, and the data-set block names what is active."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, net_desc, random_weights
from test_host_driver import BIN, _weights_of, problem

NC = os.path.join(GOLDEN, "val_1_speaker.nc")
PARSE_ERROR = "FAILED: Error while parsing the command line and/or options file: "
OPTIONS = ["--input_noise_on_device", "--spec_augment_freq_masks", "--spec_augment_freq_width", "--spec_augment_time_masks",
           "--spec_augment_time_width", "--spec_augment_time_ratio"]
DEVICE = ["--input_noise_sigma", "0.3", "--input_noise_on_device", "true", "--spec_augment_freq_masks", "2", "--spec_augment_freq_width", "8",
          "--spec_augment_time_masks", "2", "--spec_augment_time_width", "10", "--spec_augment_time_ratio", "0.5"]
NOISE_LINE = re.compile(r"^Input noise:\s+sigma (\S+), generated on the device$", re.M)
SPEC_LINE = re.compile(r"^SpecAugment:\s+(\d+) frequency masks of up to (\d+) features, (\d+) time masks of up to (\d+) frames "
                       r"\(at most (\S+) of a sequence\), on the device$", re.M)


def _driver(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)


def test_the_options_parse_and_the_usage_names_them():
    out = _driver(DEVICE + ["--help"])
    assert out.returncode == 0, out.stdout + out.stderr
    for name in OPTIONS:
        assert name in out.stdout, name
    out = _driver(["--spec_augment_freq_mask", "2", "--help"])                   # (a misspelt one is still unknown)
    assert out.returncode == 2 and PARSE_ERROR + "unknown option 'spec_augment_freq_mask'" in out.stdout


@pytest.mark.parametrize("args,message", [
    (["--spec_augment_freq_masks", "9"], "--spec_augment_freq_masks must be in 0..8"),
    (["--spec_augment_freq_masks", "-1"], "--spec_augment_freq_masks must be in 0..8"),
    (["--spec_augment_time_masks", "9"], "--spec_augment_time_masks must be in 0..8"),
    (["--spec_augment_freq_width", "-1"], "--spec_augment_freq_width must be >= 0"),
    (["--spec_augment_time_width", "-2"], "--spec_augment_time_width must be >= 0"),
    (["--spec_augment_time_ratio", "1.5"], "--spec_augment_time_ratio must be in 0..1"),
    (["--spec_augment_time_ratio", "-0.1"], "--spec_augment_time_ratio must be in 0..1"),
    (["--spec_augment_time_ratio", "nan"], "--spec_augment_time_ratio must be in 0..1"),
    (["--input_noise_on_device", "maybe"], "invalid value 'maybe' for option 'input_noise_on_device'"),
])
def test_bad_values_are_refused(args, message):
    out = _driver(args + ["--help"])
    assert out.returncode == 2, out.stdout + out.stderr
    assert PARSE_ERROR + message in out.stdout


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("augment")
    net = str(tmp / "network.jsn")
    layers = net_desc(39, [("lstm", 8)], 51)
    weights = random_weights(layers, np.random.RandomState(27), 0.3)
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    common = ["--train", "true", "--stochastic", "true", "--train_file", NC, "--train_fraction", "0.06", "--val_file", NC, "--val_fraction", "0.06",
              "--network", net, "--parallel_sequences", "3", "--learning_rate", "1e-2", "--momentum", "0.9", "--precision", "f32",
              "--deterministic", "true", "--shuffle_fractions", "false", "--shuffle_sequences", "false", "--max_epochs", "4"]
    out = {}

    def run(name, extra):
        path = str(tmp / (name + ".jsn"))
        r = _driver(common + extra + ["--save_network", path])
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = (r.stdout, _weights_of(path), open(path, "rb").read())

    prefix = str(tmp / "auto")
    run("device", DEVICE + ["--random_seed", "3", "--autosave", "true", "--autosave_prefix", prefix])
    run("device_again", DEVICE + ["--random_seed", "3"])
    run("other_seed", DEVICE + ["--random_seed", "4"])
    run("off", ["--random_seed", "3"])
    run("noise_only", DEVICE[:4] + ["--random_seed", "3"])
    resumed = str(tmp / "resumed.jsn")
    r = _driver(["--continue", prefix + "_epoch002.autosave", "--max_epochs", "4", "--autosave", "false", "--save_network", resumed])
    assert r.returncode == 0, r.stdout + r.stderr
    out["resumed"] = (r.stdout, _weights_of(resumed), None)
    out["autosave"] = json.load(open(prefix + "_epoch002.autosave"))
    return out


def _apart(a, b):
    return max(float(np.abs(a[1][n] - b[1][n]).max()) for n in a[1])


@pytest.mark.gpu
def test_one_seed_one_network(runs):
    assert runs["device"][2] == runs["device_again"][2]            # the saved files, byte for byte
    assert _apart(runs["device"], runs["other_seed"]) > 1e-5       # (the seed reaches nothing else here: given weights, no shuffling)
    assert _apart(runs["device"], runs["off"]) > 1e-4
    assert _apart(runs["device"], runs["noise_only"]) > 1e-5       # the masks are not merely parsed
    assert _apart(runs["noise_only"], runs["off"]) > 1e-5


@pytest.mark.gpu
def test_continue_resumes_the_same_augmentation(runs):
    """the epoch-2 autosave of the 4-epoch run carries the options, and its continuation ends in the same weights (2e-6: the
    precision of the autosave's text, as in test_host_driver.py)"""
    for opt in ("input_noise_on_device=true;", "input_noise_sigma=0.3;", "spec_augment_time_ratio=0.5;", "spec_augment_freq_masks=2;"):
        assert opt in runs["autosave"]["configuration"], opt
    text, w, _ = runs["resumed"]
    assert "Restoring state from" in text
    for name, ref in runs["device"][1].items():
        assert np.abs(ref - w[name]).max() < 2e-6, (name, float(np.abs(ref - w[name]).max()))


@pytest.mark.gpu
def test_a_forward_pass_takes_the_device_noise_and_never_masks(tmp_path):
    """--ff_input_file is the other set that gets input noise: with --input_noise_on_device one seed gives one output file,
    another seed or no noise another, and the --spec_augment_* options change nothing (only training fractions are masked)"""
    _, _, _, _, nc, net = problem(tmp_path)
    base = ["--train", "false", "--ff_input_file", nc, "--network", net, "--parallel_sequences", "4", "--ff_output_format", "single_csv",
            "--revert_std", "false", "--precision", "f32"]
    noise = ["--input_noise_sigma", "0.3", "--input_noise_on_device", "true"]
    got = {}
    for name, extra in (("clean", []), ("noisy", noise + ["--random_seed", "3"]), ("noisy_again", noise + ["--random_seed", "3"]),
                        ("other_seed", noise + ["--random_seed", "4"]), ("with_mask_options", noise + DEVICE[4:] + ["--random_seed", "3"])):
        path = str(tmp_path / (name + ".csv"))
        r = _driver(base + extra + ["--ff_output_file", path])
        assert r.returncode == 0, r.stdout + r.stderr
        got[name] = (r.stdout, open(path, "rb").read())
    assert got["noisy"][1] == got["noisy_again"][1] == got["with_mask_options"][1]
    assert got["noisy"][1] != got["clean"][1] and got["noisy"][1] != got["other_seed"][1]
    assert NOISE_LINE.findall(got["noisy"][0]) == ["0.3"] and "Input noise" not in got["clean"][0]
    assert not SPEC_LINE.findall(got["with_mask_options"][0])


@pytest.mark.gpu
def test_the_data_set_block_names_what_is_active(runs):
    for name in ("device", "resumed"):
        text = runs[name][0]
        assert NOISE_LINE.findall(text) == ["0.3"], name               # the training set's block, not the validation set's
        assert SPEC_LINE.findall(text) == [("2", "8", "2", "10", "0.5")], name
    assert NOISE_LINE.findall(runs["noise_only"][0]) == ["0.3"] and not SPEC_LINE.findall(runs["noise_only"][0])
    assert "Input noise" not in runs["off"][0] and "SpecAugment" not in runs["off"][0]
