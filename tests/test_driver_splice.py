"""-m gpu: `--input_frame_skip` and `--input_splice_on_device` in the C++ driver (lstm-rnn_amd/currennt_hip), on a few sequences of
tests/golden/val_1_speaker.nc (39 x 3 -> lstm 8 -> softmax 51, f32, two epochs): splicing and skipping on the device trains the
very network that the host path of the same rule trains, a skip changes it, the data-set block names what is active, and the
forward pass writes one row per network frame; the reported classification error is taken over the frames the network classifies;
the device's augmentation runs with the device's splice at a skip.  (The options' parsing and --dump_fractions:
tests/test_splice_reference.py.)"""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, net_desc, random_weights
from test_driver_augment import _driver
from test_host_driver import _weights_of
from test_reference_test1 import read_real_file

pytestmark = pytest.mark.gpu
NC = os.path.join(GOLDEN, "val_1_speaker.nc")
CONTEXT = ["--input_left_context", "1", "--input_right_context", "1"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("splice")
    net = str(tmp / "network.jsn")
    layers = net_desc(3 * 39, [("lstm", 8)], 51)
    weights = random_weights(layers, np.random.RandomState(27), 0.3)
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    common = ["--train", "true", "--stochastic", "true", "--train_file", NC, "--train_fraction", "0.06", "--val_file", NC, "--val_fraction", "0.06",
              "--network", net, "--parallel_sequences", "3", "--learning_rate", "1e-2", "--momentum", "0.9", "--precision", "f32",
              "--deterministic", "true", "--shuffle_fractions", "false", "--shuffle_sequences", "false", "--max_epochs", "2", "--random_seed", "3"] + CONTEXT
    out = {"net": net, "tmp": tmp}
    for name, extra in (("host k2", ["--input_frame_skip", "2"]), ("device k2", ["--input_frame_skip", "2", "--input_splice_on_device", "true"]),
                        ("host k1", []), ("device k1", ["--input_splice_on_device", "true"])):
        path = str(tmp / (name.replace(" ", "_") + ".jsn"))
        r = _driver(common + extra + ["--save_network", path])
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = (r.stdout, _weights_of(path))
    # ... with the device's augmentation on top (it needs the device's splice at a skip above 1), twice
    aug = ["--input_frame_skip", "2", "--input_splice_on_device", "true", "--input_noise_sigma", "0.3", "--input_noise_on_device", "true",
           "--spec_augment_freq_masks", "2", "--spec_augment_freq_width", "8", "--spec_augment_time_masks", "2", "--spec_augment_time_width", "10"]
    for name in ("device k2 augmented", "device k2 augmented again"):
        path = str(tmp / (name.replace(" ", "_") + ".jsn"))
        r = _driver(common + aug + ["--save_network", path])
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = (r.stdout, _weights_of(path))
    # ... and with a learning rate of 0: the weights stay the file's, the error columns are those of a plain forward pass
    for name, extra in (("host k2 frozen", ["--input_frame_skip", "2"]), ("device k2 frozen", ["--input_frame_skip", "2", "--input_splice_on_device", "true"])):
        r = _driver([a if a != "1e-2" else "0" for a in common] + extra + ["--save_network", str(tmp / "frozen.jsn")])
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = (r.stdout, None)
    out["layers"], out["weights"] = layers, weights
    return out


def _error_columns(text):
    """[(classification error %, error per sequence) of the training and of the validation column] per epoch row of the driver's table"""
    rows = []
    for l in text.splitlines():
        if l.strip()[:1].isdigit() and "|" in l:
            cells = [c.strip() for c in l.split("|")]
            rows.append([tuple(float(v.rstrip("%")) for v in cells[i].split()) for i in (2, 3)])
    return rows


def test_the_class_error_is_taken_over_the_frames_the_network_classifies(pkg, runs):
    """learning rate 0, skip 2: the printed training and validation class errors are 1 - correct / sum of ceil(len / 2), with
    `correct` counted by the library from Python on the host-built fractions of the same six sequences -- not over the source frames,
    which would keep the figure above 50 %"""
    dims, tags, xs, ts = read_real_file()
    xs, ts = xs[:6], ts[:6]                                     # --train_fraction 0.06 of 102 sequences
    correct = 0
    with pkg.NeuralNetwork(runs["layers"], runs["weights"], 3, 80, precision=pkg.PREC_F32, deterministic=True) as net:
        for i in (0, 3):
            net.load_sequences(pkg.make_fraction(xs[i:i + 3], ts[i:i + 3], 3, context_left=1, context_right=1, frame_skip=2))
            net.compute_forward_pass()
            correct += net.error_and_correct()[1]
    frames = sum(-(-len(x) // 2) for x in xs)
    want = 100.0 * (1.0 - correct / frames)
    assert 0 < correct < frames and want < 100.0 * (1.0 - correct / sum(len(x) for x in xs))
    for name in ("host k2 frozen", "device k2 frozen"):
        rows = _error_columns(runs[name][0])
        assert len(rows) == 2, runs[name][0]
        for train, val in rows:
            assert abs(train[0] - want) <= 0.0051 and abs(val[0] - want) <= 0.0051, (name, train, val, want)      # (printed to 0.01 %)


def test_the_device_augments_behind_its_own_splice_at_a_skip(runs):
    a, again, plain = runs["device k2 augmented"][1], runs["device k2 augmented again"][1], runs["device k2"][1]
    assert all(a[n].tobytes() == again[n].tobytes() for n in a) and any(a[n].tobytes() != plain[n].tobytes() for n in a)
    assert "Input noise:      sigma 0.3, generated on the device" in runs["device k2 augmented"][0]
    assert "Input splicing:   on the device" in runs["device k2 augmented"][0]


@pytest.mark.parametrize("k", ["k1", "k2"])
def test_splicing_on_the_device_trains_the_same_network(runs, k):
    host, device = runs["host " + k][1], runs["device " + k][1]
    assert host.keys() == device.keys()
    for name in host:
        assert host[name].tobytes() == device[name].tobytes(), (name, float(np.abs(host[name] - device[name]).max()))


def test_a_skip_trains_another_network(runs):
    a, b = runs["host k1"][1], runs["host k2"][1]
    assert any(a[name].tobytes() != b[name].tobytes() for name in a)


def test_the_data_set_block_names_what_is_active(runs):
    for name in ("host k1", "host k2", "device k1", "device k2"):
        text = runs[name][0]
        assert ("Input frame skip: 2 " in text) == name.endswith("k2"), name
        assert ("Input splicing:   on the device (context 1 + 1 frames" in text) == name.startswith("device"), name
    assert runs["device k2"][0].count("Input frame skip: 2 ") == 2            # the training and the validation set


def test_the_forward_pass_writes_one_row_per_network_frame(runs):
    """--ff_input_file at a skip of 2, csv output: ceil(len / 2) rows per sequence, the same ones whichever side splices"""
    dims, tags, xs, ts = read_real_file()
    written = []
    for on_device in (False, True):
        cdir = str(runs["tmp"] / ("csv_device" if on_device else "csv_host"))
        r = _driver(["--train", "false", "--ff_input_file", NC, "--network", runs["net"], "--parallel_sequences", "3", "--ff_output_file", cdir,
                     "--ff_output_format", "csv", "--revert_std", "false", "--precision", "f32", "--input_frame_skip", "2",
                     "--input_splice_on_device", "true" if on_device else "false"] + CONTEXT)
        assert r.returncode == 0, r.stdout + r.stderr
        rows = {}
        for tag, x in zip(tags, xs):
            path = os.path.join(cdir, os.path.splitext(tag)[0] + ".csv")
            assert os.path.exists(path), path
            rows[tag] = open(path).read().strip().split("\n")
            assert len(rows[tag]) == -(-len(x) // 2) and len(rows[tag][0].split(";")) == 51, tag
        written.append(rows)
    assert written[0] == written[1]


def test_an_htk_header_carries_the_network_frame_period(runs):
    """--ff_output_format htk at a skip of 2: ceil(len / 2) samples, a period of feature_period x 2 (10 ms -> 200000 x 100 ns)"""
    dims, tags, xs, ts = read_real_file()
    hdir = str(runs["tmp"] / "htk")
    r = _driver(["--train", "false", "--ff_input_file", NC, "--network", runs["net"], "--parallel_sequences", "3", "--ff_output_file", hdir,
                 "--ff_output_format", "htk", "--revert_std", "false", "--precision", "f32", "--input_frame_skip", "2",
                 "--input_splice_on_device", "true"] + CONTEXT)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag, x in list(zip(tags, xs))[:5]:
        raw = open(os.path.join(hdir, tag + ".htk"), "rb").read()
        n, period, bpf, kind = np.frombuffer(raw[:12], ">i4,>i4,>i2,>i2")[0]
        assert (n, period, bpf) == (-(-len(x) // 2), 200000, 51 * 4), tag
        assert len(raw) == 12 + n * bpf
