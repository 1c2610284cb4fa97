"""CPU: the numpy restatement of input splicing and frame skipping (tests/splice_reference.py) against make_fraction, the host
path of the same rule, and the declarations of the C ABI.

The shapes are those of tests/test_gpu_splice.py: 5 features, 5 slots holding sequences of 12, 8, 2 and 1 frames and an empty one,
contexts (0, 0), (1, 2), (2, 0), skips 1, 2, 3: a length the skip divides, ragged last groups where the gather clamps at the last
frame, one network frame from 2 frames and from 1, K > B (frames never read) and K < B.

The C++ driver without a GPU: --input_frame_skip and --input_splice_on_device parse, bad values are refused in the parse-error
wording, the usage text names them, and --dump_fractions on tests/golden/val_1_speaker.nc prints the network-rate lengths the
restatement predicts, whichever side splices."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import splice_reference as SR
from helpers import GOLDEN, net_desc, random_sequences
from test_reference_test1 import BIN, ensure_built, read_real_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0, C, PS, T = 5, 4, 5, 12
LENGTHS = [12, 8, 2, 1]
CONTEXTS = [(0, 0), (1, 2), (2, 0)]
SKIPS = [1, 2, 3]
KEYS = ("inputs", "patTypes", "targetClasses")


def sequences(classes=True):
    return random_sequences(np.random.RandomState(2000), LENGTHS, P0, C=C) if classes else random_sequences(np.random.RandomState(2000), LENGTHS, P0, L=3)


def assert_same_fraction(a, b, keys=KEYS):
    for k in ("T", "Tmin", "PS", "numSeqs", "seqLengths"):
        assert a[k] == b[k], k
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("context", CONTEXTS)
def test_skip_one_is_the_host_splice(pkg, context):
    xs, ts = sequences()
    got = SR.network_fraction(pkg.make_fraction(xs, ts, PS), context, 1)
    assert_same_fraction(got, pkg.make_fraction(xs, ts, PS, context_left=context[0], context_right=context[1]))


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("context", CONTEXTS)
def test_a_skip_keeps_rows_k_j_with_fresh_pattern_types(pkg, context, k):
    xs, ts = sequences()
    got = SR.network_fraction(pkg.make_fraction(xs, ts, PS), context, k)
    spliced = pkg.make_fraction(xs, ts, PS, context_left=context[0], context_right=context[1])
    Tn = -(-T // k)
    assert (got["T"], got["Tmin"]) == (Tn, 1) and got["seqLengths"] == [-(-n // k) for n in LENGTHS]
    assert got["inputs"].tobytes() == spliced["inputs"].reshape(T, PS, -1)[::k].tobytes()
    assert got["targetClasses"].tobytes() == spliced["targetClasses"].reshape(T, PS)[::k].tobytes()
    # the pattern types of sequences of n_s frames: what make_fraction gives such sequences
    short = pkg.make_fraction([x[:-(-len(x) // k)] for x in xs], [t[:-(-len(t) // k)] for t in ts], PS)
    assert short["T"] == Tn and got["patTypes"].tobytes() == short["patTypes"].tobytes()
    # the ragged last group clamps at the last frame; with K > B some frames are never read
    x = got["inputs"].reshape(Tn, PS, -1)
    if context == (1, 2) and k == 3:
        assert x[2, 1, 15:].tobytes() == xs[1][7].tobytes() and x[2, 1, 10:15].tobytes() == xs[1][7].tobytes()      # frames 8, 9 of 8
    if context == (0, 0) and k == 3:
        assert not any((x[:, 0] == xs[0][1]).all(axis=-1))


@pytest.mark.parametrize("k", SKIPS)
@pytest.mark.parametrize("context", CONTEXTS)
def test_make_fraction_with_a_frame_skip_is_the_restatement(pkg, context, k):
    xs, ts = sequences()
    host = pkg.make_fraction(xs, ts, PS, context_left=context[0], context_right=context[1], frame_skip=k)
    assert_same_fraction(host, SR.network_fraction(pkg.make_fraction(xs, ts, PS), context, k))
    if k == 1:
        assert_same_fraction(host, pkg.make_fraction(xs, ts, PS, context_left=context[0], context_right=context[1]))


@pytest.mark.parametrize("k", SKIPS)
def test_target_rows_are_those_of_source_row_k_j(pkg, k):
    xs, ts = sequences(classes=False)
    src = pkg.make_fraction(xs, ts, PS, classification=False)
    got = SR.network_fraction(src, (1, 2), k)
    host = pkg.make_fraction(xs, ts, PS, classification=False, context_left=1, context_right=2, frame_skip=k)
    assert_same_fraction(got, host, ("inputs", "patTypes", "targets"))
    assert got["targets"].tobytes() == src["targets"].reshape(T, PS, 3)[::k].tobytes()


def test_a_frame_skip_below_one_is_refused(pkg):
    xs, ts = sequences()
    with pytest.raises(ValueError):
        pkg.make_fraction(xs, ts, PS, frame_skip=0)


def test_the_symbol_the_struct_and_the_method_are_declared(pkg):
    header = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    assert re.search(r"int\s+cn_ctx_set_input_splice\(cn_ctx \*ctx, const cn_input_splice \*s\);", header)
    assert re.search(r"typedef struct cn_input_splice \{ int context_left, context_right, frame_skip; \} cn_input_splice;", header)
    assert "cn_ctx_set_input_splice" in pkg.binding.EXPORTS
    assert [f[0] for f in pkg.binding.InputSplice._fields_] == ["context_left", "context_right", "frame_skip"]
    assert hasattr(pkg.NeuralNetwork, "set_input_splice")


def test_the_library_exports_the_symbol(hiplib):
    assert hasattr(hiplib, "cn_ctx_set_input_splice")


# ---- the driver, no GPU --------------------------------------------------------------------------------------------------------
NC = os.path.join(GOLDEN, "val_1_speaker.nc")
PARSE_ERROR = "FAILED: Error while parsing the command line and/or options file: "


def _driver(args):
    ensure_built()
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=120)


def test_the_options_parse_and_the_usage_names_them():
    out = _driver(["--input_frame_skip", "3", "--input_splice_on_device", "true", "--help"])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "--input_frame_skip" in out.stdout and "--input_splice_on_device" in out.stdout
    assert _driver(["--input_frame_skip", "1", "--input_frame_skip", "16", "--input_splice_on_device", "false", "--help"]).returncode == 0
    # device augmentation: with the device's splice at any skip, with a skip of 1 either way; host noise at any skip; wide host contexts
    for args in (["--input_frame_skip", "2", "--input_splice_on_device", "true", "--input_noise_sigma", "0.3", "--input_noise_on_device", "true",
                  "--spec_augment_time_masks", "1"],
                 ["--input_frame_skip", "1", "--input_noise_sigma", "0.3", "--input_noise_on_device", "true", "--spec_augment_freq_masks", "1"],
                 ["--input_frame_skip", "2", "--input_noise_sigma", "0.3"],
                 ["--input_frame_skip", "2", "--input_noise_sigma", "0", "--input_noise_on_device", "true"],
                 ["--input_left_context", "33"], ["--input_splice_on_device", "true", "--input_left_context", "32", "--input_right_context", "32"]):
        out = _driver(args + ["--help"])
        assert out.returncode == 0, (args, out.stdout)


@pytest.mark.parametrize("args,message", [
    (["--input_frame_skip", "0"], "--input_frame_skip must be in 1..16"),
    (["--input_frame_skip", "-2"], "--input_frame_skip must be in 1..16"),
    (["--input_frame_skip", "17"], "--input_frame_skip must be in 1..16"),
    (["--input_frame_skip", "two"], "--input_frame_skip must be in 1..16"),
    (["--input_splice_on_device", "perhaps"], "invalid value 'perhaps' for option 'input_splice_on_device'"),
    # the device's augmentation is stated on the source frames: fractions the host has skipped frames of cannot take it
    (["--input_frame_skip", "2", "--input_noise_sigma", "0.3", "--input_noise_on_device", "true"],
     "--input_noise_on_device and --spec_augment_* with --input_frame_skip above 1 need --input_splice_on_device true"),
    (["--input_frame_skip", "3", "--spec_augment_time_masks", "1", "--input_splice_on_device", "false"],
     "--input_noise_on_device and --spec_augment_* with --input_frame_skip above 1 need --input_splice_on_device true"),
    (["--input_frame_skip", "2", "--spec_augment_freq_masks", "2"],
     "--input_noise_on_device and --spec_augment_* with --input_frame_skip above 1 need --input_splice_on_device true"),
    # cn_ctx_set_input_splice takes at most 32 frames per side
    (["--input_splice_on_device", "true", "--input_left_context", "33"], "--input_splice_on_device true needs --input_left_context and --input_right_context in 0..32"),
    (["--input_splice_on_device", "true", "--input_right_context", "40"], "--input_splice_on_device true needs --input_left_context and --input_right_context in 0..32"),
])
def test_bad_values_are_refused(args, message):
    out = _driver(args + ["--help"])
    assert out.returncode == 2, out.stdout + out.stderr
    assert PARSE_ERROR + message in out.stdout


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("k", [2, 3])
def test_dump_fractions_prints_the_network_rate_lengths(pkg, tmp_path, k, on_device):
    """context (1, 1), 12 sequences of the real file in fractions of 5 (the last one with 2): T, Tmin, the NONE count and the
    lengths are those of the restatement; the sums are those of what is uploaded (the host-built network-rate fraction, or the
    unspliced source-rate one)"""
    dims, tags, xs, ts = read_real_file()
    net = str(tmp_path / "network.jsn")
    json.dump({"layers": net_desc(3 * 39, [("lstm", 8)], 51)}, open(net, "w"))
    out = _driver(["--train", "true", "--dump_fractions", "true", "--train_file", NC, "--train_fraction", "0.12", "--network", net,
                   "--parallel_sequences", "5", "--input_left_context", "1", "--input_right_context", "1", "--input_frame_skip", str(k),
                   "--input_splice_on_device", "true" if on_device else "false"])
    assert out.returncode == 0, out.stdout + out.stderr
    assert ("Input frame skip: %d" % k) in out.stdout and ("Input splicing:   on the device" in out.stdout) == on_device
    rows = [dict(p.split("=", 1) for p in l.split()[2:]) for l in out.stdout.splitlines() if l.startswith("FRACTION")]
    assert [int(r["seqs"]) for r in rows] == [5, 5, 2]
    index = {t: i for i, t in enumerate(tags)}
    for r in rows:
        mine = [index[t] for t in r["tags"].split(",")]
        src = pkg.make_fraction([xs[i] for i in mine], [ts[i] for i in mine], 5)
        want = SR.network_fraction(src, (1, 1), k)
        assert (int(r["T"]), int(r["Tmin"])) == (want["T"], want["Tmin"]) == (-(-src["T"] // k), -(-src["Tmin"] // k))
        assert [int(n) for n in r["lens"].split(",")] == want["seqLengths"]
        assert int(r["none"]) == int((want["patTypes"] == 0).sum())
        up = src if on_device else want
        assert abs(float(r["sum_inputs"]) - float(up["inputs"].astype(np.float64).sum())) < 1e-3
        assert int(r["sum_targets"]) == int(up["targetClasses"][up["targetClasses"] >= 0].sum())
    # the frames a per-frame error rate is taken over: the restatement's network-rate lengths, summed
    frames = re.search(r"^Input frame skip: %d \(the network sees sequences of (\d+)\.\.(\d+) frames, (\d+) frames in all\)$" % k, out.stdout, re.M)
    lens = [int(n) for r in rows for n in r["lens"].split(",")]
    assert frames and [int(v) for v in frames.groups()] == [min(lens), max(lens), sum(lens)]
    assert sum(lens) == sum(-(-len(xs[index[t]]) // k) for r in rows for t in r["tags"].split(","))


@pytest.mark.parametrize("on_device", [False, True])
def test_the_frame_count_takes_the_pieces_of_truncate_seq_one_by_one(pkg, tmp_path, on_device):
    """--truncate_seq cuts at source rate and every piece is a sequence of its own: ceil(piece / K) frames each"""
    dims, tags, xs, ts = read_real_file()
    k, trunc = 3, 50
    net = str(tmp_path / "network.jsn")
    json.dump({"layers": net_desc(39, [("lstm", 8)], 51)}, open(net, "w"))
    out = _driver(["--train", "true", "--dump_fractions", "true", "--train_file", NC, "--train_fraction", "0.06", "--network", net,
                   "--parallel_sequences", "4", "--truncate_seq", str(trunc), "--input_frame_skip", str(k),
                   "--input_splice_on_device", "true" if on_device else "false"])
    assert out.returncode == 0, out.stdout + out.stderr
    pieces = [n for x in xs[:6] for n in pkg.fraction.truncated_pieces(len(x), trunc)]
    assert len(pieces) > 6 and any(n % k for n in pieces)
    want = sorted(-(-n // k) for n in pieces)
    rows = [dict(p.split("=", 1) for p in l.split()[2:]) for l in out.stdout.splitlines() if l.startswith("FRACTION")]
    assert sorted(int(n) for r in rows for n in r["lens"].split(",")) == want
    assert ("frames, %d frames in all)" % sum(want)) in out.stdout and sum(want) != -(-sum(pieces) // k)
