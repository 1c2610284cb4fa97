"""Transcription data on the host, no GPU: the `labels` / `targetStrings` variables of a NetCDF file (the layout of RNNLIB's CTC
corpora) as data_sets::DataSet reads them -- `--dump_fractions true --dump_labels true` against the transcripts written --, and
what the driver refuses before it touches a device."""
import json
import subprocess

import numpy as np

from ctc_decode_reference import write_transcript_nc
from helpers import net_desc, random_weights
from test_ctc_host import ctc_network
from test_host_dataset import BIN, dump, make_file

P = 6
NAMES = ["a", "b", "sil", "dd"]
LENS = (14, 5, 9, 3, 11, 7, 12)
#              a a b: an immediate repeat                       the empty transcript
TRANSCRIPTS = [[0, 0, 1], [2], [3, 3, 3, 0], [], [1, 0, 1, 0, 2], [0], [3, 2, 2]]


def transcript_file(tmp_path, name="train.nc", transcripts=TRANSCRIPTS, with_classes=False, pad=" "):
    rng = np.random.RandomState(3)
    xs = [rng.randn(n, P).astype(np.float32) for n in LENS]
    ts = [rng.randint(0, len(NAMES), n).astype(np.int32) for n in LENS] if with_classes else None
    path = str(tmp_path / name)
    write_transcript_nc(path, xs, transcripts, NAMES, "a", ts=ts, pad=pad)
    return path, ts


def check_rows(rows, PS):
    by_tag = {"a%03d" % i: t for i, t in enumerate(TRANSCRIPTS)}
    assert len(rows) == (len(LENS) + PS - 1) // PS
    seen = []
    for kv in rows:
        seqs = [by_tag[t] for t in kv["tags"]]
        seen += kv["tags"]
        assert int(kv["label_seqs"]) == len(seqs)
        assert int(kv["labels_total"]) == sum(len(l) for l in seqs)
        assert int(kv["sum_labels"]) == sum(sum(l) for l in seqs)
    assert sorted(seen) == sorted(by_tag)


def run(args):
    out = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60)
    return out.returncode, out.stdout + out.stderr


def refused(args, *needles):
    code, text = run(args)
    assert code == 2 and "FAILED:" in text, text
    for n in needles:
        assert n in text, text
    assert "Creating the neural network" not in text, text          # before any device call
    return text


def test_transcripts_without_target_classes(tmp_path):
    for pad in (" ", "\0"):
        nc, _ = transcript_file(tmp_path, pad=pad)
        net = ctc_network(tmp_path, len(NAMES) + 1)
        text, (rows,) = dump(["--train_file", nc, "--network", net, "--parallel_sequences", "3", "--dump_labels", "true"])
        check_rows(rows, 3)
        assert "from targetStrings" in text
        assert all(int(kv["sum_targets"]) == 0 for kv in rows)
    # the labels belong to the sequence, not to its frames: skipping frames changes T, not the labels
    text, (rows,) = dump(["--train_file", nc, "--network", net, "--parallel_sequences", "2", "--dump_labels", "true", "--input_frame_skip", "3"])
    check_rows(rows, 2)
    # two shards of every fraction together hold every transcript once
    both = []
    for rank in (0, 1):
        _, (rows,) = dump(["--train_file", nc, "--network", net, "--parallel_sequences", "2", "--dump_labels", "true", "--dp_rank", str(rank), "--dp_world", "2"])
        both += rows
    assert sum(int(kv["labels_total"]) for kv in both) == sum(len(t) for t in TRANSCRIPTS)
    assert sum(int(kv["sum_labels"]) for kv in both) == sum(sum(t) for t in TRANSCRIPTS)


def test_both_variables_dump_the_transcripts(tmp_path):
    nc, ts = transcript_file(tmp_path, with_classes=True)
    net = ctc_network(tmp_path, len(NAMES) + 1)
    text, (rows,) = dump(["--train_file", nc, "--network", net, "--parallel_sequences", "3", "--dump_labels", "true"])
    check_rows(rows, 3)
    by_tag = {"a%03d" % i: t for i, t in enumerate(ts)}
    for kv in rows:                                                   # ... and the frames keep their classes
        assert int(kv["sum_targets"]) == sum(int(by_tag[t].sum()) for t in kv["tags"])


def test_a_file_without_target_strings_is_what_it_was(tmp_path):
    nc, xs, ts = make_file(tmp_path, "plain.nc", LENS, 4, "a")
    text, (rows,) = dump(["--train_file", nc, "--network", ctc_network(tmp_path, 5), "--parallel_sequences", "3", "--dump_labels", "true"])
    assert "targetStrings" not in text
    collapsed = {"a%03d" % i: [int(k) for j, k in enumerate(t) if j == 0 or k != t[j - 1]] for i, t in enumerate(ts)}
    for kv in rows:
        assert int(kv["labels_total"]) == sum(len(collapsed[t]) for t in kv["tags"])


def test_unknown_token_is_refused_with_token_and_tag(tmp_path):
    bad = list(TRANSCRIPTS)
    bad[4] = "b a  zz b"
    nc, _ = transcript_file(tmp_path, transcripts=bad)
    refused(["--train", "true", "--train_file", nc, "--network", ctc_network(tmp_path, len(NAMES) + 1), "--parallel_sequences", "3"],
            "'zz'", "a004")


def test_truncate_seq_is_refused(tmp_path):
    nc, _ = transcript_file(tmp_path)
    refused(["--train", "true", "--train_file", nc, "--network", ctc_network(tmp_path, len(NAMES) + 1), "--parallel_sequences", "3",
             "--truncate_seq", "10"], "--truncate_seq", "targetStrings")


def test_truncate_seq_with_both_variables(tmp_path):
    """Per-frame classes are cut with their frames as ever; the transcripts are not, so whoever would read them is refused."""
    nc, _ = transcript_file(tmp_path, with_classes=True)
    base = ["--train_file", nc, "--parallel_sequences", "3", "--truncate_seq", "4"]
    text, (rows,) = dump(base + ["--network", classification_network(tmp_path)])
    assert sum(len(kv["tags"]) for kv in rows) > len(LENS)
    refused(["--train", "true", "--network", ctc_network(tmp_path, len(NAMES) + 1)] + base, "--truncate_seq", "targetStrings")
    refused(["--train", "true", "--dump_fractions", "true", "--dump_labels", "true", "--network", classification_network(tmp_path)] + base,
            "--truncate_seq", "targetStrings")


def classification_network(tmp_path):
    layers = net_desc(P, [("blstm", 8)], len(NAMES))
    weights = random_weights(layers, np.random.RandomState(5), 0.3)
    net = str(tmp_path / "mcc.jsn")
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    return net


def test_another_post_output_layer_on_transcripts_alone_is_refused(tmp_path):
    nc, _ = transcript_file(tmp_path)
    refused(["--train", "true", "--train_file", nc, "--network", classification_network(tmp_path), "--parallel_sequences", "3"],
            "targetStrings", "targetClasses", "multiclass_classification")


def test_ctc_labels_format_needs_a_ctc_net(tmp_path):
    nc, xs, ts = make_file(tmp_path, "plain.nc", LENS, 4, "a")
    refused(["--ff_input_file", nc, "--ff_output_file", str(tmp_path / "out.txt"), "--ff_output_format", "ctc_labels",
             "--network", classification_network(tmp_path), "--parallel_sequences", "3"], "ctc_labels", "ctc")
