"""Host side of the CTC post output layer, no GPU: the label sequences data_sets::DataSet derives from the per-frame target
classes (`--dump_fractions true --dump_labels true`) against a Python collapse of the same targets; the driver's check of a ctc
network's output size against the data; the "ctc" layer type in the binding and the header."""
import json
import os
import re
import subprocess

import numpy as np

from helpers import random_weights
from test_host_dataset import BIN, dump, write_nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, LABELS = 6, 4


def collapse(t):
    """a a a b b a -> a b a"""
    t = np.asarray(t)
    return [int(k) for i, k in enumerate(t) if i == 0 or k != t[i - 1]]


def run_file(tmp_path, lens, seed=3):
    rng = np.random.RandomState(seed)
    xs = [rng.randn(n, P).astype(np.float32) for n in lens]
    ts = [np.repeat(rng.randint(0, LABELS, n), rng.randint(1, 5, n))[:n].astype(np.int32) for n in lens]     # runs of 1-4 frames
    path = str(tmp_path / "train.nc")
    write_nc(path, xs, ts, LABELS, "a")
    return path, xs, ts


def ctc_network(tmp_path, units):
    layers = [{"name": "input", "type": "input", "size": P},
              {"name": "blstm", "type": "blstm", "size": 8, "bias": 1.0},
              {"name": "output", "type": "softmax", "size": units, "bias": 1.0},
              {"name": "postoutput", "type": "ctc", "size": units}]
    weights = random_weights(layers, np.random.RandomState(5), 0.3)
    net = str(tmp_path / ("ctc_%d.jsn" % units))
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    return net


def test_dumped_label_sequences_are_the_collapsed_targets(tmp_path):
    lens = (14, 5, 9, 1, 11, 7, 12)
    nc, xs, ts = run_file(tmp_path, lens)
    net = ctc_network(tmp_path, LABELS + 1)
    PS = 3
    base = ["--train_file", nc, "--network", net, "--parallel_sequences", str(PS)]
    text, (rows,) = dump(base + ["--dump_labels", "true"])
    by_tag = {"a%03d" % i: collapse(t) for i, t in enumerate(ts)}
    assert any(len(l) < len(t) for l, t in zip(by_tag.values(), ts)) and any(l.count(l[0]) > 1 for l in by_tag.values())
    assert len(rows) == (len(lens) + PS - 1) // PS
    for kv in rows:
        seqs = [by_tag[t] for t in kv["tags"]]
        assert int(kv["label_seqs"]) == len(seqs)
        assert int(kv["labels_total"]) == sum(len(l) for l in seqs)
        assert int(kv["sum_labels"]) == sum(sum(l) for l in seqs)
    # rows are unchanged without the flag
    plain, _ = dump(base)
    stripped = [re.sub(r" label_seqs=\d+ labels_total=\d+ sum_labels=\d+$", "", l) for l in text.splitlines() if l.startswith("FRACTION")]
    assert stripped == [l for l in plain.splitlines() if l.startswith("FRACTION")] and "label_seqs" not in plain


def test_driver_rejects_a_ctc_net_without_the_blank_unit(tmp_path):
    nc, xs, ts = run_file(tmp_path, (9, 6, 7))
    for units in (LABELS, LABELS + 2):
        out = subprocess.run([BIN, "--train", "true", "--train_file", nc, "--network", ctc_network(tmp_path, units),
                              "--parallel_sequences", "3", "--max_epochs", "1"], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0
        assert "Number of classes mismatch" in out.stdout + out.stderr, out.stdout + out.stderr


def test_ctc_parses(pkg, tmp_path):
    """The type string in the binding, at the END of cn_layer_kind in the header; the driver takes a well-formed ctc network past
    its checks (what follows needs a device)."""
    header = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    body = header[header.index("typedef enum cn_layer_kind {"):header.index("} cn_layer_kind;")]
    names = re.findall(r"^\s*(CN_LAYER_[A-Z_]+)\b", body, re.M)
    assert names[-1] == "CN_LAYER_CTC" and pkg.LAYER_KINDS["ctc"] == len(names) - 1 == max(pkg.LAYER_KINDS.values())
    assert pkg.LAYER_KINDS["binary_classification"] == 13 and pkg.LAYER_KINDS["multiclass_classification"] == 8
    frac = pkg.make_fraction([np.zeros((4, P), np.float32)], None, 2, labels=[[1, 1, 0]])
    assert [list(l) for l in frac["labels"]] == [[1, 1, 0]] and (frac["targetClasses"] == -1).all()
    nc, xs, ts = run_file(tmp_path, (9, 6, 7))
    out = subprocess.run([BIN, "--train", "true", "--train_file", nc, "--network", ctc_network(tmp_path, LABELS + 1),
                          "--parallel_sequences", "3", "--max_epochs", "1"], capture_output=True, text=True, timeout=120)
    text = out.stdout + out.stderr
    assert "Unknown layer type" not in text and "mismatch" not in text, text
