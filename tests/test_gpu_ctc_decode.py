"""-m gpu: CTC decoding on the device (include/currennt_hip.h, section CTC decoding; csrc/cn_ctc_decode.hip) against its float-free
model (tests/ctc_decode_reference.py).  Everything is integer work on given fp32 values, so every comparison is for equality.

Kernel level, through cn_dbg_ctc_decode (the layer's launches on posteriors of the test's choice; the hook fills the pad columns
with +inf and checks the pad slots itself): the argmax at every width at which the row-to-wave mapping or the lane a column falls
to changes, the collapse across the workgroup's chunks of 256 frames, the distance with more cells per diagonal than threads.
The hook takes label sequences of any length (a layer's cap, option ctc_max_labels, bounds what cn_layer_set_label_sequences
accepts, not the launches).  Then through a net, the state and argument errors, and the driver."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ctc_decode_reference import decode_fraction, levenshtein, write_transcript_nc
from stride_reference import derived_pattern_types
from test_gpu_ctc import ctc_net, pattern, posteriors, toy_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")


@pytest.fixture(scope="module")
def ctx(pkg, hiplib):
    h = C.c_void_p()
    pkg.binding.check(hiplib.cn_ctx_create(0, pkg.PREC_F32, None, C.byref(h)))
    yield h
    hiplib.cn_ctx_destroy(h)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def dbg_decode(pkg, hiplib, ctx, y, pat, labels=None, accumulate=False):
    """cn_dbg_ctc_decode on y [T][PS][C] float32, pat [T][PS]: (argmax [T][PS], decoded lists, distances [PS])."""
    T, PS, Cn = y.shape
    y = np.ascontiguousarray(y, np.float32)
    pat = np.ascontiguousarray(pat, np.int8)
    amax = np.full((T, PS), -7, np.int32)
    dec = np.full((PS, T), -7, np.int32)
    lens = np.full(PS, -7, np.int32)
    dist = np.full(PS, -7, np.int32)
    if labels is None:
        flat = ll = None
    else:
        ll = np.asarray([len(l) for l in labels], np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in labels] + [np.zeros(1, np.int32)]))
    pkg.binding.check(hiplib.cn_dbg_ctc_decode(ctx, vp(y), vp(pat), T, PS, Cn, None if flat is None else vp(flat), None if ll is None else vp(ll),
                                               1 if accumulate else 0, vp(amax), vp(dec), vp(lens), vp(dist)), ctx)
    assert (lens >= 0).all() and (lens <= T).all()
    return amax, [list(dec[s, :lens[s]]) for s in range(PS)], dist


def check(pkg, hiplib, ctx, y, pat, labels, name):
    """Runs the hook and holds all three results to the model; returns them."""
    amax, decoded, dist = dbg_decode(pkg, hiplib, ctx, y, pat, labels)
    k_ref, dec_ref, dist_ref = decode_fraction(y, pat, labels)
    assert np.array_equal(amax, k_ref), name
    assert decoded == dec_ref, name
    if labels is None:
        assert (dist == -1).all(), name
    else:
        assert np.array_equal(dist, dist_ref), name
    return amax, decoded, dist


def stats(hiplib, ctx, reset):
    e, n = C.c_int64(-1), C.c_int64(-1)
    assert hiplib.cn_ctc_decode_read(ctx, C.byref(e), C.byref(n), 1 if reset else 0) == 0
    return e.value, n.value


# ---- argmax ------------------------------------------------------------------------------------------------------------------

# pairs of columns that receive the same, largest value; a lane holds four consecutive columns and a wave 256 of them, the
# workgroup form (C > 1024) 1024 per round: the same lane, neighbouring lanes, 64 columns apart, two waves, two rounds
TIES = [(1, 2), (3, 4), (0, 1), (5, 69), (63, 64), (100, 164), (300, 900), (7, 1028), (255, 256), (1023, 1024), (2, 1029)]


@pytest.mark.parametrize("Cn", [2, 5, 65, 183, 1030])
def test_argmax(pkg, hiplib, ctx, Cn):
    rng = np.random.RandomState(Cn)
    ties = [(i, j) for i, j in TIES if j < Cn] + ([(Cn - 1 - 64, Cn - 1)] if Cn > 64 else [])
    T, PS = 8 + len(ties), 3
    y = posteriors(rng, T, PS, Cn)
    lens = [T, T - 3, 0]
    pat = pattern(T, PS, lens)
    y[0, :, :] *= 0.5; y[0, :, 0] = 2.0                                # the maximum at index 0
    y[1, :, :] *= 0.5; y[1, :, Cn - 1] = 2.0                           # ... at the blank
    y[2, 0, :] = 0.0                                                   # exact zeros: index 0 (the pad columns hold +inf)
    y[3, 0, :] = 0.25                                                  # every column equal
    for r, (i, j) in enumerate(ties):
        y[4 + r, :, i] = y[4 + r, :, j] = 3.0
    y[T - 2:, 1, 1] = 9.0                                              # behind the second slot's length: ignored
    labels = [list(rng.randint(0, Cn - 1, 4)), list(rng.randint(0, Cn - 1, 2)), []]
    amax, decoded, dist = check(pkg, hiplib, ctx, y, pat, labels, "C%d" % Cn)
    assert amax[0, 0] == 0 and amax[1, 0] == Cn - 1 and amax[2, 0] == 0 and amax[3, 0] == 0
    for r, (i, j) in enumerate(ties):
        assert amax[4 + r, 0] == i and amax[4 + r, 1] == (i if 4 + r < lens[1] else -1)
    assert (amax[:, 2] == -1).all() and (amax[lens[1]:, 1] == -1).all()


# ---- collapse ----------------------------------------------------------------------------------------------------------------

def from_paths(paths, T, Cn, behind=1):
    """One-hot-like posteriors of the given class per frame; the rows behind a path favour the non-blank class `behind`."""
    PS = len(paths)
    y = np.full((T, PS, Cn), 0.1, np.float32)
    y[:, :, behind] = 0.7
    for s, p in enumerate(paths):
        if len(p):
            y[:len(p), s, :] = 0.1
            y[np.arange(len(p)), s, np.asarray(p, np.int64)] = 0.8
    return y, pattern(T, PS, [len(p) for p in paths])


def run_path(rng, cross, Cn):
    """A path of cross + 1 frames in runs of 1-3 frames that ends in a blank and a run of class 2 over frames cross-2 .. cross."""
    p = np.repeat(rng.randint(0, Cn, cross + 1), rng.randint(1, 4, cross + 1))[:cross + 1]
    p[cross - 3] = Cn - 1
    p[cross - 2:] = 2
    return [int(k) for k in p]


def test_collapse_one_frame(pkg, hiplib, ctx):
    y, pat = from_paths([[2], [4], []], 1, 5)
    amax, decoded, dist = check(pkg, hiplib, ctx, y, pat, [[2], [2], [1]], "T1")
    assert decoded == [[2], [], []] and list(dist) == [0, 1, 1]


@pytest.mark.parametrize("T,cross", [(257, 256), (1025, 1024)])
def test_collapse_across_chunks(pkg, hiplib, ctx, T, cross):
    """PS = 5 (three pad slots): a run of one class across frames cross-1 / cross (the last frames of a sequence of T = cross + 1),
    `x _ x` in a sequence whose tail rows favour a non-blank class, all blanks, an empty slot, and a sequence that ends with the
    chunk, at frame cross-1, inside the same run."""
    rng = np.random.RandomState(T)
    Cn = 5
    long = run_path(rng, cross, Cn)
    assert len(long) == T
    paths = [long, [1, 4, 1], [4] * 300 if T > 300 else [4] * 77, [], long[:cross]]
    y, pat = from_paths(paths, T, Cn)
    labels = [list(rng.randint(0, 4, 40)), [1, 1], [], [0, 3], list(rng.randint(0, 4, 90))]
    amax, decoded, dist = check(pkg, hiplib, ctx, y, pat, labels, "T%d" % T)
    assert decoded[1] == [1, 1] and decoded[2] == [] and decoded[3] == [] and list(dist[1:4]) == [0, 0, 2]
    # the run across the chunk boundary is one label: what the frames in front of it decode to, then one 2
    before = decode_fraction(y[:cross - 2, :1], pat[:cross - 2, :1], None)[1][0]
    assert decoded[0] == before + [2] and decoded[4] == before + [2]


def test_collapse_three_slots(pkg, hiplib, ctx):
    """PS = 3 (one pad slot), a sequence that ends in a run, another that starts with blanks."""
    y, pat = from_paths([[0, 0, 4, 0, 1, 1, 4, 3, 3], [4, 4, 2, 2, 2], [3]], 9, 5)
    amax, decoded, dist = check(pkg, hiplib, ctx, y, pat, [[0, 0, 1], [2, 2], []], "PS3")
    assert decoded == [[0, 0, 1, 3], [2], [3]] and list(dist) == [1, 1, 1]


# ---- distance ----------------------------------------------------------------------------------------------------------------

def distinct_path(rng, n, Cn):
    """n frames, no blank, no two neighbours alike: decodes to itself."""
    p = [int(rng.randint(0, Cn - 1))]
    while len(p) < n:
        k = int(rng.randint(0, Cn - 1))
        if k != p[-1]:
            p.append(k)
    return p


def test_distance_edges(pkg, hiplib, ctx):
    rng = np.random.RandomState(3)
    Cn = 6
    seven = distinct_path(rng, 7, Cn)
    paths = [[Cn - 1] * 9, seven, seven, seven + [Cn - 1, Cn - 1], distinct_path(rng, 12, Cn)]
    labels = [list(rng.randint(0, 5, 7)), [], seven, seven[1:], seven[:3] + [4, 4] + seven[3:]]
    y, pat = from_paths(paths, 12, Cn)
    amax, decoded, dist = check(pkg, hiplib, ctx, y, pat, labels, "edges")
    assert list(dist[:4]) == [7, 7, 0, 1] and decoded[0] == [] and decoded[1] == seven


def test_distance_longer_than_a_workgroup(pkg, hiplib, ctx):
    """D = 700 against U = 300 and D = 300 against U = 700: 301 cells per diagonal on 256 threads, 1000 diagonals."""
    rng = np.random.RandomState(4)
    Cn = 6
    a, b = distinct_path(rng, 700, Cn), distinct_path(rng, 300, Cn)
    # related sequences (a distance well below the trivial bounds): the labels are the other slot's path with edits
    la = [k for i, k in enumerate(a) if i % 7 != 3][:300]
    lb = (b + distinct_path(rng, 400, Cn))
    y, pat = from_paths([a, b], 700, Cn)
    amax, decoded, dist = check(pkg, hiplib, ctx, y, pat, [la, lb], "long")
    assert decoded == [a, b] and len(la) == 300 and len(lb) == 700
    assert dist[0] == 400 and 400 <= dist[1] < 700          # (la is a subsequence of a: 400 deletions)


def test_no_labels_still_decodes(pkg, hiplib, ctx):
    rng = np.random.RandomState(5)
    y, pat = posteriors(rng, 40, 3, 7), pattern(40, 3, [40, 22, 0])
    amax, decoded, dist = check(pkg, hiplib, ctx, y, pat, None, "unlabelled")
    assert (dist == -1).all() and len(decoded[0]) > 0 and decoded[2] == []
    with pytest.raises(pkg.binding.CurrenntHipError) as ei:           # nothing to count against
        dbg_decode(pkg, hiplib, ctx, y, pat, None, accumulate=True)
    assert ei.value.code == -4


# ---- sums --------------------------------------------------------------------------------------------------------------------

def test_sums_over_two_fractions(pkg, hiplib, ctx):
    rng = np.random.RandomState(6)
    stats(hiplib, ctx, True)
    assert stats(hiplib, ctx, False) == (0, 0)
    want_e = want_n = 0
    for T, PS, lens in ((30, 3, [30, 17, 4]), (50, 5, [50, 50, 21, 0, 9])):
        y, pat = posteriors(rng, T, PS, 6), pattern(T, PS, lens)
        labels = [list(rng.randint(0, 5, rng.randint(0, 12))) for _ in range(PS)]
        _, _, dist = dbg_decode(pkg, hiplib, ctx, y, pat, labels, accumulate=True)
        ref = decode_fraction(y, pat, labels)[2]
        assert np.array_equal(dist, ref)
        want_e += int(ref.sum()); want_n += sum(len(l) for l in labels)
    assert want_e > 0 and stats(hiplib, ctx, False) == (want_e, want_n)
    assert stats(hiplib, ctx, True) == (want_e, want_n)               # read, then cleared
    assert stats(hiplib, ctx, False) == (0, 0)
    dbg_decode(pkg, hiplib, ctx, y, pat, labels)                      # without `accumulate` the sums stay
    assert stats(hiplib, ctx, True) == (0, 0)


# ---- through a net -----------------------------------------------------------------------------------------------------------

def strided_ctc_net():
    layers = ctc_net()
    layers.insert(1, {"name": "context", "type": "context", "size": 18, "left": 1, "right": 1, "dilation": 1, "stride": 2})
    return layers


@pytest.mark.parametrize("prec", ["PREC_F32", "PREC_BF16"])
@pytest.mark.parametrize("strided", [False, True], ids=["plain", "stride2"])
def test_net_decodes_what_its_posteriors_say(pkg, prec, strided):
    from helpers import random_weights
    rng = np.random.RandomState(8)
    layers = strided_ctc_net() if strided else ctc_net()
    weights = random_weights(layers, rng, 1.5)
    xs, labels = toy_set(rng, 3)
    lens = [len(x) for x in xs]
    frac = pkg.make_fraction(xs, None, 3, labels=labels)
    with pkg.NeuralNetwork(layers, weights, 3, 14, precision=getattr(pkg, prec)) as net:
        net.load_sequences(frac)
        net.compute_forward_pass()
        decoded, dist = net.ctc_decode()
        y = net.outputs()                                               # [T'][PS][5] float32, as the layer saw them
        rate = 2 if strided else 1
        Tn = -(-max(lens) // rate)
        assert y.shape == (Tn, 3, 5) and net.layers[-1].time()[0] == Tn
        pat = derived_pattern_types(lens, max(lens), 3, rate) if strided else frac["patTypes"].reshape(Tn, 3)
        assert [int((pat[:, s] != 0).sum()) for s in range(3)] == [-(-n // rate) for n in lens]
        _, dec_ref, dist_ref = decode_fraction(y, pat, labels)
        print("%s %s: decoded %s, distances %s" % (prec, "stride 2" if strided else "plain", dec_ref, list(dist_ref)))
        assert [list(d) for d in decoded] == dec_ref and np.array_equal(dist, dist_ref)
        # accumulated: the same numbers; a second fraction of two sequences adds to them
        net.ctc_decode_stats()
        net.ctc_decode_accumulate()
        assert net.ctc_decode_stats(reset=False) == (int(dist_ref.sum()), sum(len(l) for l in labels))
        frac2 = pkg.make_fraction(xs[:2], None, 3, labels=labels[:2])
        net.load_sequences(frac2); net.compute_forward_pass(); net.ctc_decode_accumulate()
        d2, dist2 = net.ctc_decode()
        assert len(d2) == 2 and len(dist2) == 2
        assert net.ctc_decode_stats() == (int(dist_ref.sum()) + int(dist2.sum()), sum(len(l) for l in labels) + sum(len(l) for l in labels[:2]))
        # without labels: decoded all the same, no distances
        bare = dict(frac); bare.pop("labels")
        net.load_sequences(bare); net.compute_forward_pass()
        d3, dist3 = net.ctc_decode()
        assert [list(d) for d in d3] == dec_ref and dist3 is None


# ---- state and argument errors -----------------------------------------------------------------------------------------------

def test_state_and_argument_errors(pkg, hiplib):
    from helpers import net_desc, random_weights
    rng = np.random.RandomState(10)
    E = pkg.binding.CurrenntHipError
    layers = ctc_net()
    xs, labels = toy_set(rng, 3)
    frac = pkg.make_fraction(xs, None, 3, labels=labels)
    bare = dict(frac); bare.pop("labels")
    with pkg.NeuralNetwork(layers, random_weights(layers, rng, 0.1), 3, 14) as net:
        for call in (net.ctc_decode, net.ctc_decode_accumulate):       # before a load
            with pytest.raises(E) as ei:
                call()
            assert ei.value.code == -4
        net.load_sequences(frac)
        for call in (net.ctc_decode, net.ctc_decode_accumulate):       # loaded, but no forward pass of this fraction
            with pytest.raises(E) as ei:
                call()
            assert ei.value.code == -4 and "forward pass" in str(ei.value)
        net.compute_forward_pass()
        net.ctc_decode(); net.ctc_decode_accumulate()
        net.load_sequences(frac)                                       # the posteriors belonged to the previous load
        with pytest.raises(E) as ei:
            net.ctc_decode()
        assert ei.value.code == -4
        net.load_sequences(bare); net.compute_forward_pass()
        assert net.ctc_decode()[1] is None
        with pytest.raises(E) as ei:                                   # accumulating needs labels
            net.ctc_decode_accumulate()
        assert ei.value.code == -4 and "no label sequences" in str(ei.value)
        for handle in (net.layers[-2].handle, net.layers[0].handle):   # not a ctc layer
            assert hiplib.cn_ctc_decode(handle, None, None, None) == -1
            assert hiplib.cn_ctc_decode_accumulate(handle) == -1
        assert hiplib.cn_ctc_decode(None, None, None, None) == -1 and hiplib.cn_ctc_decode_read(None, None, None, 0) == -1
        assert hiplib.cn_ctc_decode(net.layers[-1].handle, None, None, None) == 0           # every pointer may be NULL
    mcc = net_desc(6, [("blstm", 8)], 5)
    ts = [np.zeros(len(x), np.int32) for x in xs]
    with pkg.NeuralNetwork(mcc, random_weights(mcc, rng, 0.1), 3, 14) as net:
        net.load_sequences(pkg.make_fraction(xs, ts, 3)); net.compute_forward_pass()
        with pytest.raises(E) as ei:
            net.ctc_decode()
        assert ei.value.code == -1


# ---- driver ------------------------------------------------------------------------------------------------------------------

NAMES = ["a", "b", "c", "d"]


def test_driver_trains_on_transcripts_and_writes_what_it_scores(tmp_path):
    """`--train true` on transcription files (no targetClasses) with --ctc_train_label_errors: both columns show a label error rate,
    two runs print the same table.  Then `--ff_output_format ctc_labels` over the validation file with the network the run
    stored: the lines, scored here against the transcripts, give the validation percentage of the epoch whose weights were kept
    (the last `yes` in the table), to the two printed decimals."""
    from helpers import random_weights
    rng = np.random.RandomState(12)
    files, sets = {}, {}
    for name, n_seq in (("train", 7), ("val", 4)):
        xs, labels = toy_set(rng, n_seq)
        files[name] = str(tmp_path / (name + ".nc"))
        sets[name] = labels
        write_transcript_nc(files[name], xs, labels, NAMES, name[0])
    layers = ctc_net()
    weights = random_weights(layers, rng, 0.1)
    net = str(tmp_path / "ctc.jsn")
    json.dump({"layers": layers, "weights": {k: {a: np.asarray(b).tolist() for a, b in w.items()} for k, w in weights.items()}}, open(net, "w"))
    tables = []
    for run in range(2):
        trained = str(tmp_path / ("trained_%d.jsn" % run))
        args = [BIN, "--train", "true", "--train_file", files["train"], "--val_file", files["val"], "--network", net, "--save_network", trained,
                "--parallel_sequences", "3", "--max_epochs", "3", "--max_epochs_no_best", "10", "--learning_rate", "1e-2", "--momentum", "0.9",
                "--optimizer", "steepest_descent", "--precision", "f32", "--shuffle_fractions", "false", "--shuffle_sequences", "false",
                "--ctc_train_label_errors", "true"]
        out = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.count("from targetStrings") == 2, out.stdout
        rows = [re.sub(r"\|\s*[0-9.]+ \|", "|", l, count=1) for l in out.stdout.splitlines() if re.match(r"^\s+\d+ \|", l)]     # without the duration
        assert len(rows) == 3, out.stdout
        kept = None
        for r in rows:
            cols = [c.strip() for c in r.split("|")]
            for col in cols[1:3]:
                m = re.fullmatch(r"([0-9]+\.[0-9]{2})%\s+([0-9]+\.[0-9]{3})", col)
                assert m and np.isfinite(float(m.group(2))) and 0.0 <= float(m.group(1)), r
            if cols[4] == "yes":
                kept = re.fullmatch(r"([0-9]+\.[0-9]{2})%.*", cols[2]).group(1)
        assert kept is not None, out.stdout
        tables.append(rows)
    assert tables[0] == tables[1]

    written = str(tmp_path / "decoded.txt")
    out = subprocess.run([BIN, "--ff_input_file", files["val"], "--ff_output_file", written, "--ff_output_format", "ctc_labels", "--network", trained,
                          "--parallel_sequences", "3", "--precision", "f32"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = open(written).read().splitlines()
    assert len(lines) == len(sets["val"])
    errors = count = 0
    seen = set()
    for l in lines:
        tag, _, text = l.partition(";")
        idx = int(tag[1:])
        assert tag[0] == "v" and idx not in seen
        seen.add(idx)
        decoded = [NAMES.index(t) for t in text.split()]
        errors += levenshtein(decoded, sets["val"][idx]); count += len(sets["val"][idx])
    rate = float(np.float32(errors) / np.float32(count)) * 100.0        # the driver's arithmetic: a float quotient, printed as a double
    print("validation label error rate: table %s%%, scored from the written lines %.2f%% (%d / %d)" % (kept, rate, errors, count))
    assert "%.2f" % rate == kept
