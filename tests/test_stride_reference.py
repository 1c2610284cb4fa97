"""CPU: the restated rule of the strided context layers (tests/stride_reference.py) against the plain context layers' at stride 1,
against torch autograd, and against itself where two strides compose; the ABI symbols; the driver's refusals; and the conditions
that tests/test_gpu_stride.py states for its test nets."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from context_reference import context_backward, context_forward
from stride_reference import (CASES, FIRST, LAST, NONE, NORMAL, axes_of, ceil_div, derived_pattern_types, derived_targets, stride_net_desc,
                              strided_backward, strided_forward, strided_lengths, torch_strided, unread_frames)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [13, 6, 1, 2, 9]
MEMBERS = [(0, 0, 1), (1, 1, 1), (2, 1, 3), (0, 2, 2), (3, 0, 1)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_input(rng, T, PS, P):
    return (rng.randn(T, PS, P) + 0.25).astype(np.float32)


@pytest.mark.parametrize("L,R,D", MEMBERS)
def test_stride_one_is_the_context_layer(L, R, D):
    rng = np.random.RandomState(1)
    T, PS, P = max(LENS), len(LENS) + 1, 3
    x = random_input(rng, T, PS, P)
    assert np.array_equal(bits(strided_forward(x, LENS, L, R, D, 1)), bits(context_forward(x, LENS, L, R, D)))
    e = random_input(rng, T, PS, (L + R + 1) * P)
    assert np.array_equal(bits(strided_backward(e, LENS, T, L, R, D, 1)), bits(context_backward(e, LENS, L, R, D)))


@pytest.mark.parametrize("S", [2, 3, 8])
@pytest.mark.parametrize("L,R,D", MEMBERS)
def test_fold_is_the_gradient_of_the_gather(L, R, D, S):
    """The fold against torch autograd of the gather, in float64 on float32 values with few terms: equal up to the order of sums."""
    rng = np.random.RandomState(2)
    T, PS, P = max(LENS), len(LENS) + 1, 3
    x = random_input(rng, T, PS, P)
    h = torch.tensor(x.astype(np.float64), requires_grad=True)
    out = torch_strided(h, LENS, L, R, D, S)
    want_fwd = strided_forward(x, LENS, L, R, D, S)
    assert out.shape == want_fwd.shape and np.array_equal(out.detach().numpy().astype(np.float32), want_fwd)
    e = random_input(rng, *want_fwd.shape)
    (out * torch.tensor(e.astype(np.float64))).sum().backward()
    got = strided_backward(e, LENS, T, L, R, D, S)
    # the rows of e behind n_s are non-zero and must not be read
    assert np.abs(got.astype(np.float64) - h.grad.numpy()).max() < 1e-5
    # frames nobody reads are exactly +0.0 and the gradient agrees
    unread = unread_frames(LENS, T, PS, L, R, D, S)
    assert np.all(bits(got[unread]) == 0) and np.all(h.grad.numpy()[unread] == 0)
    if L == 0 and R == 0 and S == 2:
        assert unread[1::2][:, 0][:6].all()


def test_two_strides_compose():
    rng = np.random.RandomState(3)
    T, PS, P = max(LENS), len(LENS), 2
    x = random_input(rng, T, PS, P)
    for S1, S2 in ((2, 3), (3, 2), (2, 2), (8, 2)):
        l1 = strided_lengths(LENS, S1)
        assert strided_lengths(l1, S2) == strided_lengths(LENS, S1 * S2)
        assert ceil_div(ceil_div(T, S1), S2) == ceil_div(T, S1 * S2)
        # L = R = 0: frame j of the second axis is parent frame S1 * S2 * j
        two = strided_forward(strided_forward(x, LENS, 0, 0, 1, S1), l1, 0, 0, 1, S2)
        one = strided_forward(x, LENS, 0, 0, 1, S1 * S2)
        assert np.array_equal(bits(two), bits(one))
        tc = rng.randint(0, 5, (T, PS)).astype(np.int32)
        assert np.array_equal(derived_targets(derived_targets(tc, LENS, S1), l1, S2), derived_targets(tc, LENS, S1 * S2))
        p2 = derived_pattern_types(l1, ceil_div(T, S1), PS, S2)
        assert np.array_equal(p2, derived_pattern_types(LENS, T, PS, S1 * S2))


def test_derived_axis():
    pat = derived_pattern_types([13, 6, 1], 13, 4, 2)
    assert pat.shape == (7, 4)
    assert list(pat[:, 0]) == [FIRST] + [NORMAL] * 5 + [LAST]
    assert list(pat[:, 1]) == [FIRST, NORMAL, LAST] + [NONE] * 4
    assert list(pat[:, 2]) == [FIRST] + [NONE] * 6 and np.all(pat[:, 3] == NONE)
    tc = np.arange(13 * 3, dtype=np.int32).reshape(13, 3)
    got = derived_targets(tc, [13, 6, 1], 2)
    assert list(got[:, 1]) == [1, 7, 13, -1, -1, -1, -1] and got[0, 2] == 2 and np.all(got[1:, 2] == -1)
    tg = np.ones((13, 3, 2), np.float32)
    got = derived_targets(tg, [13, 6, 1], 2)
    assert got.dtype == np.float32 and np.all(got[:3, 1] == 1) and np.all(got[3:, 1] == 0)


def test_the_test_nets_meet_their_conditions():
    P, hidden, C, PS, lens, *_ = CASES["small"]
    layers = stride_net_desc(P, hidden, C)
    ax = axes_of(layers, lens, max(lens))
    assert PS == 3 and lens == [13, 6, 1]
    assert ax["context_1"][1] == [7, 3, 1] and ax["context_3"][1] == [3, 1, 1] and ax["output"][2] == 6
    assert any(n % 2 == 0 for n in lens) and any(n % 2 for n in lens) and 1 in lens                      # a multiple of S, one that is not, one frame
    assert all(min(ax[d["name"]][1]) < ax[d["name"]][0] for d in layers)                                # dummy rows in every axis
    assert [t for t, _ in hidden] == ["lstm", "context", "blstm", "context", "feedforward_tanh", "lstm"] and hidden[2][1] // 2 == 5
    P, hidden, C, PS, lens, *_ = CASES["wide"]
    layers = stride_net_desc(P, hidden, C)
    assert PS == 8 and lens == [17 - (i % 5) for i in range(8)]
    T = max(lens)
    for d in layers:
        if d["type"] == "context":
            Tp, lp, _ = axes_of(layers, lens, T)[layers[layers.index(d) - 1]["name"]]
            assert unread_frames(lp, Tp, PS, d["left"], d["right"], d["dilation"], d["stride"]).any(), d["name"]     # both folds leave frames unread
            assert layers[layers.index(d) - 1]["size"] % 8 == 0                                                          # the 16-byte paths
    P, hidden, C, PS, lens, *_ = CASES["from_input"]
    assert hidden[0] == ("context", (2, 3, 1, 2)) and lens == [7, 5, 2]
    P, hidden, C, PS, lens, *_ = CASES["features"]
    assert hidden[1][0] == "context" and hidden[2] == ("feedforward_tanh", 3 * hidden[0][1])           # a residual follower of size B * P


def test_abi_symbols():
    header = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    lib = os.path.join(ROOT, "lstm-rnn_amd", "libcurrennt_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for name in ("cn_layer_create_context_strided", "cn_layer_context_stride", "cn_layer_time"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r" T %s$" % name, syms, re.M), name
    assert "Strided context layers" in header
    assert header.index("Strided context layers") > header.index("---- Context layers")


def driver_binary():
    exe = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build()
    return exe


@pytest.mark.parametrize("value", [0, 9, 2.5, True])
def test_driver_refuses_a_bad_stride(tmp_path, value):
    """The refusal comes from parsing the network file, before any device is touched, and names the layer."""
    net = {"layers": [{"name": "input", "type": "input", "size": 39},
                      {"name": "lstm_1", "type": "lstm", "size": 8, "bias": 1.0},
                      {"name": "pyramid_2", "type": "context", "size": 16, "left": 0, "right": 1, "stride": value},
                      {"name": "output", "type": "softmax", "size": 51, "bias": 1.0},
                      {"name": "postoutput", "type": "multiclass_classification", "size": 51}]}
    path = tmp_path / "network.jsn"
    path.write_text(json.dumps(net))
    nc = os.path.join(ROOT, "tests", "golden", "val_1_speaker.nc")
    r = subprocess.run([driver_binary(), "--network", str(path), "--train", "true", "--train_file", nc, "--max_epochs", "1",
                        "--parallel_sequences", "3", "--train_fraction", "0.01", "--save_network", str(tmp_path / "out.jsn")],
                       capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode != 0, out
    assert "Invalid value 'stride' in layer 'pyramid_2'" in out and "1..8" in out, out
