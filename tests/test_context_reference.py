"""The restated rule of the context layers (tests/context_reference.py) against the input splicing's restatement, against itself
(adjointness, exact) and against autograd; and the ABI of the feature: the header declares it, the built library exports it, the
new layer kind is the last enumerator.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from context_reference import context_backward, context_forward, torch_context
from splice_reference import gather

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# lengths 1 and 2, one longer than (L + R) * D for every case below, an empty slot
LENS = [1, 2, 23, 5, 0]
T, PS, P = 23, 5, 3
MEMBERS = [(0, 0, 1), (2, 1, 1), (0, 2, 1), (3, 0, 1), (1, 2, 3), (0, 3, 3), (2, 0, 3), (3, 3, 3)]


def real_rows():
    return np.arange(T)[:, None] < np.asarray(LENS)[None, :]


# ---- (a) D = 1 is the input splicing's gather ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R", [(0, 0), (2, 1), (0, 3), (4, 0), (5, 5)])
def test_forward_with_dilation_one_is_the_input_gather(L, R):
    x = np.random.RandomState(1).randn(T, PS, P).astype(np.float32)
    want = gather(x, LENS, context=(L, R), frame_skip=1)
    got = context_forward(x, LENS, L, R, 1)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- (b) adjointness, exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R,D", MEMBERS)
def test_backward_is_the_exact_adjoint(L, R, D):
    """Integer-valued float32 arrays: every product and every partial sum is an integer far below 2^24, so both sides are exact."""
    assert D in (1, 3) and max(LENS) > (L + R) * D and {1, 2} <= set(LENS)
    rng = np.random.RandomState(2)
    x = rng.randint(-8, 9, (T, PS, P)).astype(np.float32)
    e = rng.randint(-8, 9, (T, PS, (L + R + 1) * P)).astype(np.float32)
    y, dx = context_forward(x, LENS, L, R, D), context_backward(e, LENS, L, R, D)
    lhs, rhs = np.sum(y.astype(np.float64) * e), np.sum(x.astype(np.float64) * dx)
    assert lhs == rhs and lhs != 0


# ---- (c) the autograd gradient ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R,D", MEMBERS)
def test_backward_is_the_autograd_gradient(L, R, D):
    rng = np.random.RandomState(3)
    x = rng.randn(T, PS, P)
    e = rng.randn(T, PS, (L + R + 1) * P).astype(np.float32)
    h = torch.tensor(x, requires_grad=True)
    y = torch_context(h, LENS, L, R, D)
    assert np.array_equal(y.detach().numpy(), context_forward(x, LENS, L, R, D))           # (the differentiable form is the rule)
    (y * torch.tensor(e.astype(np.float64))).sum().backward()
    want = h.grad.numpy()
    # the same gradient of |e|: what the terms of each sum add up to in magnitude.  A sum of m fp32 terms is off by at most
    # (m - 1) * 2^-24 of that; m <= B * (max(L, R) * D + 1)
    g = torch.tensor(x, requires_grad=True)
    (torch_context(g, LENS, L, R, D) * torch.tensor(np.abs(e).astype(np.float64))).sum().backward()
    m = (L + R + 1) * (max(L, R) * D + 1)
    got = context_backward(e, LENS, L, R, D)
    assert got.dtype == np.float32
    assert np.all(np.abs(got - want) <= m * 2.0 ** -24 * g.grad.numpy()), float(np.abs(got - want).max())
    assert np.abs(want).max() > 1


# ---- (d) dummy rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R,D", MEMBERS)
def test_dummy_rows_are_zero_and_never_read(L, R, D):
    rng = np.random.RandomState(4)
    real = real_rows()
    x = rng.randn(T, PS, P).astype(np.float32) + 3
    e = rng.randn(T, PS, (L + R + 1) * P).astype(np.float32) + 3
    y, dx = context_forward(x, LENS, L, R, D), context_backward(e, LENS, L, R, D)
    assert (~real).any() and np.all(y[~real] == 0) and np.all(dx[~real] == 0)
    assert np.all(y[real] != 0) and np.all(dx[real] != 0)
    # what the arrays hold on dummy rows does not matter
    x2, e2 = x.copy(), e.copy()
    x2[~real], e2[~real] = 99, -99
    assert np.array_equal(context_forward(x2, LENS, L, R, D), y) and np.array_equal(context_backward(e2, LENS, L, R, D), dx)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def header_text():
    src = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


# the values every cn_layer_kind had before the context layer: they are part of the ABI (network tools, the Python binding)
KINDS_BEFORE = ["CN_LAYER_INPUT", "CN_LAYER_LSTM", "CN_LAYER_BLSTM", "CN_LAYER_FF_TANH", "CN_LAYER_FF_LOGISTIC", "CN_LAYER_FF_IDENTITY",
                "CN_LAYER_SOFTMAX", "CN_LAYER_SSE", "CN_LAYER_MULTICLASS_CLASSIFICATION", "CN_LAYER_WEIGHTEDSSE", "CN_LAYER_SSE_MASK",
                "CN_LAYER_CE", "CN_LAYER_RMSE", "CN_LAYER_BINARY_CLASSIFICATION", "CN_LAYER_CTC"]


def test_abi_declares_and_exports_the_context_layer(pkg):
    """The library builds without a GPU, exports the two entry points the header declares, and CN_LAYER_CONTEXT is the last
    enumerator behind the unchanged earlier ones."""
    src = header_text()
    assert re.search(r"\bint\s+cn_layer_create_context\s*\(\s*cn_ctx\s*\*\s*ctx\s*,\s*cn_layer\s*\*\s*preceding\s*,\s*int\s+left\s*,\s*int\s+right\s*,"
                     r"\s*int\s+dilation\s*,\s*cn_layer\s*\*\*\s*out\s*\)\s*;", src)
    assert re.search(r"\bint\s+cn_layer_context\s*\(\s*const\s+cn_layer\s*\*\s*layer\s*,\s*int\s*\*\s*left\s*,\s*int\s*\*\s*right\s*,\s*int\s*\*\s*dilation\s*\)\s*;", src)
    body = re.search(r"typedef\s+enum\s+cn_layer_kind\s*\{(.*?)\}\s*cn_layer_kind\s*;", src, flags=re.S).group(1)
    names = [n.strip() for n in body.split(",") if n.strip()]
    assert names[0] == "CN_LAYER_INPUT = 0" and [n.split("=")[0].strip() for n in names] == KINDS_BEFORE + ["CN_LAYER_CONTEXT"]
    assert all("=" not in n for n in names[1:])                              # (consecutive values: the position is the value)
    assert pkg.KIND_CONTEXT == len(KINDS_BEFORE) and sorted(pkg.LAYER_KINDS.values()) == list(range(len(KINDS_BEFORE)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lstm-rnn_amd", "csrc"), "-j4"])
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], universal_newlines=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"cn_layer_create_context", "cn_layer_context"} <= exported
