"""The restatement the GPU is held to (tests/residual_reference.py), checked on the CPU: the fp64 autograd stack without a marked
layer is the double oracle; with a marked layer the error handed to the predecessor is the branch's term plus the layer's own
dL/d out, and it is the derivative (finite differences); the sum rule rounds once, ties to even."""
import numpy as np
import torch

from helpers import net_desc, oracle_reference, random_sequences, random_weights, real_mask
from residual_reference import autograd_residual, ff_delta, flat_weights, residual_sum

# the smallest net of tests/test_gpu_residual.py
P, C, PS, LENS = 7, 5, 3, [9, 6, 4]
HIDDEN = [("lstm", 10), ("blstm", 10), ("feedforward_tanh", 10), ("lstm", 10)]
MARKED = ("blstm_1", "feedforward_tanh_2", "lstm_3")


def small_case(pkg):
    rng = np.random.RandomState(41)
    layers = net_desc(P, HIDDEN, C)
    weights = random_weights(layers, rng, 0.3)
    xs, ts = random_sequences(rng, LENS, P, C=C)
    return layers, weights, pkg.make_fraction(xs, ts, PS)


def test_unmarked_stack_is_the_double_oracle(pkg, orc):
    """No layer marked: the stack (now with feed-forward hidden layers) against oracle_reference(orc.real64()), to the 1e-10 that
    test_double_oracle_equals_fp64_autograd_to_rounding_noise allows two fp64 statements of the same equations."""
    layers, weights, frac = small_case(pkg)
    want = oracle_reference(orc.real64(), layers, weights, frac, PS)
    branches = {}
    loss, post, grads, errs = autograd_residual(layers, flat_weights(weights), frac, LENS, (), branches=branches)
    # (the oracle, like the reference, overwrites a feed-forward layer's outputErrors with act'(y) * e in its backward pass)
    errs["feedforward_tanh_2"] = ff_delta("feedforward_tanh", branches["feedforward_tanh_2"], errs["feedforward_tanh_2"])
    worst = {"loss": abs(loss - want["error"]) / max(1.0, abs(loss)), "post": float(np.abs(post - want["post"]).max())}
    for name, g in grads.items():
        worst["grad/" + name] = float(np.abs(g - want["grad/" + name]).max() / np.abs(g).max())
    for name, e in errs.items():
        worst["err/" + name] = float(np.abs(e - want["err/" + name]).max() / np.abs(e).max())
    print({k: float("%.2g" % v) for k, v in worst.items()})
    assert len(errs) == 4 and all(v <= 1e-10 for v in worst.values()), worst


def test_marked_layer_hands_back_branch_term_plus_its_own_error(pkg):
    layers, weights, frac = small_case(pkg)
    w64 = flat_weights(weights)
    real = real_mask(frac)
    T = frac["T"]
    seen = {}

    def record(name, h):
        seen[name] = h.detach().clone()
        return h
    loss, _, _, errs = autograd_residual(layers, w64, frac, LENS, MARKED, hook=record)
    realm = torch.tensor(real.reshape(T, PS, 1).astype(np.float64))
    names = [d["name"] for d in layers[1:-2]]
    for l in MARKED:
        p = names[names.index(l) - 1]
        # (1) the same net with l unmarked, its output shifted by the CONSTANT skip term of the marked run: every activation is the
        # marked run's, but no gradient flows through the skip path -- "the unmarked value recomputed on the summed activations"
        skip = seen[p] * realm
        _, _, _, branch_only = autograd_residual(layers, w64, frac, LENS, tuple(m for m in MARKED if m != l),
                                                 hook=lambda name, h: h + skip if name == l else h)
        assert np.abs(branch_only[l] - errs[l]).max() <= 1e-12 * np.abs(errs[l]).max()
        want = branch_only[p] + errs[l]
        assert np.abs(errs[p] - want).max() <= 1e-12 * np.abs(want).max(), (l, float(np.abs(errs[p] - want).max()))
        assert np.abs(errs[l]).max() > 1e-3 and np.abs(branch_only[p]).max() > 1e-4          # (both terms are there)
        # (2) ... and the sum is the derivative: central differences of the loss along random directions of p's output on real
        # frames.  eps = 1e-6 in fp64: truncation ~ eps^2, rounding ~ 1e-16 * loss / eps ~ 1e-9; bound 1e-6 of the larger of 1 and
        # the directional derivative.
        rng = np.random.RandomState(7)
        for _ in range(3):
            V = torch.tensor(rng.randn(T, PS, 10)) * realm
            eps = 1e-6
            lp = autograd_residual(layers, w64, frac, LENS, MARKED, hook=lambda name, h: h + eps * V if name == p else h)[0]
            lm = autograd_residual(layers, w64, frac, LENS, MARKED, hook=lambda name, h: h - eps * V if name == p else h)[0]
            fd = (lp - lm) / (2 * eps)
            an = float((errs[p] * V.numpy().reshape(T * PS, -1)[real]).sum())
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (l, fd, an)
    assert loss > 0


def test_sum_rule_rounds_once_ties_to_even():
    u = 2.0 ** -7                                   # the spacing of bf16 in [1, 2)
    b = np.array([[1.0, 1.0 + u, 1.0, 1.0, -1.0, -(1.0 + u), 0.5, 3.0]], np.float32)
    x = np.array([[u / 2, u / 2, u / 2 + u / 256, u / 4, -u / 2, -u / 2, 0.25, 0.0]], np.float32)
    # 1 + u/2 is a tie: the even neighbour is 1;  (1 + u) + u/2 is a tie: the even neighbour is 1 + 2u;  just above a tie rounds
    # up, a quarter rounds down;  the negative mirror images;  an exact sum stays;  x = 0 leaves the branch
    want = np.array([[1.0, 1.0 + 2 * u, 1.0 + u, 1.0, -1.0, -(1.0 + 2 * u), 0.75, 3.0]], np.float32)
    got = residual_sum(b, x, np.array([True]), bf16=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    # fp32 operands: the fp32 sum, unrounded
    got32 = residual_sum(b, x, np.array([True]), bf16=False)
    assert np.array_equal(got32, (b + x).astype(np.float32)) and not np.array_equal(got32, want)
    # a row that is no real frame is the branch, bit for bit
    both = residual_sum(np.vstack([b, b]), np.vstack([x, x]), np.array([True, False]), bf16=True)
    assert np.array_equal(both[0], want[0]) and np.array_equal(both[1].view(np.uint32), b[0].view(np.uint32))
