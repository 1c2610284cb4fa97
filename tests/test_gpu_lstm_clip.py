"""-m gpu: every backward recurrent kernel inside the cell's delta clip.

Each case runs the forward pass of 9 -> lstm 32 -> the layer under test -> softmax 7, writes LARGE errors into the layer under
test (Layer.write_output_errors; recipe and conditions: tests/test_lstm_clip_reference.py), runs that layer's backward pass alone
(Layer.backward) and compares the four stored gate deltas per direction, the four sections of the weight gradient (each against
its own largest entry) and the errors handed to the preceding layer.  The kernel that ran is asserted by name.

In every case: max |delta| <= 1 on all rows; exactly sign(u64) on the forced set F (u64: the unclipped delta of the float64
restatement; |u64| >= 1.01, bf16: 1.25); deltas of dummy frames exactly 0.
f32:    distance to the double oracle <= K * D_ref per quantity (D_ref: the fp32 oracle's own distance, K = 8.46), and the 2e-4
        of test_gpu_parity.check_network against the fp32 oracle.
bf16x3: distance to the double oracle <= K * (D_model + D_ref), D_model: the split-operand model's distance.
bf16:   against the oracle's bf16 operand model GRAD_TOL_BF16_PINNED on the whole gradient, ERR_TOL_BF16_PINNED on the propagated
        errors, the deltas off F within 2^-7 (one bf16 step); the gradient sections <= K * (D_model + D_ref) from the double oracle.
        Those bounds are bf16-wide: a kernel that built the cell state error from the clipped output gate delta, or carried
        unclipped deltas, moves a stored delta by 0.012 .. 0.39, in most cases less than 10 of those bounds.  So every stored delta is also REPLAYED
        (lstm_clip_reference.replay_stored_deltas): the rule, in float64, on the kernel's own forward internals and its own stored
        deltas of the step before, with a running bound on the kernel's fp32 rounding; a stored delta must be one bf16 rounding
        (2^-8 relative) of that value.  The wrong rules miss this by 19 .. 370 bounds (tests/test_lstm_clip_reference.py).
Twin pairs (a hand-written or generated loop and the compiled kernel of its cut, in one test): all four deltas on real frames
bit-identical, gradients and propagated errors at 1e-6 -- the assertions of test_gpu_parity.test_hand_written_*, with the clip
engaged.

None of the bounds comes from the kernels.  MEASURED on one MI355X (table: DESIGN.md section 3): largest D_hip / bound 0.24 (f32), 0.19
(bf16x3), 0.13 (bf16 gradient sections); bf16 against its model: deltas off F 1.9e-3 .. 3.6e-3 (2^-7), whole gradient <= 9.7e-5 (2e-3),
propagated errors <= 4.3e-4 (5e-3); replay 0.985 .. 0.994 of its bound on every bf16 kernel (a round-to-nearest half step: the bound
is met, the fp32 terms are invisible).  Before lstm_bwd_kernel's f32 form added the injected error behind its chained product
instead of seeding the chain with it, <1,128,1,1> sat at 0.84 and <1,128,1,2> at 1.93 of the bound on the net-input deltas.
"""
import contextlib
import os

import numpy as np
import pytest

from lstm_clip_reference import GATES
from test_gpu_parity import rel_err
from test_lstm_clip_reference import (DELTA_TOL_BF16, ERR_TOL_BF16_PINNED, GPU_CASES, GRAD_TOL_BF16_PINNED, GRAD_TOL_F32, PS, distances,
                                      fmt, references, replay)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def environment(env):
    """CN_* switches that select a kernel: a context reads them when it is created."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_hip(pkg, inp, mode, env, internals=False):
    """Forward pass, injected errors, the layer's backward pass alone -> (backward kernel of the layer under test, quantities in
    the layout of test_lstm_clip_reference.oracle_run)."""
    precision = {"f32": pkg.PREC_F32, "bf16": pkg.PREC_BF16, "bf16x3": pkg.PREC_BF16X3}[mode]
    T = inp["T"]
    with environment(env):
        net = pkg.NeuralNetwork(inp["layers"], inp["weights"], PS, T, precision=precision)
    with net:
        net.load_sequences(inp["frac"]); net.compute_forward_pass()
        lay = net.layer(inp["name"])
        lay.write_output_errors(inp["errors"])
        lay.backward()
        kernel = net.lib.cn_layer_recurrent_kernel(lay.handle, 1).decode()
        got = {"deltas": [{g: lay.internal(g + "Deltas", d).astype(np.float64) for g in GATES} for d in range(lay.dirs)],
               "grad_flat": lay.weight_updates().astype(np.float64),
               "prev_errors": lay.prev.output_errors().astype(np.float64)}
        if internals:
            got["internals"] = [{n: lay.internal(n, d).astype(np.float64) for n in ("niActs", "igActs", "fgActs", "ogActs", "cellStates")}
                                for d in range(lay.dirs)]
    return kernel, got


def check(case, got, label):
    """The assertions on one kernel's results; prints the figures first."""
    inp, mode, r64, model = case["inp"], case["mode"], case["R64"], case["M"]
    real = inp["real"]
    D_hip = distances(got, r64, inp)
    bound = case["bound"]
    print("\n[%s] D_ref   %s" % (label, fmt(case["D_ref"])))
    print("[%s] D_model %s" % (label, fmt(case["D_model"])))
    print("[%s] D_hip   %s" % (label, fmt(D_hip)))
    vs_model = distances(got, model, inp)
    whole = {"grad": rel_err(got["grad_flat"], model["grad_flat"]), "err": rel_err(got["prev_errors"][real], model["prev_errors"][real])}
    print("[%s] against the model: %s whole %s" % (label, fmt(vs_model), fmt(whole)))
    ratio = {q: D_hip[q] / bound[q] for q in D_hip if not (mode == "bf16" and (q.startswith("delta/") or q == "err"))}
    print("[%s] D_hip / bound %s" % (label, fmt(ratio)))
    assert all(np.all(np.isfinite(v)) for v in (got["grad_flat"], got["prev_errors"]))
    off_f = {}
    for d in range(inp["dirs"]):
        for g in GATES:
            v, F, u = got["deltas"][d][g], case["F"][d][g], case["U64"][d][g]
            assert np.all(np.isfinite(v)) and np.abs(v).max() <= 1.0, (label, d, g, float(np.abs(v).max()))
            assert np.abs(v[real]).max() == 1.0, (label, d, g)                  # (the clip is engaged)
            wrong = v[F] != np.sign(u[F])
            assert not wrong.any(), (label, d, g, "forced set", int(wrong.sum()), int(F.sum()))
            assert np.all(v[~real] == 0), (label, d, g, "frames without a pattern")
            if mode == "bf16":
                free = real[:, :, None] & ~F
                off_f["%d/%s" % (d, g)] = float(np.abs(v[free] - model["deltas"][d][g][free]).max())
    if mode == "bf16":
        print("[%s] deltas off F against the model %s" % (label, fmt(off_f)))
        assert all(x <= DELTA_TOL_BF16 for x in off_f.values()), (label, fmt(off_f))
        assert whole["grad"] < GRAD_TOL_BF16_PINNED, (label, whole)
        assert whole["err"] < ERR_TOL_BF16_PINNED, (label, whole)
        replayed = replay(inp, got["internals"], got["deltas"])
        print("[%s] replay: |stored - rule| / bound %s" % (label, fmt(replayed)))
        assert replayed["dummy"] == 0 and all(x <= 1.0 for x in replayed.values()), (label, fmt(replayed))
    if mode == "f32":
        assert whole["grad"] < GRAD_TOL_F32 and whole["err"] < GRAD_TOL_F32, (label, whole)
    bad = {q: (D_hip[q], bound[q]) for q in ratio if not D_hip[q] <= bound[q]}
    assert not bad, (label, bad)
    return D_hip


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_backward_kernel_inside_the_delta_clip(pkg, orc, name):
    spec = GPU_CASES[name]
    kind, size, T, mode, env, kernel = spec[:6]
    case = references(pkg, orc, kind, size, T, mode)
    ran, got = run_hip(pkg, case["inp"], mode, env, internals=mode == "bf16")
    assert ran == kernel, ran
    check(case, got, "%s %s" % (name, ran))
    if len(spec) > 6:
        twin_env, twin_kernel = spec[6:]
        ran2, twin = run_hip(pkg, case["inp"], mode, twin_env, internals=mode == "bf16")
        assert ran2 == twin_kernel, ran2
        check(case, twin, "%s %s" % (name, ran2))
        real = case["inp"]["real"]
        for d in range(case["inp"]["dirs"]):
            for g in GATES:
                a, b = got["deltas"][d][g][real], twin["deltas"][d][g][real]
                assert np.array_equal(a, b), (name, d, g, int((a != b).sum()), float(np.abs(a - b).max()))
        assert rel_err(got["grad_flat"], twin["grad_flat"]) < 1e-6, name
        assert rel_err(got["prev_errors"][real], twin["prev_errors"][real]) < 1e-6, name
