"""Adam without a GPU: the numpy restatement the GPU tests compare against bit for bit (tests/adam_reference.py) is Adam
-- it agrees with torch.optim.Adam in float64 --, the new symbols are declared, and the driver knows the option."""
import os
import re
import subprocess

import numpy as np

from adam_reference import adam_scalars, adam_step, test_gradients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
NEW_SYMBOLS = ("cn_adam_update", "cn_adam_update_all", "cn_ctx_arm_adam")


def test_restatement_is_torch_adam_in_float64():
    """12 steps on 5000 weights, gradient magnitudes 1e-6 ... 1 with exact zeros: the restatement (bias correction folded into
    alpha_t and eps_t) run in float64 against torch.optim.Adam in float64.  Bound: 1e-10 of max |w|, DESIGN section 3's
    bound for its fp64 pins; the two differ by rounding only (5.6e-17 measured)."""
    import torch
    rng = np.random.RandomState(11)
    n, steps, lr, b1, b2, eps = 5000, 12, 1e-3, 0.9, 0.999, 1e-8
    w0 = rng.uniform(-0.3, 0.3, n)
    grads = [test_gradients(rng, n).astype(np.float64) for _ in range(steps)]
    assert any((g == 0).any() for g in grads) and min(np.abs(g[g != 0]).min() for g in grads) < 1e-5
    p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    w, m, v = w0.copy(), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        w, m, v = adam_step(w, g, m, v, lr, b1, b2, eps, t, dtype=np.float64)
    ref = p.detach().numpy()
    d = float(np.abs(w - ref).max())
    print("restatement vs torch.optim.Adam, float64: %.3g (max |w| %.3g)" % (d, np.abs(ref).max()))
    assert d <= 1e-10 * np.abs(ref).max()
    assert np.abs(ref - w0).max() > 1e-3              # the weights moved


def test_float32_restatement_is_close_to_float64_and_rounds_scalars_once():
    rng = np.random.RandomState(12)
    n = 2000
    w32 = w64 = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    m32 = v32 = np.zeros(n, np.float32)
    m64 = v64 = np.zeros(n)
    for t in range(1, 13):
        g = test_gradients(rng, n)
        w32, m32, v32 = adam_step(w32, g, m32, v32, 1e-3, step=t)
        w64, m64, v64 = adam_step(w64, g, m64, v64, 1e-3, step=t, dtype=np.float64)
    assert w32.dtype == np.float32 and np.abs(w32 - w64).max() < 1e-6
    s = adam_scalars(1e-3, 0.9, 0.999, 1e-8, 1)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert s["omb1"] == np.float32(1.0 - b1) and s["omb2"] == np.float32(1.0 - b2)
    assert s["alpha_t"] == np.float32(float(np.float32(1e-3)) * np.sqrt(1.0 - b2) / (1.0 - b1))
    assert all(isinstance(x, np.float32) for x in s.values())


def test_new_symbols_are_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in pkg.binding.EXPORTS
        assert re.search(r"\bint\s+%s\(" % sym, header), sym
    assert pkg.binding.EXPORTS[-len(NEW_SYMBOLS):] == list(NEW_SYMBOLS)          # appended
    assert pkg.binding.BUF["adamSecondMoments"] == max(pkg.binding.BUF.values())  # at the end of cn_buffer
    assert re.search(r"CN_BUF_LSTM_TMP_OUTPUTS,.*?CN_BUF_ADAM_SECOND_MOMENTS\s*\}\s*cn_buffer;", header, re.S)
    for name in ("update_weights_adam", "arm_adam"):
        assert hasattr(pkg.NeuralNetwork, name)
    for name in ("first_moments", "second_moments", "upload"):
        assert hasattr(pkg.network.Layer, name)


def test_library_exports_new_symbols(pkg):
    if not os.path.exists(pkg.lib_path()):
        import __graft_entry__ as ge
        ge.build()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path()], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for sym in NEW_SYMBOLS:
        assert sym in have, sym


def _driver(args, tmp_path):
    if not os.path.exists(BIN):
        import __graft_entry__ as ge
        ge.build()
    return subprocess.run([BIN, "--train", "true", "--network", str(tmp_path / "missing.jsn"), "--train_file", str(tmp_path / "missing.nc")] + args,
                          capture_output=True, text=True, timeout=60)


def test_driver_accepts_optimizer_adam(tmp_path):
    """Option parsing comes before the device and the files: an accepted option fails later, on the missing network file."""
    out = _driver(["--optimizer", "adam", "--adam_beta1", "0.8", "--adam_beta2", "0.99", "--adam_epsilon", "1e-7"], tmp_path)
    assert out.returncode == 2 and "unknown" not in out.stdout and "Cannot open file" in out.stdout, out.stdout
    out = _driver(["--optimizer", "steepest_descent"], tmp_path)
    assert out.returncode == 2 and "unknown" not in out.stdout and "Cannot open file" in out.stdout, out.stdout


def test_driver_rejects_other_optimizers_with_the_same_text(tmp_path):
    for bogus in ("rprop", "Adam", "sgd"):
        out = _driver(["--optimizer", bogus], tmp_path)
        assert out.returncode == 2
        assert "FAILED: Error while parsing the command line and/or options file: unknown optimizer '%s'" % bogus in out.stdout
