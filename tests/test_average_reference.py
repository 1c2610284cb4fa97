"""The restatement the GPU is held to (tests/average_reference.py), checked on the CPU: float32 against the same recurrence in
float64, the closed form for constant weights, the exact copy at decay 0; then that the feature is declared where the header,
the binding, the library and the driver declare such things."""
import os
import re
import subprocess

import numpy as np
import pytest

from average_reference import average_step, one_minus_decay, warmup_decay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
NEW_SYMBOLS = ("cn_ctx_average_weights", "cn_ctx_swap_weight_average", "cn_ctx_weight_average_state", "cn_layer_read_weight_average",
               "cn_layer_upload_weight_average")
DECAYS = (0.0, 0.1, 0.5, 0.9, 0.999, 0.9999)
BAD_DECAY_TEXT = "Error while parsing the command line and/or options file: --weight_average_decay must be in [0, 1) (0 = off)"


def magnitudes(rng, n):
    return ((10.0 ** rng.uniform(-6.0, 0.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


@pytest.mark.parametrize("decay", DECAYS)
def test_float32_restatement_stays_within_its_rounding_bound_of_float64(decay):
    """200 steps on 4096 entries of magnitudes 1e-6 ... 1 with moving w.  Three roundings per step on magnitudes <= 2M, M and M
    (M: the largest |w| or |avg| seen so far), and the map contracts, so errors do not grow: |avg32 - avg64| <= 5 n M 2^-24 after
    step n.  Both runs take the decay as float32 holds it; float64 forms 1 - decay exactly."""
    rng = np.random.RandomState(31)
    n = 4096
    d = float(np.float32(decay))
    w = magnitudes(rng, n)
    a32 = magnitudes(rng, n)
    a64 = a32.astype(np.float64)
    M, worst = float(max(np.abs(w).max(), np.abs(a32).max())), 0.0
    for step in range(1, 201):
        w = (w + magnitudes(rng, n) * np.float32(0.05)).astype(np.float32)
        a32 = average_step(a32, w, d)
        a64 = average_step(a64, w.astype(np.float64), d, dtype=np.float64)
        M = float(max(M, np.abs(w).max(), np.abs(a32).max()))
        bound = 5.0 * step * M * 2.0 ** -24
        diff = float(np.abs(a32.astype(np.float64) - a64).max())
        worst = max(worst, diff / bound)
        assert diff <= bound, (decay, step, diff, bound)
    print("decay %g: largest |avg32 - avg64| / bound = %.3g" % (decay, worst))
    assert a32.dtype == np.float32 and (decay == 0.0 or worst > 0.0)


@pytest.mark.parametrize("decay", DECAYS[1:])
def test_constant_weights_follow_the_closed_form(decay):
    """Constant w, float64: avg_n - w == (1 - omd)^n (avg_0 - w), to 1e-12 relative."""
    rng = np.random.RandomState(32)
    w, a0 = rng.randn(64), rng.randn(64)
    omd = float(one_minus_decay(decay, np.float64))
    a = a0.copy()
    for step in range(1, 101):
        a = average_step(a, w, decay, dtype=np.float64)
        want = (1.0 - omd) ** step * (a0 - w)
        assert np.abs((a - w) - want).max() <= 1e-12 * np.abs(a0 - w).max(), (decay, step)


def test_decay_zero_is_an_exact_copy():
    rng = np.random.RandomState(33)
    w, a = magnitudes(rng, 4096), magnitudes(rng, 4096)
    assert np.array_equal(average_step(a, w, 0.0), w)
    # avg + (w - avg) is not w in float32 ...
    one, tiny = np.float32(1.0), np.float32(1e-10)
    assert one + (tiny - one) != tiny
    # ... the step copies: omd == 1 at decay 0, and at every decay that 1 - decay rounds away (the driver's 1e-30)
    for decay in (0.0, 1e-30):
        assert one_minus_decay(decay) == np.float32(1.0)
        got = average_step(np.array([1.0], np.float32), np.array([1e-10], np.float32), decay)
        assert got.dtype == np.float32 and got[0] == tiny


def test_warmup_decay():
    assert warmup_decay(0.999, 1) == np.float32(0.999)                      # step 1: the decay as given (the first step copies anyway)
    assert warmup_decay(0.999, 2) == np.float32(2.0 / 11.0)
    assert warmup_decay(0.5, 5) == np.float32(5.0 / 14.0) and warmup_decay(0.5, 9) == np.float32(0.5) and warmup_decay(0.5, 100) == np.float32(0.5)
    assert all(isinstance(warmup_decay(0.9, k), np.float32) and 0 < warmup_decay(0.9, k) < 1 for k in range(1, 200))


def test_new_symbols_are_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    assert "Weight averaging" in header
    assert header.index("---- Weight averaging") < header.index("---- Adam")
    for sym in NEW_SYMBOLS:
        assert sym in pkg.binding.EXPORTS
        assert re.search(r"\bint\s+%s\(" % sym, header), sym
    adam = ["cn_adam_update", "cn_adam_update_all", "cn_ctx_arm_adam"]
    assert pkg.binding.EXPORTS[-3:] == adam                                  # still ends in the Adam section
    assert max(pkg.binding.EXPORTS.index(s) for s in NEW_SYMBOLS) < pkg.binding.EXPORTS.index("cn_adam_update")
    assert pkg.binding.BUF == {"outputs": 0, "outputErrors": 1, "weights": 2, "weightUpdates": 3, "weightDeltas": 4,
                               "cellStates": 5, "niActs": 6, "igActs": 7, "fgActs": 8, "ogActs": 9,
                               "niDeltas": 10, "igDeltas": 11, "fgDeltas": 12, "ogDeltas": 13, "tmpOutputs": 14,
                               "adamSecondMoments": 15}                      # cn_buffer gets no new value
    assert re.search(r"CN_BUF_ADAM_SECOND_MOMENTS\s*\}\s*cn_buffer;", header)
    for name in ("average_weights", "swap_weight_average", "weight_average_state"):
        assert hasattr(pkg.NeuralNetwork, name)
    for name in ("weight_average", "upload_weight_average"):
        assert hasattr(pkg.network.Layer, name)
    makefile = open(os.path.join(ROOT, "lstm-rnn_amd", "csrc", "Makefile")).read()
    objs = next(l for l in makefile.splitlines() if l.startswith("OBJS"))
    assert "cn_average.o" in objs.split() and os.path.exists(os.path.join(ROOT, "lstm-rnn_amd", "csrc", "cn_average.hip"))


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


def test_driver_accepts_the_weight_average_options(tmp_path):
    """Option parsing comes before the device and the files: an accepted option fails later, on the missing network file."""
    for args in (["--weight_average_decay", "0.999"], ["--weight_average_decay", "0"], ["--weight_average_decay", "1e-30"],
                 ["--weight_average_decay", "0.9", "--weight_average_warmup", "false"], ["--weight_average_warmup", "true"]):
        out = _driver(args, tmp_path)
        assert out.returncode == 2 and "unknown" not in out.stdout and "Cannot open file" in out.stdout, (args, out.stdout)
    usage = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--weight_average_decay" in usage and "--weight_average_warmup" in usage


@pytest.mark.parametrize("bad", ["-0.1", "1", "1.5", "nan", "inf"])
def test_driver_refuses_a_decay_outside_the_range(tmp_path, bad):
    out = _driver(["--weight_average_decay", bad], tmp_path)
    assert out.returncode == 2, out.stdout
    assert "FAILED: " + BAD_DECAY_TEXT in out.stdout, out.stdout
