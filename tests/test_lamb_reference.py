"""LAMB without a GPU: the numpy restatement the GPU tests compare against bit for bit (tests/lamb_reference.py) is LAMB -- it
agrees with a plain float64 LAMB written from the paper's formulas to the error its float32 operations allow --, a layer's step
has the size lr * |w|, the degenerate cases give ratio 1, both bounds bite, the six entry points are declared and exported, and
the driver knows the options."""
import os
import re
import subprocess

import numpy as np

import decay_reference as DR
import lamb_reference as LR_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip")
NEW_SYMBOLS = ("cn_lamb_update", "cn_lamb_update_all", "cn_ctx_arm_lamb", "cn_ctx_set_trust_bounds", "cn_ctx_get_trust_bounds",
               "cn_layer_trust_ratio")
EPS32 = 2.0 ** -24                  # unit roundoff of float32: one operation rounded to nearest errs by at most EPS32, relatively
L_, P_ = 6, 5                       # a small lstm layer: 6 units, 5 inputs -> 120 | 24 | 144 + 18 = 306 weights (two pad entries)


def paper_lamb_layer(w, g, m, v, decays, lr, lam, b1, b2, eps, t):
    """You et al. 2020, Algorithm 2, for one layer, in float64, phi the identity:
    m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  m^ = m / (1 - b1^t);  v^ = v / (1 - b2^t);  r = m^ / (sqrt(v^) + eps);
    w = w - lr * (|w| / |r + lam w|) * (r + lam w), the quotient of the norms read as 1 when either is 0."""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    mhat, vhat = m / (1.0 - b1 ** t), v / (1.0 - b2 ** t)
    r = mhat / (np.sqrt(vhat) + eps)
    u = r + np.where(decays, lam * w, 0.0)
    nw, nu = np.linalg.norm(w), np.linalg.norm(u)
    phi = nw / nu if nw > 0 and nu > 0 else 1.0
    return w - lr * phi * u, m, v, r, u, phi


def layer_state(rng):
    n = DR.weight_count("lstm", L_, P_)
    pad = LR_.padded(n)
    mask = DR.decay_mask(pad, DR.decayed_ranges("lstm", L_, P_))
    w = np.zeros(pad, np.float32)
    w[:n] = rng.uniform(-0.3, 0.3, n)
    sign = np.zeros(pad, np.float32)
    sign[:n] = rng.choice([-1.0, 1.0], n)
    return n, pad, mask, w, sign


def gradient(rng, n, pad, sign):
    """magnitudes 1e-4 ... 1 with one fixed sign per entry: b1 * m and omb1 * g then never cancel"""
    g = np.zeros(pad, np.float32)
    g[:n] = 10.0 ** rng.uniform(-4.0, 0.0, n)
    return g * sign


def test_restatement_is_paper_lamb_to_float32_rounding():
    """Five steps, decay 0.01, lr 0.01.  Every step starts both versions from the restatement's float32 state, and the float64
    version takes the hyper-parameters as float32 holds them (the entry points take floats), so the two differ by the float32
    roundings of ONE step.  With e = 2^-24 and entries whose gradient keeps its sign (no cancellation in m; none in v anyway):
        m: scalar rounding + product, then the sum                      <= 3e relative
        v: omb2 rounding, g*g, product, sum                             <= 4e relative
        r: numerator c_t*m: 3e + c_t's rounding + product = 5e; denominator: sqrt halves v's 4e and rounds (3e), eps_t's term is
           smaller still, the sum rounds (4e); the division rounds      <= 5e + 4e + e = 10e relative
        u = r + decay*w may cancel: |du_i| <= 10e |r_i| + 2e |decay w_i| + e |u_i| =: a_i (absolute)
        nu: |dnu| <= |a|_2, and one rounding to float; nw: one rounding -> ratio <= e + (|a|_2 / nu + e) + e =: q relative
        step = lr * ratio: lr's rounding and the product               <= q + 2e =: s relative
        d = step * u_i: |dd_i| <= step * a_i + (s + e) |d_i|;  w' = w - d rounds once: |dw'_i| <= |dd_i| + e |w'_i|
    (first order in e; the factor 1.01 below covers the second).  The bound is derived here, not fitted."""
    rng = np.random.RandomState(61)
    n, pad, mask, w32, sign = layer_state(rng)
    m32, v32 = np.zeros(pad, np.float32), np.zeros(pad, np.float32)
    lr, lam = float(np.float32(0.01)), float(np.float32(0.01))
    b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
    e = EPS32
    worst = 0.0
    for t in range(1, 6):
        g = gradient(rng, n, pad, sign)
        w64, m64, v64, r64, u64, phi = paper_lamb_layer(w32.astype(np.float64), g.astype(np.float64), m32.astype(np.float64),
                                                        v32.astype(np.float64), mask, lr, lam, b1, b2, eps, t)
        w32n, m32, v32, rec = LR_.lamb_layer_step(w32, g, m32, v32, mask, lr, lam, step=t)
        assert np.all(np.abs(m32 - m64) <= 1.01 * 3 * e * np.abs(m64)) and np.all(np.abs(v32 - v64) <= 1.01 * 4 * e * np.abs(v64))
        a = 10 * e * np.abs(r64) + 2 * e * np.abs(np.where(mask, lam * w32.astype(np.float64), 0.0)) + e * np.abs(u64)
        nu = np.linalg.norm(u64)
        q = 3 * e + np.linalg.norm(a) / nu
        assert abs(float(rec[0]) - phi) <= 1.01 * q * phi
        assert abs(float(rec[1]) - np.linalg.norm(w32.astype(np.float64))) <= 1.01 * e * float(rec[1])
        assert abs(float(rec[2]) - nu) <= 1.01 * (np.linalg.norm(a) + e * nu)
        d64 = lr * phi * u64
        bound = 1.01 * (lr * phi * a + (q + 3 * e) * np.abs(d64) + e * np.abs(w64))
        err = np.abs(w32n.astype(np.float64) - w64)
        assert np.all(err <= bound), (t, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[:n] / bound[:n]).max()))
        assert np.abs(w32n - w32).max() > 1e-4             # the weights moved
        w32 = w32n
    print("restatement vs float64 LAMB: largest error / bound %.3f" % worst)
    assert not w32[n:].any() and not m32[n:].any() and not v32[n:].any()          # pad entries stay zero


def test_a_layers_step_has_the_size_lr_times_its_weights():
    """Bounds off, decay 0: |w' - w| / |w| = lr for every layer, over five steps.  d = step * u with step = lr * nw / nu: nw and nu
    are rounded to float (e each), the division, lr's rounding, the product lr * ratio and the product step * u_i round (4e), so
    |d| = lr |w| (1 + 6e); w' = w - d rounds once per entry, an error of at most e |w'_i| that the difference w' - w inherits:
    | |w' - w| / |w| - lr | <= 6e lr + e (1 + lr), first order; the factor 1.01 covers the second."""
    rng = np.random.RandomState(62)
    layers = [("lstm", L_, P_), ("softmax", 7, L_), ("feedforward_tanh", 9, 7)]
    segs, mask, total = LR_.arena_layout(layers)
    w, m, v = np.zeros(total, np.float32), np.zeros(total, np.float32), np.zeros(total, np.float32)
    for a, b, n in segs:
        w[a:a + n] = rng.uniform(-0.5, 0.5, n)
    lr = 0.01
    tol = 1.01 * (6 * EPS32 * lr + EPS32 * (1 + lr))
    for t in range(1, 6):
        g = np.zeros(total, np.float32)
        for a, b, n in segs:
            g[a:a + n] = rng.randn(n) * 10.0 ** rng.uniform(-3, 0)
        wn, m, v, recs = LR_.lamb_step(w, g, m, v, [(a, b, lr) for a, b, _ in segs], mask, step=t)
        for (a, b, _), rec in zip(segs, recs):
            rel = np.linalg.norm(wn[a:b].astype(np.float64) - w[a:b].astype(np.float64)) / np.linalg.norm(w[a:b].astype(np.float64))
            assert abs(rel - float(np.float32(lr))) <= tol, (t, rel)
            assert rec[0] > 0 and rec[1] > 0 and rec[2] > 0
        w = wn


def test_degenerate_layers_take_ratio_one():
    rng = np.random.RandomState(63)
    n, pad, mask, w, sign = layer_state(rng)
    g = gradient(rng, n, pad, sign)
    zeros = np.zeros(pad, np.float32)
    # an all-zero layer: nw == 0 -> ratio 1, and the step is lr * u
    wn, m, v, rec = LR_.lamb_layer_step(zeros, g, zeros, zeros, mask, 0.01, 0.01, step=1)
    assert rec[0] == 1.0 and rec[1] == 0.0 and rec[2] > 0
    _, _, u = LR_.lamb_direction(zeros, g, zeros, zeros, mask, 0.01, step=1)
    assert np.array_equal(wn, zeros - np.float32(0.01) * u) and wn[:n].any()
    # zero gradient with zero moments (decay 0): u == 0 -> nu == 0 -> ratio 1, weights unchanged
    wn, m, v, rec = LR_.lamb_layer_step(w, zeros, zeros, zeros, mask, 0.01, 0.0, step=1)
    assert rec[0] == 1.0 and rec[1] > 0 and rec[2] == 0.0
    assert np.array_equal(wn, w) and not m.any() and not v.any()
    # a sum that is not finite: ratio 1
    big = w.copy(); big[3] = np.inf
    assert LR_.trust_ratio(big, g)[0] == 1.0 and LR_.trust_ratio(w, big)[0] == 1.0


def test_both_bounds_bite():
    rng = np.random.RandomState(64)
    n, pad, mask, w, sign = layer_state(rng)
    g = gradient(rng, n, pad, sign)
    zeros = np.zeros(pad, np.float32)
    free = LR_.lamb_layer_step(w, g, zeros, zeros, mask, 0.01, step=1)
    nat = float(free[3][0])
    assert LR_.lamb_layer_step(w, g, zeros, zeros, mask, 0.01, bounds=(0.5 * nat, 2 * nat), step=1)[3][0] == free[3][0]
    lo = LR_.lamb_layer_step(w, g, zeros, zeros, mask, 0.01, bounds=(2 * nat, 0.0), step=1)
    hi = LR_.lamb_layer_step(w, g, zeros, zeros, mask, 0.01, bounds=(0.0, 0.5 * nat), step=1)
    assert lo[3][0] == np.float32(2 * nat) and hi[3][0] == np.float32(0.5 * nat)
    assert lo[3][1:] == free[3][1:] and hi[3][1:] == free[3][1:]                    # the norms are the natural ones
    d_free, d_lo, d_hi = (np.linalg.norm(x[0].astype(np.float64) - w) for x in (free, lo, hi))
    # (each |w' - w| carries the rounding of w', e |w| against a step of lr |w| * factor: at most 3e / lr on the quotients, first order)
    assert abs(d_lo / d_free - 2.0) < 4 * EPS32 / 0.01 and abs(d_hi / d_free - 0.5) < 4 * EPS32 / 0.01
    assert LR_.lamb_layer_step(w, g, zeros, zeros, mask, 0.01, bounds=(2 * nat, 2 * nat), step=1)[3][0] == np.float32(2 * nat)


def test_scalars_are_rounded_once_and_lr_stays_outside():
    s = LR_.lamb_scalars(0.9, 0.999, 1e-8, 3)
    b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
    assert s["omb1"] == np.float32(1.0 - b1) and s["omb2"] == np.float32(1.0 - b2)
    assert s["c_t"] == np.float32(np.sqrt(1.0 - b2 ** 3) / (1.0 - b1 ** 3)) and s["eps_t"] == np.float32(eps * np.sqrt(1.0 - b2 ** 3))
    assert all(isinstance(x, np.float32) for x in s.values())


def test_new_symbols_are_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "currennt_hip.h")).read()
    assert "---- LAMB" in header
    for sym in NEW_SYMBOLS:
        assert sym in pkg.binding.EXPORTS
        assert re.search(r"\bint\s+%s\(" % sym, header), sym
    for name in ("update_weights_lamb", "arm_lamb", "set_trust_bounds", "trust_bounds"):
        assert hasattr(pkg.NeuralNetwork, name)
    assert hasattr(pkg.network.Layer, "trust_ratio")


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
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60)


def test_driver_knows_the_lamb_options(tmp_path):
    out = _driver(["--help"], tmp_path)
    assert "--lamb_min_trust" in out.stdout and "--lamb_max_trust" in out.stdout and "steepest_descent|adam|lamb" in out.stdout
    # option parsing comes before the device and the files: an accepted option fails later, on the missing network file
    missing = ["--train", "true", "--network", str(tmp_path / "missing.jsn"), "--train_file", str(tmp_path / "missing.nc")]
    out = _driver(missing + ["--optimizer", "lamb", "--lamb_min_trust", "0.1", "--lamb_max_trust", "10"], tmp_path)
    assert out.returncode == 2 and "unknown" not in out.stdout and "Cannot open file" in out.stdout, out.stdout
    out = _driver(missing + ["--optimizer", "lamb", "--lamb_max_trust", "-1"], tmp_path)
    assert out.returncode == 2 and "--lamb_max_trust must be finite and >= 0" in out.stdout, out.stdout
    out = _driver(missing + ["--optimizer", "lars"], tmp_path)
    assert out.returncode == 2 and "unknown optimizer 'lars'" in out.stdout and "lamb" in out.stdout.split("unknown optimizer")[1]
