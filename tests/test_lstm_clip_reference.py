"""CPU: the float64 restatement of the clipped LSTM backward cell (tests/lstm_clip_reference.py) against the double oracle, the
input recipe that tests/test_gpu_lstm_clip.py shares, the conditions on those inputs, and the teeth of the comparison.

Why: every backward recurrent kernel clips the four gate deltas to [-1, 1] when it stores them, and with the suite's usual
inputs (weights +-0.04 .. 0.4, errors of order 1) no delta comes near 1: the clip, what it is applied to, and what reads the
clipped or the unclipped value were outside every GPU test.  Here a layer gets LARGE injected errors (Layer.write_output_errors +
Layer.backward / OracleNetwork.backward_layer) on top of an ordinary forward pass: no large weights, no saturated gates, no
forward comparison changes.

The recipe (build_inputs): input 9 -> lstm 32 -> the layer under test -> softmax 7; weights random_weights at the scale the
existing tests use for the width; PS = 12 with 11 sequences of lengths [T, T, T-1, T-2, T-2, ceil(T/2), .., 2, 1, T] and one
unused slot; errors randn * SLOT_SCALE[slot] -- 0.5 .. 128, so that clipped and unclipped sequences share a workgroup, a pair
and a quad --; dummy frames of the error array hold 1e4.

Conditions on the inputs (asserted per case of the GPU module, from the references alone): per direction and gate, over the real
frames, the forced set F = {|u64| >= m} (u64: the UNCLIPPED delta in float64) holds >= 1 % and the free set {|u64| <= 0.8}
>= 25 %; on F the model of the case's arithmetic -- the fp32 oracle, the split-operand model, the bf16 operand model -- stores
exactly sign(u64).  m = 1.01 for f32 and bf16x3, 1.25 for bf16.  Measured: forced 1.3 % (forget gate, blstm1024) .. 65 % (net input),
free 33 .. 97 %.

Teeth: three wrong rules (no clip; the cell state error from the clipped output gate delta; unclipped deltas in the carry) must each
move a compared quantity by more than 10 of the GPU module's bounds on every case.  f32 and bf16x3: 113 .. 5e4 bounds, or onto the
forced set.  bf16: the tolerances against the bf16 operand model are too wide for the second and the third (1.6 .. 50 bounds, below
10 in 12 of 20 pairs); the replay of the stored deltas (lstm_clip_reference.replay_stored_deltas, bound 1, an unmutated stand-in
reaches 0.99) gives 19 .. 371.
"""
import os

import numpy as np
import pytest

from helpers import net_desc, random_sequences, random_weights, real_mask
from lstm_clip_reference import GATES, SECTIONS, computed_frames, lstm_backward_clip, replay_stored_deltas, split_gradient

K = 8.46                      # tests/test_gpu_long_fp64.py (tools/derive_fp64_k.py)
PS, P_IN, C_OUT, BELOW = 12, 9, 7, ("lstm", 32)
SLOT_SCALE = [32, 0.5, 8, 32, 8, 0.5, 32, 8, 32, 32, 128, 1]
DUMMY_ERROR = 1e4
FORCED = {"f32": 1.01, "bf16x3": 1.01, "bf16": 1.25}
FREE = 0.8
GRAD_TOL_F32 = 2e-4           # test_gpu_parity.check_network
GRAD_TOL_BF16_PINNED, ERR_TOL_BF16_PINNED = 2e-3, 5e-3         # tests/test_gpu_bf16_pinned.py
DELTA_TOL_BF16 = 2.0 ** -7    # one bf16 step of a value below 1 (the rule of tests/test_gpu_bf16_pinned.py)
BELOW_SCALE = 0.4             # the layer below and the output layer: the narrow layers of test_gpu_parity.test_single_lstm_layer_internals
# The layer under test: the scale the existing tests use for a layer of that width (test_gpu_parity.py, test_gpu_bf16_pinned.py), with two
# exceptions that the conditions on the inputs ask for: 384 takes the 0.1 of the other wide register-resident shape (192) instead of
# 0.05 (forced share of the input gate 0.5 %), 1024 the 0.06 of the 2-CU cluster width instead of 0.04 / 0.05 (forced share of the
# forget gate 0.93 % at 0.05).  The largest is the 0.4 of the 20-unit layer.
WEIGHT_SCALE = {20: 0.4, 128: 0.1, 192: 0.1, 250: 0.1, 320: 0.08, 384: 0.1, 500: 0.06, 1024: 0.06}

# The cases of tests/test_gpu_lstm_clip.py: id -> (kind, size, T, mode, environment, backward kernel[, twin environment, twin kernel]).
# A twin is the compiled kernel a hand-written or generated loop is held bit-equal to.
_S2C = {"CN_NO_S2C": "1"}
GPU_CASES = {
    # compiled single-CU kernels, lstm_bwd_kernel
    "f32-Hp32": ("lstm", 20, 9, "f32", {}, "lstm_bwd_kernel<1,32,1,1>"),
    "f32-Hp128-rpl1": ("blstm", 250, 9, "f32", {}, "lstm_bwd_kernel<1,128,1,1>"),
    "f32-Hp128-rpl2": ("blstm", 250, 9, "f32", {"CN_RPL": "2"}, "lstm_bwd_kernel<1,128,1,2>"),
    "f32-streaming": ("blstm", 320, 9, "f32", {}, "lstm_bwd_kernel<1,0,1,1>"),
    "x3-Hp128": ("blstm", 250, 9, "bf16x3", {"CN_NO_S2_ASM": "1"}, "lstm_bwd_kernel<2,128,1,1>"),
    "bf16-Hp96": ("blstm", 192, 9, "bf16", {}, "lstm_bwd_kernel<0,96,1,1>"),
    "bf16-Hp192": ("blstm", 384, 9, "bf16", {}, "lstm_bwd_kernel<0,192,1,1>"),
    "bf16-Hp128-ug1": ("blstm", 250, 9, "bf16", {"CN_NO_S2": "1"}, "lstm_bwd_kernel<0,128,1,1>"),
    "bf16-Hp128-ug2": ("blstm", 250, 9, "bf16", {"CN_NO_S2": "1", "CN_BWD_UG2": "1"}, "lstm_bwd_kernel<0,128,2,1>"),
    # the two-sequence cut
    "s2-Hp64-T9": ("blstm", 128, 9, "bf16", {}, "lstm_bwd_s2_kernel<0,64>"),
    "s2-Hp64-T33": ("blstm", 128, 33, "bf16", {}, "lstm_bwd_s2_kernel<0,64>"),
    "s2-asm-T9": ("blstm", 250, 9, "bf16", {}, "lstm_bwd_s2_asm_kernel", {"CN_NO_S2_ASM": "1"}, "lstm_bwd_s2_kernel<0,128>"),
    "s2-asm-T33": ("blstm", 250, 33, "bf16", {}, "lstm_bwd_s2_asm_kernel", {"CN_NO_S2_ASM": "1"}, "lstm_bwd_s2_kernel<0,128>"),
    "s2-x3-asm-T9": ("blstm", 250, 9, "bf16x3", {"CN_S2_X3": "1"}, "lstm_bwd_s2_x3_asm_kernel",
                     {"CN_S2_X3": "1", "CN_NO_S2_ASM": "1"}, "lstm_bwd_s2_kernel<2,128>"),
    "s2-x3-asm-T33": ("blstm", 250, 33, "bf16x3", {"CN_S2_X3": "1"}, "lstm_bwd_s2_x3_asm_kernel",
                      {"CN_S2_X3": "1", "CN_NO_S2_ASM": "1"}, "lstm_bwd_s2_kernel<2,128>"),
    # Hp = 256
    "s2c-asm-T9": ("blstm", 500, 9, "bf16", {}, "lstm_bwd_s2c_asm_kernel", {"CN_S2C": "1"}, "lstm_bwd_s2c_kernel"),
    "s2c-asm-T33": ("blstm", 500, 33, "bf16", {}, "lstm_bwd_s2c_asm_kernel", {"CN_S2C": "1"}, "lstm_bwd_s2c_kernel"),
    "cluster256-rpl1": ("blstm", 500, 9, "bf16", _S2C, "lstm_bwd_cluster_kernel<0,256,128,1>"),
    "cluster256-rpl2": ("blstm", 500, 9, "bf16", dict(_S2C, CN_RPL="2"), "lstm_bwd_cluster_kernel<0,256,128,2>"),
    "cluster256-four": ("blstm", 500, 9, "bf16", dict(_S2C, CN_CLUSTER4="1"), "lstm_bwd_cluster_kernel<0,256,64,1>"),
    "psum256": ("blstm", 500, 9, "bf16", {"CN_BWD_PSUM": "1", "CN_NO_S2W": "1"}, "lstm_bwd_cluster_psum_kernel<0,256,128>"),
    "x3-psum256": ("blstm", 500, 9, "bf16x3", {}, "lstm_bwd_cluster_psum_kernel<2,256,64>"),
    "x3-cluster256": ("blstm", 500, 9, "bf16x3", {"CN_NO_BWD_PSUM": "1"}, "lstm_bwd_cluster_kernel<2,256,64,1>"),
    # Hp = 512, bf16: the packed exchange (4-bit step tag in bit 14 of a lane's four bf16 deltas: correct because |delta| <= 1);
    # T = 33 takes the 15-step tag around twice
    "cluster512-helpers-T9": ("blstm", 1024, 9, "bf16", {}, "lstm_bwd_cluster_kernel<0,512,64,1>"),
    "cluster512-helpers-T33": ("blstm", 1024, 33, "bf16", {}, "lstm_bwd_cluster_kernel<0,512,64,1>"),
    "cluster512-plain-T9": ("blstm", 1024, 9, "bf16", {"CN_NO_CLUSTER_HELPERS": "1"}, "lstm_bwd_cluster_kernel<0,512,64,1>"),
    "cluster512-plain-T33": ("blstm", 1024, 33, "bf16", {"CN_NO_CLUSTER_HELPERS": "1"}, "lstm_bwd_cluster_kernel<0,512,64,1>"),
    "cluster512-rpl2-T9": ("blstm", 1024, 9, "bf16", {"CN_RPL": "2"}, "lstm_bwd_cluster_kernel<0,512,64,2>"),
    "cluster512-rpl2-T33": ("blstm", 1024, 33, "bf16", {"CN_RPL": "2"}, "lstm_bwd_cluster_kernel<0,512,64,2>"),
    "psum512": ("blstm", 1024, 9, "bf16", {"CN_BWD_PSUM": "1"}, "lstm_bwd_cluster_psum_kernel<0,512,64>"),
}
# the distinct (inputs, arithmetic) pairs among them: what the CPU checks below run over
INPUT_MODES = sorted({(c[0], c[1], c[2], c[3]) for c in GPU_CASES.values()})


def lengths_for(T):
    half = -(-T // 2)
    quarter = -(-half // 2)                                           # the ".." of the recipe: halved twice more, rounded up
    return [T, T, T - 1, T - 2, T - 2, half, quarter, -(-quarter // 2), 2, 1, T]


def build_inputs(pkg, kind, size, T):
    """The shared recipe -> dict(layers, weights, frac, errors [T][PS][size], name of the layer under test, ...)."""
    rng = np.random.RandomState(9000 + size + T)
    layers = net_desc(P_IN, [BELOW, (kind, size)], C_OUT)
    weights = random_weights(layers, rng, BELOW_SCALE)
    name = "%s_1" % kind
    # the layer under test at the scale of its width
    weights[name] = random_weights([{"name": "below", "type": "input", "size": BELOW[1]}, layers[2]], rng, WEIGHT_SCALE[size])[name]
    lengths = lengths_for(T)
    assert len(lengths) == PS - 1 and max(lengths) == T
    xs, ts = random_sequences(rng, lengths, P_IN, C=C_OUT)
    frac = pkg.make_fraction(xs, ts, PS)
    real = real_mask(frac).reshape(T, PS)
    errors = (rng.randn(T, PS, size) * np.asarray(SLOT_SCALE, np.float64)[None, :, None]).astype(np.float32)
    # dummy frames: those the layer checks (t >= Tmin) and finds without a pattern.  Frame 0 of the unused slot lies before Tmin = 1:
    # the reference computes it like a real one (lstm_clip_reference.computed_frames), and so do the compiled kernels, while the
    # hand-written and generated loops treat it as a dummy frame.  No layer ever hands an error to such a
    # frame, and with a zero error both readings store zero deltas there: it gets 0, not DUMMY_ERROR.
    dummy = ~computed_frames(frac["patTypes"], T, PS, frac["Tmin"])
    assert frac["Tmin"] == 1 and (real | dummy).sum() == T * PS - 1
    errors[dummy] = DUMMY_ERROR
    errors[~real & ~dummy] = 0.0
    return {"kind": kind, "size": size, "T": T, "layers": layers, "weights": weights, "frac": frac, "errors": errors, "name": name,
            "real": real, "dummy": dummy, "dirs": 2 if kind == "blstm" else 1, "H": size // (2 if kind == "blstm" else 1), "below": BELOW[1]}


def oracle_run(ons, inp, rounding=None, errors=None):
    """Forward pass of the whole net, then the injected errors through the layer under test alone (OracleNetwork.backward_layer),
    in the oracle namespace `ons` under an operand rounding model.  -> (quantities, the layer)."""
    T = inp["T"]
    with ons.operand_rounding(rounding):
        ref = ons.OracleNetwork(inp["layers"], inp["weights"], PS, T)
        ref.load_sequences(inp["frac"]); ref.compute_forward_pass()
        lay = ref.layer(inp["name"])
        e = inp["errors"] if errors is None else errors
        lay.outputErrors[:] = np.asarray(e, lay.outputErrors.dtype).reshape(-1)
        ref.backward_layer(lay)
    H = inp["H"]
    deltas = [{g: lay.internal(g + "Deltas", d).reshape(T, PS, H).astype(np.float64) for g in GATES} for d in range(inp["dirs"])]
    q = {"deltas": deltas, "grad_flat": lay.weightUpdates.astype(np.float64),
         "prev_errors": lay.prev.outputErrors.reshape(T, PS, inp["below"]).astype(np.float64)}
    return q, lay


def numpy_reference(inp, lay64, **switches):
    """tests/lstm_clip_reference.py on the double oracle's forward internals."""
    T, H = inp["T"], inp["H"]
    internals = [{n: lay64.internal(n, d).reshape(T, PS, H) for n in ("niActs", "igActs", "fgActs", "ogActs", "cellStates")}
                 for d in range(inp["dirs"])]
    x = lay64.prev.outputs.reshape(T, PS, inp["below"])
    out = lstm_backward_clip(internals, lay64.weights, inp["frac"]["patTypes"], x, inp["errors"], t_min=inp["frac"]["Tmin"], bias=lay64.bias, **switches)
    out["deltas"] = out["stored"]
    return out


def flat_weights(inp):
    w = inp["weights"][inp["name"]]
    return np.concatenate([np.asarray(w[k], np.float32) for k in ("input", "bias", "internal")])


def replay(inp, internals, stored):
    """lstm_clip_reference.replay_stored_deltas on what a bf16 kernel (or its CPU stand-in) stored: {"<d>/<gate>": largest
    |stored - rule| / bound, "dummy": largest |delta| on a dummy frame}."""
    return replay_stored_deltas(internals, flat_weights(inp), inp["frac"]["patTypes"], inp["errors"], stored, t_min=inp["frac"]["Tmin"])


def distances(got, r64, inp):
    """Per compared quantity, `got` against the double oracle: delta/<direction>/<gate> max-abs over the real frames (a stored
    delta lies in [-1, 1] and reaches both ends: the scale is 1); grad/<section> max-abs over the section's OWN largest entry, so
    that a wrong peephole sum cannot hide under dW_in; err: the errors handed to the preceding layer, real frames, over their max."""
    real = inp["real"]
    d = {}
    for dd in range(inp["dirs"]):
        for g in GATES:
            d["delta/%d/%s" % (dd, g)] = float(np.abs(got["deltas"][dd][g][real] - r64["deltas"][dd][g][real]).max())
    a = split_gradient(got["grad_flat"], inp["below"], inp["size"], inp["dirs"] == 2)
    b = split_gradient(r64["grad_flat"], inp["below"], inp["size"], inp["dirs"] == 2)
    for s in SECTIONS:
        d["grad/" + s] = float(np.abs(a[s] - b[s]).max() / max(1e-300, np.abs(b[s]).max()))
    d["err"] = float(np.abs(got["prev_errors"][real] - r64["prev_errors"][real]).max() / np.abs(r64["prev_errors"][real]).max())
    return d


_REFS = {}


def references(pkg, orc, kind, size, T, mode):
    """The references of one (inputs, arithmetic) pair, computed once: the inputs, R64 (double oracle), U64 (the unclipped deltas,
    numpy on R64's internals), R32 (fp32 oracle), the model of `mode` (f32: R32; bf16x3: the split-operand model in double; bf16:
    the bf16 operand model in fp32), D_ref, D_model, the forced sets and the bounds of the GPU module."""
    key = (kind, size, T)
    o64 = orc.real64()
    n = min(16, len(os.sched_getaffinity(0)))
    prev, prev64 = orc.get_threads(), o64.get_threads()
    orc.set_threads(n); o64.set_threads(n)
    try:
        if key not in _REFS:
            inp = build_inputs(pkg, kind, size, T)
            r64, lay64 = oracle_run(o64, inp)
            ref = numpy_reference(inp, lay64)
            r32, _ = oracle_run(orc, inp)
            _REFS[key] = {"inp": inp, "R64": r64, "lay64": lay64, "NP": ref, "U64": ref["unclipped"], "R32": r32,
                          "D_ref": distances(r32, r64, inp), "model": {"f32": r32}}
        base = _REFS[key]
        if mode not in base["model"]:
            base["model"][mode] = oracle_run(o64, base["inp"], rounding="bf16x3")[0] if mode == "bf16x3" else oracle_run(orc, base["inp"], rounding="bf16")[0]
    finally:
        orc.set_threads(prev); o64.set_threads(prev64)
    case = dict(base)
    inp = case["inp"]
    case["mode"] = mode
    case["M"] = base["model"][mode]
    case["D_model"] = {k: 0.0 for k in case["D_ref"]} if mode == "f32" else distances(case["M"], case["R64"], inp)
    m = FORCED[mode]
    case["F"] = [{g: (np.abs(case["U64"][d][g]) >= m) & inp["real"][:, :, None] for g in GATES} for d in range(inp["dirs"])]
    case["bound"] = bounds(case)
    return case


def bounds(case):
    """What tests/test_gpu_lstm_clip.py holds a kernel to, per quantity of distances() (against the double oracle unless stated):
    f32: K * D_ref; bf16x3: K * (D_model + D_ref); bf16: the gradient sections K * (D_model + D_ref), the deltas off the forced
    set one bf16 step (2^-7) and the propagated errors ERR_TOL_BF16_PINNED, those two against the bf16 operand model."""
    b = {}
    for q, dr in case["D_ref"].items():
        b[q] = K * (dr + case["D_model"][q])
        if case["mode"] == "bf16" and q.startswith("delta/"):
            b[q] = DELTA_TOL_BF16
        if case["mode"] == "bf16" and q == "err":
            b[q] = ERR_TOL_BF16_PINNED
    return b


def fmt(d):
    return {k: float("%.3g" % v) for k, v in sorted(d.items())}


# ---- a. the reference against the double oracle -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,size,T", sorted({k[:3] for k in INPUT_MODES}))
def test_float64_restatement_equals_the_double_oracle(pkg, orc, kind, size, T):
    """Every returned quantity at 1e-12 (relative to the quantity's largest entry) against oracle.real64() through
    backward_layer: stored deltas, cell state errors, the four gradient sections, the propagated errors; and clipping the
    returned unclipped deltas gives the stored ones."""
    case = references(pkg, orc, kind, size, T, "f32")
    inp, ref, r64, lay64 = case["inp"], case["NP"], case["R64"], case["lay64"]
    worst = distances(ref, r64, inp)
    for d in range(inp["dirs"]):
        ce = lay64.internal("cellStateErrors", d).reshape(T, PS, inp["H"])[inp["real"]]
        worst["cell_errors/%d" % d] = float(np.abs(ref["cell_errors"][d][inp["real"]] - ce).max() / np.abs(ce).max())
        for g in GATES:
            assert np.array_equal(np.clip(ref["unclipped"][d][g], -1, 1), ref["stored"][d][g])
            assert np.all(ref["stored"][d][g][inp["dummy"]] == 0)
    print(kind, size, T, fmt(worst))
    assert all(v <= 1e-12 for v in worst.values()), fmt(worst)
    assert np.array_equal(np.concatenate([ref["grad"][s] for s in SECTIONS]), ref["grad_flat"])


# ---- c. conditions on the inputs ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,size,T,mode", INPUT_MODES)
def test_inputs_force_and_free_every_gate_and_the_models_store_the_sign(pkg, orc, kind, size, T, mode):
    case = references(pkg, orc, kind, size, T, mode)
    inp = case["inp"]
    real = inp["real"]
    nreal = float(real.sum() * inp["H"])
    shares = {}
    for d in range(inp["dirs"]):
        for g in GATES:
            u, F = case["U64"][d][g], case["F"][d][g]
            forced = F.sum() / nreal
            free = (np.abs(u[real]) <= FREE).sum() / nreal
            shares["%d/%s" % (d, g)] = (float("%.3g" % forced), float("%.3g" % free))
            assert forced >= 0.01, (d, g, forced)
            assert free >= 0.25, (d, g, free)
            for name, q in (("R32", case["R32"]), ("model", case["M"])) if mode == "f32" else (("model", case["M"]),):
                assert np.array_equal(q["deltas"][d][g][F], np.sign(u[F])), (name, d, g, int((q["deltas"][d][g][F] != np.sign(u[F])).sum()))
    print(kind, size, T, mode, "forced / free shares", shares)
    print("D_ref", fmt(case["D_ref"])); print("D_model", fmt(case["D_model"]))


# ---- d. dummy frames are never read -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,size,T", sorted({k[:3] for k in INPUT_MODES if k[2] == 9}))
def test_the_oracle_never_reads_the_errors_of_dummy_frames(pkg, orc, kind, size, T):
    case = references(pkg, orc, kind, size, T, "f32")
    inp = case["inp"]
    zeroed = inp["errors"].copy()
    zeroed[inp["dummy"]] = 0.0
    assert np.all(inp["errors"][inp["dummy"]] == DUMMY_ERROR) and inp["dummy"].sum() > 0
    other, _ = oracle_run(orc, inp, errors=zeroed)
    r32 = case["R32"]
    assert np.array_equal(other["grad_flat"], r32["grad_flat"])
    assert np.array_equal(other["prev_errors"], r32["prev_errors"])
    for d in range(inp["dirs"]):
        for g in GATES:
            assert np.array_equal(other["deltas"][d][g], r32["deltas"][d][g])


# ---- e. teeth -----------------------------------------------------------------------------------------------------------------

MUTANTS = {"no_clip": {"clip": False}, "ec_from_clipped_dog": {"ec_from_clipped_dog": True}, "carry_unclipped": {"carry_unclipped": True}}


def mutant_ratio(case, mutated):
    """Largest distance / bound over the compared quantities between the mutated and the true restatement; a difference on the
    forced set, where the GPU module asks for exact signs, counts as infinite."""
    inp, ref = case["inp"], case["NP"]
    dist = distances(mutated, ref, inp)
    ratios = {q: v / case["bound"][q] for q, v in dist.items()}
    for d in range(inp["dirs"]):
        for g in GATES:
            F = case["F"][d][g]
            if np.any(mutated["deltas"][d][g][F] != ref["deltas"][d][g][F]):
                ratios["delta/%d/%s" % (d, g)] = float("inf")
    if case["mode"] == "bf16":        # the replay of what a bf16 kernel with that rule would have stored (bound: 1)
        for k, v in replay(inp, bf16_internals(case), mutated["stored_bf16"]).items():
            ratios["replay/" + k] = float("inf") if (k == "dummy" and v > 0) else v
    q = max(ratios, key=ratios.get)
    return q, ratios[q], ratios


def bf16_internals(case):
    inp, lay = case["inp"], case["lay64"]
    return [{n: lay.internal(n, d).reshape(inp["T"], PS, inp["H"]).astype(np.float32).astype(np.float64) for n in ("niActs", "igActs", "fgActs", "ogActs", "cellStates")}
            for d in range(inp["dirs"])]


def bf16_stand_in(case, **switches):
    """A CPU stand-in for a CN_PREC_BF16 backward kernel with the given rule: the float64 restatement on fp32 forward internals with
    bf16 W_rec and bf16 stored deltas (lstm_backward_clip(bf16_operands=True)).  -> the stored deltas per direction."""
    inp, lay = case["inp"], case["lay64"]
    x = lay.prev.outputs.reshape(inp["T"], PS, inp["below"])
    return lstm_backward_clip(bf16_internals(case), lay.weights.astype(np.float32), inp["frac"]["patTypes"], x, inp["errors"], t_min=inp["frac"]["Tmin"],
                              bias=lay.bias, bf16_operands=True, **switches)["stored"]


@pytest.mark.parametrize("kind,size,T,mode", INPUT_MODES)
def test_each_wrong_rule_moves_a_compared_quantity_ten_bounds(pkg, orc, kind, size, T, mode):
    """A kernel that did not clip, that built the cell state error from the clipped output gate delta, or that carried unclipped
    input / forget gate deltas into the next step would miss the GPU module's bounds by more than a factor of 10 on every case."""
    case = references(pkg, orc, kind, size, T, mode)
    if mode == "bf16":
        clean = replay(case["inp"], bf16_internals(case), bf16_stand_in(case))
        print("replay of the unmutated stand-in", fmt(clean))
        assert clean["dummy"] == 0 and all(v <= 1.0 for v in clean.values()), fmt(clean)
    for name, switches in sorted(MUTANTS.items()):
        mutated = numpy_reference(case["inp"], case["lay64"], **switches)
        if mode == "bf16":
            mutated["stored_bf16"] = bf16_stand_in(case, **switches)
        q, ratio, ratios = mutant_ratio(case, mutated)
        finite = {k: v for k, v in ratios.items() if np.isfinite(v)}
        print("%s %d T=%d %s: %s moves %s by %.3g bounds (largest finite: %.3g)" % (kind, size, T, mode, name, q, ratio, max(finite.values()) if finite else 0.0))
        assert ratio > 10.0, (name, q, ratio)
