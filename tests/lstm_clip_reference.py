"""numpy float64 restatement of ONE (b)lstm layer's backward pass with the cell's delta clip -- no oracle import.

The rules (csrc/cn_lstm_device.h, comment of lstm_cell_bwd_explicit; the reference's ComputeBlockErrorsFn, LstmLayer.cu:213-286,
and limitedError.cuh:31-34), per unit of a real frame, ' = the step handled before this one (t + 1 in the forward direction,
t - 1 in the backward direction):

    e    = outputErrors + sum over the four gates of W_rec^T delta'          (LstmLayer.cu:936-943, 973-976: STORED deltas)
    dog  = og (1 - og) tanh(c) e                                               (:245)
    ec   = og (1 - tanh(c)^2) e + po dog  +  fg' ec' + pi dig' + pf dfg'       (:262-263: the UNCLIPPED dog; :265-276: the carry
                                                                                takes the STORED, i.e. clipped, dig' and dfg')
    dni  = ig (1 - ni^2) ec,  dfg = fg (1 - fg) c_prev ec (0 at the last call),  dig = ig (1 - ig) ni ec      (:278-280, 248-259)
    stored delta = min(max(delta, -1), 1) for the four gate deltas             (:281-285); ec is stored unclipped
    dummy frames: the four deltas and ec are 0                                 (:219-231)

A dummy frame is one the layer CHECKS and finds without a pattern: t >= t_min, the shortest sequence's length, and pattern type 0
(checkPatType, LstmLayer.cu:949,983).  The frames of an unused slot before t_min are not checked: the reference computes them like
real ones, forward and backward, and so do the kernels; they count as computed here.

and, from the STORED deltas (ComputeWeightUpdateFn, LstmLayer.cu:316-511; :990-1009):

    dW_in[g]  = sum_n delta_g[n] x[n]^T          dbias[g] = bias sum_n delta_g[n]
    dW_rec[g] = sum_t delta_g[t] y[t -+ 1]^T     dpeep_i / dpeep_f = sum_t dig / dfg [t] c[t -+ 1],  dpeep_o = sum_t dog[t] c[t]
    errors to the preceding layer [n] = sum over directions and gates of W_in[g]^T delta_g[n]

Weight layout as tests/test_oracle_autograd.py:lstm_layer: input [4][dirs][H][P], bias [4][dirs][H], recurrent [4][dirs][H][H],
peepholes [3][dirs][H]; gates in the order n, i, f, o.

Three switches state WRONG rules, for the teeth checks of tests/test_lstm_clip_reference.py:
    clip=False               nothing is clipped
    ec_from_clipped_dog=True the output gate's peephole term of ec takes the clipped dog
    carry_unclipped=True     the carry into the next step takes the unclipped dig' and dfg'
and bf16_operands=True states what a CN_PREC_BF16 kernel does with its operands: W_rec rounded to bf16, the deltas stored as bf16 and
read back as such by the next step's product; the carry keeps the unrounded values (registers).

replay_stored_deltas() is the second half: given what a bf16 kernel STORED (its forward internals, its bf16 deltas), it forms in
float64 what every delta must have been and a running bound on the kernel's own fp32 rounding, so that a stored delta is held to
ONE bf16 rounding of the rule's value -- two orders tighter than a comparison with a model that ran its own forward pass.
"""
import numpy as np

GATES = ("ni", "ig", "fg", "og")
SECTIONS = ("input", "bias", "recurrent", "peephole")


def split_weights(w, P, L, bidir):
    dirs = 2 if bidir else 1
    H = L // dirs
    w = np.asarray(w, np.float64)
    a, b, c = 4 * L * P, 4 * L * (P + 1), 4 * L * (P + 1) + 4 * L * H
    return (w[:a].reshape(4, dirs, H, P), w[a:b].reshape(4, dirs, H), w[b:c].reshape(4, dirs, H, H), w[c:].reshape(3, dirs, H))


def split_gradient(g, P, L, bidir):
    """A flat gradient in its four sections (flat arrays): input weights, bias, recurrent weights, peepholes."""
    H = L // (2 if bidir else 1)
    g = np.asarray(g, np.float64)
    a, b, c = 4 * L * P, 4 * L * (P + 1), 4 * L * (P + 1) + 4 * L * H
    return {"input": g[:a], "bias": g[a:b], "recurrent": g[b:c], "peephole": g[c:]}


def computed_frames(pat_types, T, PS, t_min):
    """[T][PS] bool: the frames the layer computes (everything but the checked dummy frames)."""
    pat = np.asarray(pat_types).reshape(T, PS)
    return (pat != 0) | (np.arange(T)[:, None] < t_min)


def bf16_rne(v):
    """float64 array -> the nearest bf16 values (round to nearest even on the fp32 bit pattern), as float64."""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def lstm_backward_clip(internals, weights, pat_types, x, errors, t_min=0, bias=1.0, clip=True, ec_from_clipped_dog=False, carry_unclipped=False,
                       bf16_operands=False):
    """internals: per direction a dict of niActs, igActs, fgActs, ogActs, cellStates, each [T][PS][H]; weights: the flat vector;
    pat_types: [T * PS] and t_min: see computed_frames; x: the layer's input [T][PS][P]; errors: the injected outputErrors [T][PS][L].
    -> dict: `unclipped` and `stored`: per direction {gate: [T][PS][H]}; `cell_errors`: per direction [T][PS][H]; `grad`: the
    four sections (flat, reference layout); `grad_flat`; `prev_errors` [T][PS][P]."""
    dirs = len(internals)
    x = np.asarray(x, np.float64)
    errors = np.asarray(errors, np.float64)
    T, PS, P = x.shape
    L = errors.shape[2]
    H = L // dirs
    Win, _, Wr, Wp = split_weights(weights, P, L, dirs == 2)
    if bf16_operands:
        Wr = bf16_rne(Wr)
    real = computed_frames(pat_types, T, PS, t_min)
    m = real[:, :, None].astype(np.float64)
    lim = (lambda v: np.clip(v, -1.0, 1.0)) if clip else (lambda v: v)

    unclipped, stored, cell_errors = [], [], []
    gin = np.zeros((4, dirs, H, P)); gb = np.zeros((4, dirs, H)); gr = np.zeros((4, dirs, H, H)); gp = np.zeros((3, dirs, H))
    prev_errors = np.zeros((T, PS, P))
    for d in range(dirs):
        a = {k: np.asarray(v, np.float64).reshape(T, PS, H) for k, v in internals[d].items()}
        ni, ig, fg, og, c = a["niActs"], a["igActs"], a["fgActs"], a["ogActs"], a["cellStates"]
        th = np.tanh(c)
        y = th * og * m                                             # the block outputs; dummy frames hold 0 (LstmLayer.cu:78-85)
        pi, pf, po = Wp[0, d], Wp[1, d], Wp[2, d]
        u = {g: np.zeros((T, PS, H)) for g in GATES}
        s = {g: np.zeros((T, PS, H)) for g in GATES}
        sq = {g: np.zeros((T, PS, H)) for g in GATES} if bf16_operands else s      # what the next step's product reads
        ec = np.zeros((T, PS, H))
        order = range(T - 1, -1, -1) if d == 0 else range(T)
        nxt, prv = (1, -1) if d == 0 else (-1, 1)                   # ' = t + nxt; the previous cell state is that of t + prv
        for i, t in enumerate(order):
            e = errors[t, :, d * H:(d + 1) * H].copy()
            first, last = i == 0, i == T - 1
            if not first:
                for k, g in enumerate(GATES):
                    e += sq[g][t + nxt] @ Wr[k, d]                  # e[k] += sum_j W[j][k] delta'[j]
            dog = og[t] * (1 - og[t]) * th[t] * e
            cell = og[t] * (1 - th[t] ** 2) * e + po * (lim(dog) if ec_from_clipped_dog else dog)
            if not first:
                cd = u if carry_unclipped else s
                fgn = np.where(real[t + nxt][:, None], fg[t + nxt], 0.0)           # (a dummy step hands zeros on, whatever its forget gate holds)
                cell += fgn * ec[t + nxt] + pi * cd["ig"][t + nxt] + pf * cd["fg"][t + nxt]
            cell = cell * m[t]
            ec[t] = cell
            u["og"][t] = dog * m[t]
            u["ni"][t] = ig[t] * (1 - ni[t] ** 2) * cell
            u["ig"][t] = ig[t] * (1 - ig[t]) * ni[t] * cell
            u["fg"][t] = 0.0 if last else fg[t] * (1 - fg[t]) * c[t + prv] * cell
            for g in GATES:
                s[g][t] = lim(u[g][t])
                if bf16_operands:
                    sq[g][t] = bf16_rne(s[g][t])
        unclipped.append(u); stored.append(sq); cell_errors.append(ec)
        s = sq                                                      # the gradient products and sums below
        for k, g in enumerate(GATES):
            dl = s[g]
            gin[k, d] = np.einsum("tsh,tsp->hp", dl, x)
            gb[k, d] = bias * dl.sum((0, 1))
            if T > 1:
                if d == 0:
                    gr[k, d] = np.einsum("tsj,tsk->jk", dl[1:], y[:-1])          # skipFirstPattern, LstmLayer.cu:432-435
                else:
                    gr[k, d] = np.einsum("tsj,tsk->jk", dl[:-1], y[1:])          # skipLastPattern, :428-431
            prev_errors += dl @ Win[k, d]
        if T > 1:
            if d == 0:
                gp[0, d] = (s["ig"][1:] * c[:-1]).sum((0, 1)); gp[1, d] = (s["fg"][1:] * c[:-1]).sum((0, 1))
            else:
                gp[0, d] = (s["ig"][:-1] * c[1:]).sum((0, 1)); gp[1, d] = (s["fg"][:-1] * c[1:]).sum((0, 1))
        gp[2, d] = (s["og"] * c).sum((0, 1))
    grad = {"input": gin.reshape(-1), "bias": gb.reshape(-1), "recurrent": gr.reshape(-1), "peephole": gp.reshape(-1)}
    return {"unclipped": unclipped, "stored": stored, "cell_errors": cell_errors, "grad": grad,
            "grad_flat": np.concatenate([grad[k] for k in SECTIONS]), "prev_errors": prev_errors}


U32 = 2.0 ** -24              # unit roundoff of fp32
TH_ABS = 2.0 ** -20           # tanh(c) as the kernels hold it (2 sigmoid(2c) - 1 through v_exp_f32 / v_rcp_f32, 1 ulp each: a few 2^-24 absolute) against np.tanh
BF16_STEP = 2.0 ** -8         # round to nearest of a bf16 significand (8 bits): |bf16(x) - x| <= 2^-8 |x| (2^-9 away from a power of two)


def replay_stored_deltas(internals, weights, pat_types, errors, stored, t_min=0):
    """What a CN_PREC_BF16 backward kernel stored, against the rule applied to ITS OWN inputs.

    internals: the kernel's forward internals per direction (fp32 values), stored: its deltas per direction {gate: [T][PS][H]} (bf16
    values), errors: the injected outputErrors.  Per step, in float64: e from the injected error and the STORED deltas of the step
    before times bf16(W_rec) -- exactly the operands of the kernel's product --, then the rule of this module's header with the
    carry taken from the replay itself.  Beside every value runs a bound on what the kernel's fp32 arithmetic may have made of it:
        e     2 (4 H / 32 + 8) U32 (|err| + sum |delta'| |W|)      a chained sum of 4 H / 32 MFMA chunks seeded with err, each chunk and
                                                                   each link rounding once at the running magnitude, the partners' parts
        tanh  TH_ABS absolute
        ec    |w| err(e) + |e| err(w) + 6 U32 (sum of the terms' magnitudes) + fg' err(ec') + |pi| err(dig') + |pf| err(dfg')
        delta |factor| err(ec) + 4 U32 |delta|      (dog: 0.25 (|e| TH_ABS + |th| err(e)) + 4 U32 |dog|)
    and a stored delta s must satisfy |s - clip(v)| <= BF16_STEP |clip(v)| + (1 + BF16_STEP) err(v): one bf16 rounding of a value
    within the kernel's own noise of the rule's.  Returns {"<direction>/<gate>": largest |s - clip(v)| / bound over the computed
    frames} and, under "dummy", the largest |s| on dummy frames (must be 0)."""
    dirs = len(internals)
    errors = np.asarray(errors, np.float64)
    T, PS, L = errors.shape
    H = L // dirs
    P = (np.asarray(weights).size - L * (4 + 4 * H + 3)) // (4 * L)
    _, _, Wr, Wp = split_weights(weights, P, L, dirs == 2)
    Wr = bf16_rne(Wr)
    real = computed_frames(pat_types, T, PS, t_min)
    m = real[:, :, None].astype(np.float64)
    links = 2.0 * (4 * H / 32.0 + 8) * U32
    out = {"dummy": 0.0}
    for d in range(dirs):
        a = {k: np.asarray(v, np.float64).reshape(T, PS, H) for k, v in internals[d].items()}
        ni, ig, fg, og, c = a["niActs"], a["igActs"], a["fgActs"], a["ogActs"], a["cellStates"]
        S = {g: np.asarray(stored[d][g], np.float64).reshape(T, PS, H) for g in GATES}
        th = np.tanh(c)
        pi, pf, po = Wp[0, d], Wp[1, d], Wp[2, d]
        worst = {g: 0.0 for g in GATES}
        order = range(T - 1, -1, -1) if d == 0 else range(T)
        nxt, prv = (1, -1) if d == 0 else (-1, 1)
        ec_n = err_ec_n = np.zeros((PS, H))
        dlt_n = {g: np.zeros((PS, H)) for g in GATES}
        err_n = {g: np.zeros((PS, H)) for g in GATES}
        fg_n = np.zeros((PS, H))
        for i, t in enumerate(order):
            e = errors[t, :, d * H:(d + 1) * H].copy()
            mag = np.abs(e)
            if i > 0:
                for k, g in enumerate(GATES):
                    e += S[g][t + nxt] @ Wr[k, d]
                    mag += np.abs(S[g][t + nxt]) @ np.abs(Wr[k, d])
            err_e = links * mag
            t2 = og[t] * (1 - og[t]) * th[t]
            w = og[t] * (1 - th[t] ** 2) + po * t2
            err_w = TH_ABS * (2 * np.abs(th[t]) * og[t] + np.abs(po) * 0.25) + 8 * U32 * np.abs(w)
            carry = fg_n * ec_n + pi * dlt_n["ig"] + pf * dlt_n["fg"]
            cell = (e * w + carry) * m[t]
            err_ec = (np.abs(w) * err_e + np.abs(e) * err_w + 6 * U32 * (np.abs(e * w) + np.abs(fg_n * ec_n) + np.abs(pi * dlt_n["ig"]) + np.abs(pf * dlt_n["fg"]))
                      + fg_n * err_ec_n + np.abs(pi) * err_n["ig"] + np.abs(pf) * err_n["fg"]) * m[t]
            factor = {"ni": ig[t] * (1 - ni[t] ** 2), "ig": ig[t] * (1 - ig[t]) * ni[t],
                      "fg": np.zeros((PS, H)) if i == T - 1 else fg[t] * (1 - fg[t]) * c[t + prv]}
            v = {g: f * cell for g, f in factor.items()}
            err_v = {g: np.abs(f) * err_ec + 4 * U32 * np.abs(v[g]) for g, f in factor.items()}
            v["og"] = t2 * e * m[t]
            err_v["og"] = (og[t] * (1 - og[t]) * (np.abs(e) * TH_ABS + np.abs(th[t]) * err_e) + 4 * U32 * np.abs(v["og"])) * m[t]
            for g in GATES:
                cv = np.clip(v[g], -1.0, 1.0)
                bound = BF16_STEP * np.abs(cv) + (1 + BF16_STEP) * err_v[g] + 1e-38
                ratio = np.abs(S[g][t] - cv) / bound
                if real[t].any():
                    worst[g] = max(worst[g], float(ratio[real[t]].max()))
                if (~real[t]).any():
                    out["dummy"] = max(out["dummy"], float(np.abs(S[g][t][~real[t]]).max()))
                dlt_n[g], err_n[g] = cv, err_v[g]
            ec_n, err_ec_n, fg_n = cell, err_ec, fg[t] * m[t]
        for g in GATES:
            out["%d/%s" % (d, g)] = worst[g]
    return out
