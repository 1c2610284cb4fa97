"""What context layers cost on the headline net (39 -> 3 x blstm 250 -> softmax 183 -> multiclass_classification, PS 50,
T ~ U[250,350], bf16): the same fractions trained on one device as they are and with a context (1, 1) layer in front of the second
and the third blstm layer -- two gathers in the forward pass, two folds in the backward pass (and input products of the two
followers that are three times as wide: those are the model's, not the kernels').  Prints, per variant, the whole step time and
cn_ctx_timing class 4 ("everything else": softmax, loss, re-layout, updates -- and the context kernels), of a whole step and of the
forward pass alone: the difference of the forward figures is the two gathers (with their length pass), the rest of the step's
difference the two folds.  From the bytes the kernels must move -- gather: one read of the source row and one write of the spliced
row per real frame; fold: one read of the spliced error row and one write of the predecessor's per real frame -- it derives their
GB/s.  The plain net runs before and after: the two plain figures show the run-to-run spread the differences have to be read
against.  DESIGN.md section 4.4 records the figures.

    python tools/context_cost.py [--steps 40] [--warmup 10] [--precision bf16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3", "f32"])
    args = ap.parse_args()
    pkg = ge.load_package()
    prec = {"bf16": pkg.PREC_BF16, "bf16x3": pkg.PREC_BF16X3, "f32": pkg.PREC_F32}[args.precision]
    esz = 2 if args.precision == "bf16" else 4
    rng = np.random.RandomState(0)
    P, C, PS, n_frac, H, B = 39, 183, 50, 4, 250, 3
    fractions = []
    for _ in range(n_frac):
        lens = np.sort(rng.randint(250, 351, PS))
        xs = [rng.randn(n, P).astype(np.float32) for n in lens]
        ts = [rng.randint(0, C, n).astype(np.int32) for n in lens]
        fractions.append(pkg.make_fraction(xs, ts, PS))
    frames_per_step = np.mean([sum(f["seqLengths"]) for f in fractions])

    result = {"precision": args.precision, "steps": args.steps}
    for label, context in (("plain", False), ("context", True), ("plain_again", False)):
        layers = [{"name": "input", "type": "input", "size": P}]
        for i in range(3):
            if context and i > 0:
                layers.append({"name": "context_%d" % i, "type": "context", "size": B * H, "left": 1, "right": 1})
            layers.append({"name": "blstm_%d" % i, "type": "blstm", "size": H, "bias": 1.0})
        layers += [{"name": "output", "type": "softmax", "size": C, "bias": 1.0}, {"name": "postoutput", "type": "multiclass_classification", "size": C}]
        with pkg.NeuralNetwork(layers, None, PS, 350, precision=prec, seed=1) as net:
            def forward(i):
                net.load_sequences(fractions[i % n_frac])
                net.compute_forward_pass()

            def step(i):
                forward(i)
                net.loss_accumulate()
                net.arm_update(1e-5, 0.9)
                net.compute_backward_pass()
                net.update_weights_fused(1e-5, 0.9)
            for i in range(args.warmup):
                step(i)
            net.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(i)
            net.synchronize()
            step_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            err, correct = net.loss_read()
            # further passes with the events on: the classes' device time (the events themselves lengthen the step)
            net.timing_enable(True); net.timing_reset()
            for i in range(args.steps):
                step(i)
            other_ms, launches = net.timing_read()["other"]
            net.timing_reset()
            for i in range(args.steps):
                forward(i)
            fwd_ms, fwd_launches = net.timing_read()["other"]
            net.timing_enable(False)
            result[label] = {"step_ms": round(step_ms, 4), "class4_ms_per_step": round(other_ms / args.steps, 4),
                             "class4_spans_per_step": launches / args.steps, "class4_ms_per_forward": round(fwd_ms / args.steps, 4),
                             "class4_spans_per_forward": fwd_launches / args.steps, "frames_per_sec": round(frames_per_step / step_ms * 1e3),
                             "error_sum": err}
    plain = {k: 0.5 * (result["plain"][k] + result["plain_again"][k]) for k in ("class4_ms_per_step", "class4_ms_per_forward")}
    gather_ms = result["context"]["class4_ms_per_forward"] - plain["class4_ms_per_forward"]
    fold_ms = result["context"]["class4_ms_per_step"] - plain["class4_ms_per_step"] - gather_ms
    gather_bytes = 2 * frames_per_step * (1 + B) * H * esz           # two layers; per real frame: P operands in, B * P out
    fold_bytes = 2 * frames_per_step * (B + 1) * H * 4               # per real frame: B * P floats in, P out
    # (a difference that comes out at or below zero is a disturbed run: no rate then)
    for key, ms, nbytes in (("gathers", gather_ms, gather_bytes), ("folds", fold_ms, fold_bytes)):
        result[key] = {"ms_per_step": round(ms, 4), "bytes": int(nbytes), "GB_per_s": round(nbytes / ms / 1e6, 1) if ms > 0 else None}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
