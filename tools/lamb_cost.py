"""What LAMB costs on the headline net (39 -> 3 x blstm 250 -> softmax 183 -> multiclass_classification, PS 50, T ~ U[250,350],
bf16, armed update): the same fractions trained on one device with Adam and with LAMB on the same build.  Adam's armed step runs
layer by layer behind each layer's gradient, fused into the operand-copy launch; LAMB's is deferred to the completing call (the
direction pass writes a layer's moments before the layer's ratio is known), which launches the direction kernel, the apply kernel
and then the plain operand-copy launch on the tail of the step.  Prints, per optimizer, the whole step time and cn_ctx_timing class
4 ("everything else": softmax, loss, re-layout, updates); Adam runs before and after, and the two Adam figures show the run-to-run
spread the difference has to be read against.  Then the update call alone, behind a finished backward pass: the median host time
of a synchronised cn_adam_update_all (one fused launch) and of a synchronised cn_lamb_update_all (direction, apply, operand
copies); the difference is what the two new launches add.  DESIGN.md section 4.4 records the figures.

    python tools/lamb_cost.py [--steps 40] [--warmup 10] [--precision bf16] [--calls 200]
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
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    pkg = ge.load_package()
    prec = {"bf16": pkg.PREC_BF16, "bf16x3": pkg.PREC_BF16X3, "f32": pkg.PREC_F32}[args.precision]
    rng = np.random.RandomState(0)
    P, C, PS, n_frac = 39, 183, 50, 4
    fractions = []
    for _ in range(n_frac):
        lens = np.sort(rng.randint(250, 351, PS))
        xs = [rng.randn(n, P).astype(np.float32) for n in lens]
        ts = [rng.randint(0, C, n).astype(np.int32) for n in lens]
        fractions.append(pkg.make_fraction(xs, ts, PS))
    frames_per_step = np.mean([sum(f["seqLengths"]) for f in fractions])
    layers = [{"name": "input", "type": "input", "size": P}]
    layers += [{"name": "blstm_%d" % i, "type": "blstm", "size": 250, "bias": 1.0} for i in range(3)]
    layers += [{"name": "output", "type": "softmax", "size": C, "bias": 1.0}, {"name": "postoutput", "type": "multiclass_classification", "size": C}]

    result = {"precision": args.precision, "steps": args.steps, "calls": args.calls}
    for label, optimizer in (("adam", "adam"), ("lamb", "lamb"), ("adam_again", "adam")):
        with pkg.NeuralNetwork(layers, None, PS, 350, precision=prec, seed=1) as net:
            arm, update = (net.arm_adam, net.update_weights_adam) if optimizer == "adam" else (net.arm_lamb, net.update_weights_lamb)
            count = [0]

            def step(i):
                count[0] += 1
                net.load_sequences(fractions[i % n_frac])
                net.compute_forward_pass()
                net.loss_accumulate()
                arm(1e-5, step=count[0])
                net.compute_backward_pass()
                update(1e-5, step=count[0])
            for i in range(args.warmup):
                step(i)
            net.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(i)
            net.synchronize()
            step_ms = (time.perf_counter() - t0) * 1e3 / args.steps
            err, correct = net.loss_read()
            # a second pass with the events on: the classes' device time (the events themselves lengthen the step)
            net.timing_enable(True); net.timing_reset()
            for i in range(args.steps):
                step(i)
            other_ms, launches = net.timing_read()["other"]
            net.timing_enable(False)
            # the update call alone, on the gradient the last backward pass left
            net.synchronize()
            times = []
            for k in range(args.calls):
                count[0] += 1
                t0 = time.perf_counter()
                update(1e-5, step=count[0])
                net.synchronize()
                times.append((time.perf_counter() - t0) * 1e6)
            entry = {"step_ms": round(step_ms, 4), "class4_ms_per_step": round(other_ms / args.steps, 4),
                     "class4_spans_per_step": launches / args.steps, "frames_per_sec": round(frames_per_step / step_ms * 1e3),
                     "error_sum": err, "update_call_us_median": round(float(np.median(times)), 2),
                     "update_call_us_min": round(float(np.min(times)), 2)}
            if optimizer == "lamb":
                entry["trust_ratios"] = {l.name: [float(x) for x in l.trust_ratio()] for l in net.trainable_layers()}
            result[label] = entry
    adam_us = 0.5 * (result["adam"]["update_call_us_median"] + result["adam_again"]["update_call_us_median"])
    result["two_new_launches_us"] = round(result["lamb"]["update_call_us_median"] - adam_us, 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
