"""What decoupled weight decay costs on the headline net (39 -> 3 x blstm 250 -> softmax 183 -> multiclass_classification, PS 50,
T ~ U[250,350], bf16, armed update): the same fractions trained on one device without decay and with it, under momentum and
under Adam.  With decay on the armed update stays overlapped with the backward pass; what changes is the instantiation of the
fused update + operand-copy launch (two more fp32 operations per input / recurrent weight, the same loads and stores).  Prints,
per optimizer and variant, the whole step time and cn_ctx_timing class 4 ("everything else": softmax, loss, re-layout, updates).
The plain net runs before and after: the two plain figures show the run-to-run spread the differences have to be read against.
DESIGN.md section 4.4 records the figures.

    python tools/decay_cost.py [--steps 40] [--warmup 10] [--precision bf16] [--decay 0.01]
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
    ap.add_argument("--decay", type=float, default=0.01)
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

    result = {"precision": args.precision, "steps": args.steps, "decay": args.decay}
    for optimizer in ("sgd", "adam"):
        result[optimizer] = {}
        for label, decay in (("plain", 0.0), ("decay", args.decay), ("plain_again", 0.0)):
            with pkg.NeuralNetwork(layers, None, PS, 350, precision=prec, seed=1) as net:
                net.set_weight_decay(decay)
                count = [0]

                def step(i):
                    count[0] += 1
                    net.load_sequences(fractions[i % n_frac])
                    net.compute_forward_pass()
                    net.loss_accumulate()
                    if optimizer == "adam":
                        net.arm_adam(1e-5, step=count[0])
                        net.compute_backward_pass()
                        net.update_weights_adam(1e-5, step=count[0])
                    else:
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
                # a second pass with the events on: the classes' device time (the events themselves lengthen the step)
                net.timing_enable(True); net.timing_reset()
                for i in range(args.steps):
                    step(i)
                other_ms, launches = net.timing_read()["other"]
                net.timing_enable(False)
                result[optimizer][label] = {"step_ms": round(step_ms, 4), "class4_ms_per_step": round(other_ms / args.steps, 4),
                                            "class4_spans_per_step": launches / args.steps,
                                            "frames_per_sec": round(frames_per_step / step_ms * 1e3), "error_sum": err}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
