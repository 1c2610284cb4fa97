"""What the CTC post output layer costs on the headline net (39 -> 3 x blstm 250 -> softmax -> post output, PS 50, T ~ U[250,350],
bf16): the same fractions trained twice on one device, once with multiclass_classification on 183 classes and once with ctc on
184 units (183 classes + the blank), labels = the per-frame classes' runs of 5-8 frames collapsed.  Prints, per variant, the
whole step time and cn_ctx_timing class 4 ("everything else": softmax, loss and post output kernels, re-layout, updates), which
is where the CTC launches are counted.  The ctc net runs a second time with option ctc_serial_sweeps (the beta sweep as a launch of
its own behind the alpha sweep): the difference is what running the two sweeps beside each other saves.  DESIGN.md section 4.4
records the figures.

    python tools/ctc_cost.py [--steps 40] [--warmup 10] [--precision bf16]
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
    rng = np.random.RandomState(0)
    P, C, PS, n_frac = 39, 183, 50, 4
    fractions = []
    for _ in range(n_frac):
        lens = np.sort(rng.randint(250, 351, PS))
        xs = [rng.randn(n, P).astype(np.float32) for n in lens]
        labels, ts = [], []
        for n in lens:
            l, frames = [], []
            while len(frames) < n:
                k = int(rng.randint(0, C))
                if l and l[-1] == k:
                    continue                                   # (an adjacent repeat cannot be expressed by per-frame classes)
                l.append(k)
                frames += [k] * int(rng.randint(5, 9))
            frames = frames[:n]
            labels.append([k for i, k in enumerate(frames) if i == 0 or k != frames[i - 1]])
            ts.append(np.asarray(frames, np.int32))
        fractions.append(pkg.make_fraction(xs, ts, PS, labels=labels))
    frames_per_step = np.mean([sum(f["seqLengths"]) for f in fractions])

    result = {"precision": args.precision, "steps": args.steps, "labels_per_sequence": float(np.mean([len(l) for f in fractions for l in f["labels"]]))}
    for post, units, options in (("multiclass_classification", C, {}), ("ctc", C + 1, {}), ("ctc", C + 1, {"ctc_serial_sweeps": 1})):
        layers = [{"name": "input", "type": "input", "size": P}]
        layers += [{"name": "blstm_%d" % i, "type": "blstm", "size": 250, "bias": 1.0} for i in range(3)]
        layers += [{"name": "output", "type": "softmax", "size": units, "bias": 1.0}, {"name": "postoutput", "type": post, "size": units}]
        with pkg.NeuralNetwork(layers, None, PS, 350, precision=prec, seed=1, options=options) as net:
            def step(i):
                net.load_sequences(fractions[i % n_frac])
                net.compute_forward_pass()
                net.loss_accumulate()
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
            err, count = net.loss_read()
            # a second pass with the events on: the classes' device time (the events themselves lengthen the step)
            net.timing_enable(True); net.timing_reset()
            for i in range(args.steps):
                step(i)
            other_ms, launches = net.timing_read()["other"]
            net.timing_enable(False)
            result[post + ("_serial_sweeps" if options else "")] = {"step_ms": round(step_ms, 4), "class4_ms_per_step": round(other_ms / args.steps, 4),
                            "class4_spans_per_step": launches / args.steps, "frames_per_sec": round(frames_per_step / step_ms * 1e3),
                            "error_sum": err, "count": count}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
