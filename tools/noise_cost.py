"""What weight noise costs on the headline net (39 -> 3 x blstm 250 -> softmax 183 -> multiclass_classification, PS 50,
T ~ U[250,350], bf16): the same fractions trained on one device clean (armed update), with noise drawn on the HOST -- the
driver's protocol without --weight_noise_on_device: every layer's weights read back, one std::normal-like sample per weight
(numpy's generator here), the noisy vectors uploaded through set_weights, backward pass, join, clean vectors uploaded again, update
not armed -- and with noise generated on the DEVICE (cn_ctx_set_weight_noise, armed update).  Prints, per variant, the whole step
time and cn_ctx_timing class 4 ("everything else": softmax, loss, re-layout, updates, operand copies -- and the noisy copies).
The clean net runs before and after: the two clean figures show the run-to-run spread the differences have to be read against.
DESIGN.md section 4.4 records the figures.

    python tools/noise_cost.py [--steps 40] [--warmup 10] [--precision bf16] [--sigma 0.01]
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
    ap.add_argument("--sigma", type=float, default=0.01)
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

    result = {"precision": args.precision, "steps": args.steps, "sigma": args.sigma}
    for label in ("clean", "host_noise", "device_noise", "device_noise_ahead", "clean_again"):
        # device_noise_ahead: option noise_ahead -- the noisy copies are generated on the side stream beside the forward pass
        # (the key is set in front of it) instead of on the main stream in front of the first backward kernel
        with pkg.NeuralNetwork(layers, None, PS, 350, precision=prec, seed=1,
                               options={"noise_ahead": 1} if label == "device_noise_ahead" else None) as net:
            host_rng = np.random.RandomState(3)
            tl = net.trainable_layers()
            count = [0]
            result.setdefault("weights", sum(l.weight_count for l in tl))

            def step(i):
                count[0] += 1
                if label.startswith("device_noise"):
                    net.set_weight_noise(args.sigma, 3, count[0])
                net.load_sequences(fractions[i % n_frac])
                net.compute_forward_pass()
                net.loss_accumulate()
                if label == "host_noise":
                    clean = [l.weights() for l in tl]
                    for l, w in zip(tl, clean):
                        l.set_weights(w + host_rng.normal(0.0, args.sigma, w.size).astype(np.float32))
                    net.compute_backward_pass()
                    net.join()
                    for l, w in zip(tl, clean):
                        l.set_weights(w)
                    net.update_weights(1e-5, 0.9)
                    return
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
            result[label] = {"step_ms": round(step_ms, 4), "class4_ms_per_step": round(other_ms / args.steps, 4),
                             "class4_spans_per_step": launches / args.steps, "frames_per_sec": round(frames_per_step / step_ms * 1e3),
                             "error_sum": err}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
