"""What a pyramid costs and buys on the headline net (39 -> 3 x blstm 250 -> softmax 183 -> multiclass_classification, PS 50,
T ~ U[250,350], bf16): the same fractions trained on one device by three nets in ONE process, in turn, round after round --

    plain       the headline net as it is
    pyramid_1   context(0, 1, x1, /2) in front of the second blstm: the second and third blstm, the softmax layer and the loss run
                on half the steps (the second blstm's input products are twice as wide: that is the model's, not the kernels')
    pyramid_2   the same in front of the second and of the third blstm: the third runs on a quarter of the steps

Per variant: the median step time over the rounds, cn_ctx_timing's device time per class and step (with the events on: the events
themselves lengthen a step, so the classes are read against each other, not against the step time), and for the pyramids the
GB/s of the new launches -- class "other" of a whole step minus the plain net's, over the bytes the gathers and folds must move
(gather: B * P operands in and out per frame it writes; fold: B * P floats in per frame of its own axis and P floats out per
frame of the parent's).  The plain net's "other" holds the softmax and loss kernels at full rate, the pyramids' at the reduced
one, so the difference UNDERSTATES the new launches' time where it is positive at all; a figure at or below zero is printed as
null.  DESIGN.md section 4.4 records the figures.

    python tools/stride_cost.py [--steps 20] [--warmup 5] [--rounds 3] [--precision bf16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

P, C, PS, N_FRAC, H = 39, 183, 50, 4, 250
VARIANTS = (("plain", ()), ("pyramid_1", (1,)), ("pyramid_2", (1, 2)))


def layers_of(strided):
    layers = [{"name": "input", "type": "input", "size": P}]
    for i in range(3):
        if i in strided:
            layers.append({"name": "pyramid_%d" % i, "type": "context", "size": 2 * H, "left": 0, "right": 1, "dilation": 1, "stride": 2})
        layers.append({"name": "blstm_%d" % i, "type": "blstm", "size": H, "bias": 1.0})
    return layers + [{"name": "output", "type": "softmax", "size": C, "bias": 1.0}, {"name": "postoutput", "type": "multiclass_classification", "size": C}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3", "f32"])
    args = ap.parse_args()
    pkg = ge.load_package()
    prec = {"bf16": pkg.PREC_BF16, "bf16x3": pkg.PREC_BF16X3, "f32": pkg.PREC_F32}[args.precision]
    esz = 2 if args.precision == "bf16" else 4
    rng = np.random.RandomState(0)
    fractions = []
    for _ in range(N_FRAC):
        lens = np.sort(rng.randint(250, 351, PS))
        xs = [rng.randn(n, P).astype(np.float32) for n in lens]
        ts = [rng.randint(0, C, n).astype(np.int32) for n in lens]
        fractions.append(pkg.make_fraction(xs, ts, PS))
    frames = float(np.mean([sum(f["seqLengths"]) for f in fractions]))          # real frames per step at the input's rate

    nets = {name: pkg.NeuralNetwork(layers_of(strided), None, PS, 350, precision=prec, seed=1) for name, strided in VARIANTS}

    def step(net, i):
        net.load_sequences(fractions[i % N_FRAC])
        net.compute_forward_pass()
        net.loss_accumulate()
        net.arm_update(1e-5, 0.9)
        net.compute_backward_pass()
        net.update_weights_fused(1e-5, 0.9)

    try:
        for name, _ in VARIANTS:
            for i in range(args.warmup):
                step(nets[name], i)
            nets[name].synchronize()
        times = {name: [] for name, _ in VARIANTS}
        for _ in range(args.rounds):                                            # the variants in turn: drift hits all alike
            for name, _ in VARIANTS:
                net = nets[name]
                t0 = time.perf_counter()
                for i in range(args.steps):
                    step(net, i)
                net.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        result = {"precision": args.precision, "steps": args.steps, "rounds": args.rounds, "frames_per_step": frames}
        for name, strided in VARIANTS:
            net = nets[name]
            net.loss_read()
            net.timing_enable(True); net.timing_reset()
            for i in range(args.steps):
                step(net, i)
            classes = {k: round(ms / args.steps, 4) for k, (ms, n) in net.timing_read().items()}
            net.timing_enable(False)
            result[name] = {"step_ms": round(float(np.median(times[name])), 4), "step_ms_rounds": [round(t, 4) for t in times[name]],
                            "class_ms_per_step": classes, "output_rate": net.output_layer().rate}
        for name, strided in VARIANTS[1:]:
            # frames each new layer writes: half the frames of its parent axis (ceil per sequence: about half)
            nbytes, parent = 0.0, frames
            for _ in strided:
                own = parent / 2
                nbytes += own * (2 * 2 * H) * esz                   # gather: B * P operands in, B * P out per frame written
                nbytes += own * (2 * H) * 4 + parent * H * 4        # fold: B * P floats in per own frame, P floats out per parent frame
                parent = own
            ms = result[name]["class_ms_per_step"]["other"] - result["plain"]["class_ms_per_step"]["other"]
            result[name]["new_launches"] = {"other_minus_plain_ms": round(ms, 4), "bytes": int(nbytes),
                                            "GB_per_s": round(nbytes / ms / 1e6, 1) if ms > 0 else None}
            result[name]["speedup"] = round(result["plain"]["step_ms"] / result[name]["step_ms"], 3)
        print(json.dumps(result))
    finally:
        for net in nets.values():
            net.close()


if __name__ == "__main__":
    main()
