"""What CTC decoding on the device costs on the headline net with a ctc output (39 -> 3 x blstm 250 -> softmax 184 -> ctc, PS 50,
T ~ U[250,350], bf16; the fractions of tools/ctc_cost.py, labels of 5-8 frames each):

  a) ms per training step without and with cn_ctc_decode_accumulate behind each forward pass (what --ctc_train_label_errors adds),
     on the same build and the same fractions;
  b) ms per evaluated fraction (load, forward pass, cn_loss_accumulate, decoding) with decoding on the device against the method
     it replaced: outputs() read back per fraction and decoded on the host.  The host decoder here is the reference function of
     tests/ctc_decode_reference.py, Python loops where the driver had C++ ones, so the read-back alone (no decoding) is reported
     beside it as the floor of that method;
  c) the argmax launch alone (option ctc_decode_argmax_only): microseconds per launch and GB/s over the real rows' bytes.

DESIGN.md section 4.4 records the figures.

    python tools/ctc_decode_cost.py [--steps 40] [--warmup 10] [--precision bf16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from ctc_decode_reference import decode_fraction  # noqa: E402


def headline_fractions(pkg, rng, P, C, PS, n_frac):
    fractions = []
    for _ in range(n_frac):
        lens = np.sort(rng.randint(250, 351, PS))
        xs = [rng.randn(n, P).astype(np.float32) for n in lens]
        labels = []
        for n in lens:
            l, frames = [], 0
            while frames < n:
                l.append(int(rng.randint(0, C)))
                frames += int(rng.randint(5, 9))
            labels.append(l)
        fractions.append(pkg.make_fraction(xs, None, PS, labels=labels))
    return fractions


def timed(net, fn, warmup, steps):
    for i in range(warmup):
        fn(i)
    net.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    net.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


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
    fractions = headline_fractions(pkg, rng, P, C, PS, n_frac)
    layers = [{"name": "input", "type": "input", "size": P}]
    layers += [{"name": "blstm_%d" % i, "type": "blstm", "size": 250, "bias": 1.0} for i in range(3)]
    layers += [{"name": "output", "type": "softmax", "size": C + 1, "bias": 1.0}, {"name": "postoutput", "type": "ctc", "size": C + 1}]
    result = {"precision": args.precision, "steps": args.steps,
              "labels_per_sequence": float(np.mean([len(l) for f in fractions for l in f["labels"]]))}
    with pkg.NeuralNetwork(layers, None, PS, 350, precision=prec, seed=1) as net:
        def train(decode):
            def step(i):
                net.load_sequences(fractions[i % n_frac])
                net.compute_forward_pass()
                net.loss_accumulate()
                if decode:
                    net.ctc_decode_accumulate()
                net.compute_backward_pass()
                net.update_weights_fused(1e-5, 0.9)
            return step
        # a) interleaved: plain, decoding, plain, decoding
        a = {"plain": [], "decoding": []}
        for _ in range(2):
            a["plain"].append(timed(net, train(False), args.warmup, args.steps))
            a["decoding"].append(timed(net, train(True), args.warmup, args.steps))
        net.loss_read(); errors, labels = net.ctc_decode_stats()
        result["train_step_ms"] = {k: [round(v, 4) for v in vs] for k, vs in a.items()}
        result["train_label_error_rate"] = errors / max(labels, 1)

        # b) an evaluated fraction
        def eval_device(i):
            net.load_sequences(fractions[i % n_frac]); net.compute_forward_pass(); net.loss_accumulate(); net.ctc_decode_accumulate()

        def eval_copy(i):
            net.load_sequences(fractions[i % n_frac]); net.compute_forward_pass(); net.loss_accumulate()
            return net.outputs()

        host = {"errors": 0, "labels": 0}

        def eval_host(i):
            f = fractions[i % n_frac]
            y = eval_copy(i)
            dist = decode_fraction(y, f["patTypes"].reshape(y.shape[0], PS), f["labels"])[2]
            host["errors"] += int(dist.sum()); host["labels"] += sum(len(l) for l in f["labels"])

        net.ctc_decode_stats()
        dev_ms = timed(net, eval_device, 4, n_frac * 4)
        dev = net.ctc_decode_stats()
        copy_ms = timed(net, eval_copy, 4, n_frac * 4)
        host_ms = timed(net, eval_host, 0, n_frac)
        net.loss_read()
        result["eval_fraction_ms"] = {"device": round(dev_ms, 4), "read_back_only": round(copy_ms, 4), "read_back_and_host_decode": round(host_ms, 3)}
        # the same fractions scored both ways: (4 + 16) / 4 device rounds over the set against one host round
        result["eval_agree"] = dev[0] * n_frac == host["errors"] * (4 + n_frac * 4) and dev[1] * n_frac == host["labels"] * (4 + n_frac * 4)

        # c) the argmax launch alone, back to back on one forward pass
        f = fractions[0]
        net.load_sequences(f); net.compute_forward_pass()
        net.set_option("ctc_decode_argmax_only", 1)
        reps = 200
        us = timed(net, lambda i: net.ctc_decode_accumulate(), 20, reps) * 1e3
        net.set_option("ctc_decode_argmax_only", 0)
        real_rows = int(sum(f["seqLengths"]))
        row_bytes = -(-(C + 1) // 32) * 32 * 4
        result["argmax"] = {"us_per_launch": round(us, 2), "real_rows": real_rows, "bytes": real_rows * row_bytes,
                            "GB_per_s": round(real_rows * row_bytes / (us * 1e-6) / 1e9, 1)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
