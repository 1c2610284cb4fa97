"""What splicing on the device costs and what a frame skip saves on the headline net (39 x 11 -> 3 x blstm 250 -> softmax 183 ->
multiclass_classification, PS 50, source T ~ U[250,350], context (5, 5), bf16).  Every leg trains the same source sequences from
Python through the prefetched host path the driver uses (prefetch announced beside the backward pass, armed update):

    host_k1     the fractions spliced on the host (make_fraction(context)), the plain load: the upload carries every frame 11 times
    device_k1   the fractions unspliced, cn_ctx_set_input_splice {5, 5, 1}
    device_k2   ... {5, 5, 2}: every layer runs on every second frame
    device_k3   ... {5, 5, 3}

Each leg runs in a process of its own under `timeout`, one after the other; the first leg that fails ends the run.  Per leg: the
median and min .. max of the rounds' step times, the bytes a fraction uploads, and the cn_ctx_timing classes per step (taken in a
run of their own: the events lengthen the step).  DESIGN.md section 4.4 records the figures.

    python tools/splice_cost.py [--steps 40] [--warmup 10] [--rounds 5] [--precision bf16] [--leg_timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

P0, C, PS, CONTEXT = 39, 183, 50, (5, 5)
LEGS = {"host_k1": (False, 1), "device_k1": (True, 1), "device_k2": (True, 2), "device_k3": (True, 3)}


def layers():
    out = [{"name": "input", "type": "input", "size": P0 * (sum(CONTEXT) + 1)}]
    out += [{"name": "blstm_%d" % i, "type": "blstm", "size": 250, "bias": 1.0} for i in range(3)]
    return out + [{"name": "output", "type": "softmax", "size": C, "bias": 1.0}, {"name": "postoutput", "type": "multiclass_classification", "size": C}]


def spread(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def leg(pkg, args, label):
    on_device, k = LEGS[label]
    prec = {"bf16": pkg.PREC_BF16, "bf16x3": pkg.PREC_BF16X3, "f32": pkg.PREC_F32}[args.precision]
    rng = np.random.RandomState(0)
    fractions = []
    for _ in range(4):
        lens = np.sort(rng.randint(250, 351, PS))
        xs, ts = [rng.randn(n, P0).astype(np.float32) for n in lens], [rng.randint(0, C, n).astype(np.int32) for n in lens]
        fr = pkg.make_fraction(xs, ts, PS) if on_device else pkg.make_fraction(xs, ts, PS, context_left=CONTEXT[0], context_right=CONTEXT[1], frame_skip=k)
        for name, t in (("inputs", np.float32), ("patTypes", np.int8), ("targetClasses", np.int32)):      # (a hint is matched by address)
            fr[name] = np.ascontiguousarray(fr[name], t)
        fractions.append(fr)
    result = {"frame_skip": k, "spliced_on": "device" if on_device else "host",
              "upload_bytes_per_fraction": int(np.mean([f["inputs"].nbytes + f["patTypes"].nbytes + f["targetClasses"].nbytes for f in fractions]))}
    count = [0]
    with pkg.NeuralNetwork(layers(), None, PS, -(-350 // k), precision=prec, seed=1) as net:
        if on_device:
            net.set_input_splice(CONTEXT, k)

        def run(steps):
            net.load_sequences(fractions[count[0] % 4])
            for _ in range(steps):
                count[0] += 1
                net.compute_forward_pass()
                net.loss_accumulate()
                net.prefetch_sequences(fractions[count[0] % 4])
                net.arm_update(1e-5, 0.9)
                net.compute_backward_pass()
                net.update_weights_fused(1e-5, 0.9)
                net.load_sequences(fractions[count[0] % 4])
            net.synchronize()

        run(args.warmup)
        times = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            run(args.steps)
            times.append((time.perf_counter() - t0) * 1e3 / args.steps)
        hits0 = net.prefetch_hits()
        net.timing_enable(True); net.timing_reset()
        run(args.steps)
        classes = net.timing_read()
        net.timing_enable(False)
        result.update(network_steps=net.T, step_ms=spread(times), prefetch_hits_per_step=(net.prefetch_hits() - hits0) / args.steps,
                      class_ms_per_step={name: round(ms / args.steps, 4) for name, (ms, n) in classes.items()})
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3", "f32"])
    ap.add_argument("--leg_timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--leg", choices=sorted(LEGS), help="run this leg alone, in this process")
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(ge.load_package(), args, args.leg)))
        return 0
    result = {"precision": args.precision, "steps": args.steps, "rounds": args.rounds, "context": list(CONTEXT)}
    for label in LEGS:
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", label, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--precision", args.precision]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:          # a leg that failed or ran out of time ends the run: nothing more is started on the device
            sys.stderr.write("leg %s ended with status %d\n%s%s" % (label, out.returncode, out.stdout[-2000:], out.stderr[-2000:]))
            print(json.dumps(result))
            return out.returncode
        result[label] = json.loads(out.stdout.strip().splitlines()[-1])
    for label in ("device_k1", "device_k2", "device_k3"):
        result[label]["ratio_to_host_k1"] = round(result[label]["step_ms"]["median"] / result["host_k1"]["step_ms"]["median"], 4)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
