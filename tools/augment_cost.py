"""What input augmentation costs on the headline net (39 -> 3 x blstm 250 -> softmax 183 -> multiclass_classification, PS 50,
T ~ U[250,350], bf16).  Three legs train the same fractions from Python through the prefetched host path the driver uses
(prefetch announced beside the backward pass, armed update): augmentation off, input noise generated on the device
(cn_ctx_set_input_augment), and that noise plus two frequency and two time masks.  The legs are interleaved over --rounds
rounds in one process; per leg the median and the min .. max of the rounds' step times are printed, the device legs also as a
ratio to the `off` leg of the same round, and cn_ctx_timing class 4 ("everything else": softmax, loss, the re-layout, updates).
The fourth leg is the HOST noise of --input_noise_sigma through the C++ driver on a NetCDF file of the same shape, beside
driver runs without noise and with --input_noise_on_device: the step time (wall time of a long run less that of a short one,
per fraction; the driver has no class timers) and the loader thread's time per fraction it packed (the driver's
CN_LOADER_TIME hook).  DESIGN.md section 4.4 records the figures.

    python tools/augment_cost.py [--steps 40] [--warmup 10] [--rounds 5] [--precision bf16] [--sigma 0.6] [--driver_seqs 400] [--driver_epochs 40]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

P, C, PS = 39, 183, 50
LEGS = {"off": None,
        "device_noise": dict(),
        "device_noise_masks": dict(freq_masks=2, freq_width=8, time_masks=2, time_width=40, time_max_permille=200)}


def layers():
    out = [{"name": "input", "type": "input", "size": P}]
    out += [{"name": "blstm_%d" % i, "type": "blstm", "size": 250, "bias": 1.0} for i in range(3)]
    return out + [{"name": "output", "type": "softmax", "size": C, "bias": 1.0}, {"name": "postoutput", "type": "multiclass_classification", "size": C}]


def spread(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def device_legs(pkg, args, result):
    prec = {"bf16": pkg.PREC_BF16, "bf16x3": pkg.PREC_BF16X3, "f32": pkg.PREC_F32}[args.precision]
    rng = np.random.RandomState(0)
    fractions = []
    for _ in range(4):
        lens = np.sort(rng.randint(250, 351, PS))
        fr = pkg.make_fraction([rng.randn(n, P).astype(np.float32) for n in lens], [rng.randint(0, C, n).astype(np.int32) for n in lens], PS)
        for k, t in (("inputs", np.float32), ("patTypes", np.int8), ("targetClasses", np.int32)):      # (a hint is matched by address)
            fr[k] = np.ascontiguousarray(fr[k], t)
        fractions.append(fr)
    result["input_elements_per_fraction"] = int(np.mean([sum(f["seqLengths"]) for f in fractions]) * P)
    nets = {label: pkg.NeuralNetwork(layers(), None, PS, 350, precision=prec, seed=1) for label in LEGS}
    counts = dict.fromkeys(LEGS, 0)

    def settings(label, net, index):
        if LEGS[label] is not None:
            net.set_input_augment(noise_sigma=args.sigma, seed=3, pass_=index, **LEGS[label])

    def run(label, steps):
        net = nets[label]
        settings(label, net, counts[label])
        net.load_sequences(fractions[counts[label] % 4])
        for _ in range(steps):
            i = counts[label] = counts[label] + 1
            net.compute_forward_pass()
            net.loss_accumulate()
            settings(label, net, i)                               # the next fraction's settings, in front of its announcement
            net.prefetch_sequences(fractions[i % 4])
            net.arm_update(1e-5, 0.9)
            net.compute_backward_pass()
            net.update_weights_fused(1e-5, 0.9)
            net.load_sequences(fractions[i % 4])
        net.synchronize()

    try:
        times = {label: [] for label in LEGS}
        for label in LEGS:
            run(label, args.warmup)
        for _ in range(args.rounds):
            for label in LEGS:
                t0 = time.perf_counter()
                run(label, args.steps)
                times[label].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for label in LEGS:
            net = nets[label]
            hits0 = net.prefetch_hits()
            net.timing_enable(True); net.timing_reset()           # (the events themselves lengthen the step)
            run(label, args.steps)
            other_ms, spans = net.timing_read()["other"]
            net.timing_enable(False)
            result[label] = {"step_ms": spread(times[label]), "class4_ms_per_step": round(other_ms / args.steps, 4),
                             "class4_spans_per_step": spans / args.steps, "prefetch_hits_per_step": (net.prefetch_hits() - hits0) / args.steps}
            if label != "off":
                result[label]["ratio_to_off"] = spread([a / b for a, b in zip(times[label], times["off"])])
    finally:
        for net in nets.values():
            net.close()


def driver_leg(args, result):
    from scipy.io import netcdf_file
    rng = np.random.RandomState(0)
    lens = rng.randint(250, 351, args.driver_seqs)
    n = int(lens.sum())
    d = tempfile.mkdtemp()
    nc, net = os.path.join(d, "train.nc"), os.path.join(d, "network.jsn")
    f = netcdf_file(nc, "w")
    f.createDimension("numSeqs", len(lens)); f.createDimension("numTimesteps", n); f.createDimension("inputPattSize", P)
    f.createDimension("numLabels", C); f.createDimension("maxSeqTagLength", 16)
    tags = f.createVariable("seqTags", "c", ("numSeqs", "maxSeqTagLength"))
    for i in range(len(lens)):
        tags[i] = np.array(list(("s%05d" % i).ljust(16, "\0")), "c")
    f.createVariable("seqLengths", "i", ("numSeqs",))[:] = lens.astype(np.int32)
    f.createVariable("targetClasses", "i", ("numTimesteps",))[:] = rng.randint(0, C, n).astype(np.int32)
    f.createVariable("inputs", "f", ("numTimesteps", "inputPattSize"))[:] = rng.randn(n, P).astype(np.float32)
    f.close()
    json.dump({"layers": layers()}, open(net, "w"))
    base = [os.path.join(ROOT, "lstm-rnn_amd", "currennt_hip"), "--train", "true", "--stochastic", "true", "--train_file", nc, "--network", net,
            "--parallel_sequences", str(PS), "--learning_rate", "1e-5", "--momentum", "0.9", "--precision", args.precision,
            "--save_network", os.path.join(d, "trained.jsn"), "--random_seed", "1"]
    fractions = (len(lens) + PS - 1) // PS
    # (the driver's table prints an epoch's duration to 0.1 s: the step time is the wall time of a long run less that of a short
    # one -- reading the file, creating the context and storing the network cancel -- over the epochs between them)
    short, long_ = 2, 2 + args.driver_epochs
    for label, extra in (("driver_off", []), ("driver_host_noise", ["--input_noise_sigma", str(args.sigma)]),
                         ("driver_device_noise", ["--input_noise_sigma", str(args.sigma), "--input_noise_on_device", "true"])):
        wall = {}
        for epochs in (short, long_):
            t0 = time.perf_counter()
            out = subprocess.run(base + extra + ["--max_epochs", str(epochs)], capture_output=True, text=True, timeout=900,
                                 env=dict(os.environ, CN_TEST_HOOKS="1", CN_LOADER_TIME="1"))
            wall[epochs] = time.perf_counter() - t0
            if out.returncode != 0:
                raise RuntimeError(out.stdout[-2000:] + out.stderr[-2000:])
        loader = re.search(r"^Loader: ([\d.]+) ms per fraction \((\d+) fractions\)", out.stdout, re.M)
        result[label] = {"step_ms": round((wall[long_] - wall[short]) * 1e3 / (args.driver_epochs * fractions), 3),
                         "loader_ms_per_fraction": float(loader.group(1)) if loader else None,
                         "fractions_per_epoch": fractions, "epochs": args.driver_epochs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3", "f32"])
    ap.add_argument("--sigma", type=float, default=0.6)
    ap.add_argument("--driver_seqs", type=int, default=400, help="sequences of the driver leg's file (0: skip the leg)")
    ap.add_argument("--driver_epochs", type=int, default=40, help="epochs the driver leg's step time is taken over")
    args = ap.parse_args()
    result = {"precision": args.precision, "steps": args.steps, "rounds": args.rounds, "sigma": args.sigma}
    device_legs(ge.load_package(), args, result)
    if args.driver_seqs > 0:
        driver_leg(args, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
