"""One rank of tests/test_gpu_noise.py::test_data_parallel_replicas_stay_identical:
python noise_rank.py <rank> <world> <dir>.  The ranks share device 0 through the library's test backend (CN_COMM_BACKEND=ipc),
train on different sequences, hand the SAME (seed, pass) to cn_ctx_set_weight_noise, exchange each layer's gradient behind its
backward pass and complete three armed momentum steps.  Writes <dir>/rank<r>.npz: final weights and deltas, each step's reduced
gradient and the noisy weights each step's backward pass read, all in arena order (layers rounded up to four entries)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge                                   # noqa: E402
from helpers import net_desc, random_sequences, random_weights  # noqa: E402


def main():
    rank, world, d = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    pkg = ge.load_package()
    P, C, PS, T = 5, 4, 3, 12
    layers = net_desc(P, [("blstm", 12), ("lstm", 7), ("feedforward_tanh", 6)], C)
    weights = random_weights(layers, np.random.RandomState(77), 0.3)
    xs, ts = random_sequences(np.random.RandomState(100 + rank), [12, 8, 5], P, C=C)
    frac = pkg.make_fraction(xs, ts, PS)
    idfile = os.path.join(d, "id")
    with pkg.NeuralNetwork(layers, weights, PS, T, precision=pkg.PREC_F32, deterministic=True) as net:
        if rank == 0:
            uid = net.comm_unique_id()
            with open(idfile + ".tmp", "wb") as f:
                f.write(uid)
            os.rename(idfile + ".tmp", idfile)
        else:
            t0 = time.time()
            while not os.path.exists(idfile):
                if time.time() - t0 > 60:
                    raise SystemExit("rank %d: no rendezvous id" % rank)
                time.sleep(0.05)
            uid = open(idfile, "rb").read()
        net.comm_init(uid, rank, world)
        tl = net.trainable_layers()

        def arena(read):
            return np.concatenate([np.pad(read(l), (0, -l.weight_count % 4)) for l in tl])

        grads, noisy = [], []
        for step in range(3):
            net.load_sequences(frac); net.compute_forward_pass()
            net.set_weight_noise(0.1, 4242, step)               # no rank offset: every replica perturbs the same weights the same way
            net.arm_update(1e-2, 0.9)
            net.compute_backward_pass_dp()
            net.update_weights_fused(1e-2, 0.9)
            grads.append(arena(lambda l: l.weight_updates()))
            # (the bias entries of the read-back are the clean weights: identical on every rank as long as the replicas are)
            noisy.append(arena(lambda l: l.noisy_weights()))
        np.savez(os.path.join(d, "rank%d.npz" % rank), w=arena(lambda l: l.weights()),
                 d=arena(lambda l: l._read("weightDeltas", l.weight_count)), g=np.stack(grads), noisy=np.stack(noisy),
                 w0=arena(lambda l: np.concatenate([weights[l.name][k] for k in ("input", "bias", "internal")])),
                 backend=np.array(net.comm_backend()[0]))


if __name__ == "__main__":
    main()
