"""One rank of tests/test_gpu_lamb.py::test_lamb_data_parallel_replicas_stay_identical:
python lamb_rank.py <rank> <world> <dir>.  The ranks share device 0 through the library's test backend (CN_COMM_BACKEND=ipc),
train on different sequences, exchange each layer's gradient behind its backward pass and apply the armed LAMB step behind the
exchange (the completing call applies it).  Writes <dir>/rank<r>.npz: the initial and final weights, both moments, every step's
summed gradient -- all in arena order, each layer padded to a multiple of four by zeros -- and the layers' records."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge                                   # noqa: E402
from helpers import net_desc, random_sequences, random_weights  # noqa: E402

P, C, PS, T = 13, 9, 3, 8
LR, OWN_LR, DECAY = 1e-3, 5e-3, 0.01


def network():
    layers = net_desc(P, [("blstm", 16), ("feedforward_tanh", 6), ("lstm", 8)], C)
    layers[2]["learningRate"] = OWN_LR
    return layers


def arena(net, read):
    parts = []
    for l in net.trainable_layers():
        x = np.zeros((l.weight_count + 3) // 4 * 4, np.float32)
        x[:l.weight_count] = read(l)
        parts.append(x)
    return np.concatenate(parts)


def main():
    rank, world, d = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    pkg = ge.load_package()
    layers = network()
    weights = random_weights(layers, np.random.RandomState(5), 0.2)
    rng = np.random.RandomState(100 + rank)
    xs, ts = random_sequences(rng, [T - (i % 3) for i in range(PS)], P, C=C)
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
        net.set_weight_decay(DECAY)
        w0 = arena(net, lambda l: l.weights())
        summed = []
        for step in (1, 2, 3):
            net.load_sequences(frac); net.compute_forward_pass()
            net.arm_lamb(LR, step=step)
            net.compute_backward_pass_dp()
            net.update_weights_lamb(LR, step=step)
            summed.append(arena(net, lambda l: l.weight_updates()))
        np.savez(os.path.join(d, "rank%d.npz" % rank), w=arena(net, lambda l: l.weights()), m=arena(net, lambda l: l.first_moments()),
                 v=arena(net, lambda l: l.second_moments()), g=np.stack(summed), w0=w0,
                 rec=np.asarray([l.trust_ratio() for l in net.trainable_layers()], np.float32),
                 backend=np.array(net.comm_backend()[0]))


if __name__ == "__main__":
    main()
