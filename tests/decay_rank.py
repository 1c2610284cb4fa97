"""One rank of tests/test_gpu_decay.py::test_decay_data_parallel_replicas_stay_identical:
python decay_rank.py <rank> <world> <dir>.  The ranks share device 0 through the library's test backend (CN_COMM_BACKEND=ipc),
train on different sequences, exchange each layer's gradient behind its backward pass and complete three ARMED Adam steps with
weight decay on.  Writes <dir>/rank<r>.npz: initial and final weights, the moments, each step's reduced gradient in arena order
(layers rounded up to four entries), the layers' segments (start, stop, rate) and the mask of the entries that decay."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge                                   # noqa: E402
import decay_reference as DR                                    # noqa: E402
from helpers import net_desc, random_sequences, random_weights  # noqa: E402

LR, OWN_LR, DECAY = 1e-3, 5e-3, 0.1


def main():
    rank, world, d = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    pkg = ge.load_package()
    P, C, PS, T = 13, 9, 4, 12
    layers = net_desc(P, [("blstm", 16), ("feedforward_tanh", 6), ("lstm", 8)], C)
    layers[2]["learningRate"] = OWN_LR
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
        tl = net.trainable_layers()

        def arena(read):
            return np.concatenate([np.pad(read(l), (0, -l.weight_count % 4)) for l in tl])

        segs, ranges, off = [], [], 0
        prev = {b.name: a for a, b in zip(net.layers[:-1], net.layers[1:])}
        for l in tl:
            segs.append((off, off + l.weight_count, l.learning_rate if l.learning_rate >= 0.0 else LR))
            ranges += [(off + a, off + b) for a, b in DR.decayed_ranges(l.type, l.size, prev[l.name].size)]
            off += (l.weight_count + 3) // 4 * 4
        w0 = arena(lambda l: l.weights())
        grads = []
        for step in (1, 2, 3):
            net.load_sequences(frac); net.compute_forward_pass()
            net.arm_adam(LR, step=step)
            net.compute_backward_pass_dp()
            net.update_weights_adam(LR, step=step)
            grads.append(arena(lambda l: l.weight_updates()))
        np.savez(os.path.join(d, "rank%d.npz" % rank), w=arena(lambda l: l.weights()), m=arena(lambda l: l.first_moments()),
                 v=arena(lambda l: l.second_moments()), g=np.stack(grads), w0=w0, segments=np.array(segs, np.float64),
                 mask=DR.decay_mask(off, ranges), decay=np.array(DECAY), backend=np.array(net.comm_backend()[0]))


if __name__ == "__main__":
    main()
