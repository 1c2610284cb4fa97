"""numpy restatement of include/currennt_hip.h, section Input splicing and frame skipping: the network-rate fraction the library
derives from a source-rate fraction of unspliced patterns.

With L, R = context, K = frame_skip, B = L + R + 1 and P0 the source patterns' width, slot s of the source fraction holds len_s
frames (pattern type not NONE) and owns n_s = ceil(len_s / K) network frames; T' = ceil(T / K), Tmin' = ceil(Tmin / K).  Network
frame (j, s), j < n_s:
    pattern type   FIRST for j = 0, LAST for j = n_s - 1 > 0, NORMAL otherwise
    input column c b = c // P0, f = c % P0, ts = clip(K*j + b - L, 0, len_s - 1): the source's inputs[ts][s][f]
    class / target those of source row K*j
Everything else: NONE, zeros, class -1, zero targets.  Nothing here calls make_fraction: the tests hold the two to each other."""
import numpy as np

NONE, FIRST, NORMAL, LAST = 0, 1, 2, 3


def ceil_div(a, b):
    return -(-int(a) // int(b))


def source_lengths(src):
    """len_s of every slot of a fraction dict"""
    return (np.asarray(src["patTypes"]).reshape(src["T"], src["PS"]) != NONE).sum(axis=0).astype(np.int64)


def gather(x, lens, context=(0, 0), frame_skip=1):
    """[T][PS][P0] source-rate values -> [ceil(T / K)][PS][P0 * B]: the input rule alone, zeros outside the network frames"""
    x = np.asarray(x)
    T, PS, P0 = x.shape
    (L, R), K = context, int(frame_skip)
    out = np.zeros((ceil_div(T, K), PS, P0 * (L + R + 1)), x.dtype)
    for s, n in enumerate(int(v) for v in lens):
        for j in range(ceil_div(n, K)):
            for b in range(L + R + 1):
                ts = min(max(K * j + b - L, 0), n - 1)
                out[j, s, b * P0:(b + 1) * P0] = x[ts, s]
    return out


def network_fraction(src, context=(0, 0), frame_skip=1):
    """src: a fraction dict at source rate, built without context (make_fraction(xs, ts, PS)).  Returns the fraction dict every
    layer behind the re-layout sees, in make_fraction's layout."""
    K = int(frame_skip)
    T, PS = int(src["T"]), int(src["PS"])
    lens = source_lengths(src)
    Tn = ceil_div(T, K)
    pat = np.full((Tn, PS), NONE, np.int8)
    for s, n in enumerate(int(v) for v in lens):
        ns = ceil_div(n, K)
        pat[:ns, s] = NORMAL
        if ns >= 1:
            pat[0, s] = FIRST
        if ns > 1:
            pat[ns - 1, s] = LAST
    real = pat != NONE
    x = gather(np.asarray(src["inputs"], np.float32).reshape(T, PS, -1), lens, context, K)
    out = {"T": Tn, "Tmin": ceil_div(src["Tmin"], K), "PS": PS, "numSeqs": src["numSeqs"],
           "seqLengths": [ceil_div(n, K) for n in src["seqLengths"]],
           "inputs": np.ascontiguousarray(x.reshape(Tn * PS, -1)), "patTypes": np.ascontiguousarray(pat.reshape(Tn * PS))}
    if src.get("labels") is not None:
        out["labels"] = src["labels"]
    if src.get("targetClasses") is not None:
        tc = np.asarray(src["targetClasses"], np.int32).reshape(T, PS)[::K]
        out["targetClasses"] = np.ascontiguousarray(np.where(real, tc, -1).astype(np.int32).reshape(Tn * PS))
    if src.get("targets") is not None:
        tg = np.asarray(src["targets"], np.float32).reshape(T, PS, -1)[::K]
        out["targets"] = np.ascontiguousarray(np.where(real[:, :, None], tg, np.float32(0)).astype(np.float32).reshape(Tn * PS, -1))
    return out
