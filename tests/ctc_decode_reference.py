"""Float-free model of CTC decoding (include/currennt_hip.h, section CTC decoding; csrc/cn_ctc_decode.hip): best path, collapse,
Levenshtein distance -- the logic of the host function the driver's evaluation passes used before the device took the work
over, and what tests/test_gpu_ctc_decode.py holds the device to, for equality.  numpy only.  Also a writer of transcription .nc
files (the `labels` / `targetStrings` layout of RNNLIB) for the driver tests."""
import numpy as np


def argmax_rows(y):
    """[..., C] -> [...]: the index of the largest value, the LOWEST index of equal ones -- the scan `if y[k] > y[best]: best = k`
    from best = 0, written out so that the tie rule does not rest on a library's."""
    y = np.asarray(y)
    best = np.zeros(y.shape[:-1], np.int64)
    top = y[..., 0].copy()
    for k in range(1, y.shape[-1]):
        better = y[..., k] > top
        best[better] = k
        top = np.where(better, y[..., k], top)
    return best


def best_path(y, length, blank):
    """y [T][C] posteriors of one sequence: the labels of frames 0 .. length-1 whose argmax is not the blank and differs from the
    frame before."""
    k = argmax_rows(np.asarray(y)[:length])
    out, prev = [], -1
    for c in k:
        c = int(c)
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def levenshtein(a, b):
    """Unit costs, one row of the table at a time."""
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        diag, row[0] = row[0], i
        for j in range(1, len(b) + 1):
            subst = diag + (a[i - 1] != b[j - 1])
            diag = row[j]
            row[j] = min(subst, row[j] + 1, row[j - 1] + 1)
    return row[len(b)]


def decode_fraction(y, pat, labels):
    """y [T][PS][C], pat [T][PS] pattern types (a sequence's frames are those with pat != 0, the first len of its slot), labels: one
    sequence per slot or None.  Returns (argmax [T][PS] with -1 outside the sequences, decoded: list of int lists, distances: int
    array, or None without labels)."""
    y, pat = np.asarray(y), np.asarray(pat)
    T, PS, C = y.shape
    k = argmax_rows(y)
    k[pat == 0] = -1
    decoded = [best_path(y[:, s], int((pat[:, s] != 0).sum()), C - 1) for s in range(PS)]
    dist = None if labels is None else np.asarray([levenshtein(decoded[s], labels[s]) for s in range(PS)], np.int64)
    return k, decoded, dist


def write_transcript_nc(path, xs, transcripts, names, prefix="a", ts=None, pad=" "):
    """A transcription file: inputs, seqLengths, seqTags, `labels` (numLabels x maxLabelLength, padded with `pad`) and `targetStrings`
    (one string of label names per sequence, NUL-padded); transcripts: lists of label indices or, verbatim, strings.  ts: per-frame
    target classes to write as `targetClasses` beside them (None: the file has none)."""
    from scipy.io import netcdf_file
    strings = [t if isinstance(t, str) else " ".join(names[k] for k in t) for t in transcripts]
    f = netcdf_file(path, "w")
    n = sum(len(x) for x in xs)
    width = max(len(s) for s in strings) + 1
    lab_w = max(len(s) for s in names) + 1
    f.createDimension("numSeqs", len(xs)); f.createDimension("numTimesteps", n)
    f.createDimension("inputPattSize", xs[0].shape[1]); f.createDimension("numLabels", len(names))
    f.createDimension("maxSeqTagLength", 16); f.createDimension("maxLabelLength", lab_w); f.createDimension("maxTargStringLength", width)
    tags = f.createVariable("seqTags", "c", ("numSeqs", "maxSeqTagLength"))
    for i in range(len(xs)):
        tags[i] = np.array(list(("%s%03d" % (prefix, i)).ljust(16, "\0")), "c")
    lab = f.createVariable("labels", "c", ("numLabels", "maxLabelLength"))
    for i, s in enumerate(names):
        lab[i] = np.array(list(s.ljust(lab_w, pad)), "c")
    tstr = f.createVariable("targetStrings", "c", ("numSeqs", "maxTargStringLength"))
    for i, s in enumerate(strings):
        tstr[i] = np.array(list(s.ljust(width, "\0")), "c")
    v = f.createVariable("seqLengths", "i", ("numSeqs",)); v[:] = np.array([len(x) for x in xs], np.int32)
    if ts is not None:
        v = f.createVariable("targetClasses", "i", ("numTimesteps",)); v[:] = np.concatenate(ts).astype(np.int32)
    v = f.createVariable("inputs", "f", ("numTimesteps", "inputPattSize")); v[:] = np.concatenate(xs).astype(np.float32)
    f.close()
