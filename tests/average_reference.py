"""The averaging step of include/currennt_hip.h (cn_ctx_average_weights) restated in numpy, operation by operation, and the
driver's warm-up rule (--weight_average_warmup).

With dtype float32 every numpy operation below is one IEEE operation rounded to nearest, which is what the device code is held
to (no contraction, denormals kept), so the library's average must EQUAL this bit for bit.  With dtype float64 the same
recurrence is the yardstick of tests/test_average_reference.py."""
import numpy as np


def one_minus_decay(decay, dtype=np.float32):
    """omd: formed in double from the decay as `dtype` holds it, rounded once to `dtype`."""
    return dtype(1.0 - float(dtype(decay)))


def average_step(avg, w, decay, dtype=np.float32):
    """One step; returns the new average.  omd == 1 is an exact copy of w (avg + (w - avg) is not w in floating point)."""
    omd = one_minus_decay(decay, dtype)
    avg, w = np.asarray(avg, dtype), np.asarray(w, dtype)
    if omd == dtype(1.0):
        return w.copy()
    out = avg + omd * (w - avg)
    assert out.dtype == dtype
    return out


def warmup_decay(D, k):
    """The decay of the driver's averaging step k (from 1) under --weight_average_warmup true: D, and for k >= 2
    min(D, k / (k + 9)), formed in double from the float D and rounded once to float."""
    D = float(np.float32(D))
    if k >= 2:
        D = min(D, k / (k + 9.0))
    return np.float32(D)
