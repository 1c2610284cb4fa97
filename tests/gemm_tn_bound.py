"""Worst-case error bound of the weight-gradient products C = A^T B (fp32 accumulation over K frames) against the float64
product of the same operands, and the numpy models that check it without a device (test_gemm_tn_bound.py); the device test
that relies on it is test_gpu_gemm_tn_group.py::test_random_operands_stay_inside_the_derived_bound.

Derivation.  u = 2^-24 (fp32, round to nearest).  A sum of n fp32 terms formed in ANY order, every addition rounded once,
satisfies |computed - exact| <= gamma(n) * sum |terms| with gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., section 4.2: each term passes through at most n - 1 additions; one more rounding for a term
that is itself a rounded product).  Per output element sum |terms| = (|A|^T |B|)[m][n].

  f32     the fp32 products are rounded once, at most K - 1 additions inside the splits, at most SPLITS more where the
          splits' partials meet (atomics or the fold):  gamma(K + SPLITS) * |A|^T |B|
  bf16    the operands ARE bf16 (compare with the float64 product of bf16_round(A), bf16_round(B)): a product of two 8-bit
          significands is exact in fp32, the additions are the same:  gamma(K + SPLITS) * |A|^T |B| on the rounded operands
  bf16x3  a = ah + al + ra with ah = bf16(a), al = bf16(a - ah); d = 2^-8 is bf16's unit roundoff, so |al| <= d |a| and
          |ra| <= d^2 |a| (b likewise).  a b = (ah bh + al bh + ah bl) + [al bl + ra b + (a - ra) rb]: the kernel keeps the first
          three products -- exact in fp32, 3 K terms of total magnitude <= (1 + d)^2 |a||b| -- and drops the bracket,
          <= (3 d^2 + d^4) |a||b|:  (gamma(3 K + SPLITS) (1 + d)^2 + 3 d^2 + d^4) * |A|^T |B|

SPLITS = 8 (DET_MAX_SPLITS; the small products of the test are cut into at most two).  Nothing here was fitted to what a
kernel returns.

Checked on the CPU at the device test's operands (K = 200 and 208; test_gemm_tn_bound.py asserts both):
  (a) numpy's float32 product of the operands: largest |error| / bound = 0.022 (f32 bound), 0.0033 (bf16x3 bound)
  (b) a bf16x3 model (float64 sum of the kept products) with ONE cross term dropped: 7.8 x (al bh) and 7.4 x (ah bl) the
      bf16x3 bound; with all three kept products it is at 0.025 of it.
The bound grows like K while a lost cross term's error grows like sqrt(K): at K = 344 the margin of (b) is down to 4.4 x,
in the thousands it is gone -- the device test stays at K = 200."""
import numpy as np

U = 2.0 ** -24
D = 2.0 ** -8
SPLITS = 8


def bf16_round(a):
    """round-to-nearest-even to bf16, returned as float32 (what the operand conversion kernel does)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def gamma(n):
    return n * U / (1.0 - n * U)


def bound(prec, A, B):
    """Per-element bound for C = A^T B, A [K][M], B [K][N] (for bf16: the operands as rounded); prec 0 f32, 1 bf16, 2 bf16x3."""
    K = A.shape[0]
    mag = np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64)
    if prec == 2:
        return (gamma(3 * K + SPLITS) * (1 + D) ** 2 + 3 * D * D + D ** 4) * mag
    return gamma(K + SPLITS) * mag


def x3_model(A, B, drop=None):
    """float64 sum of the products the bf16x3 kernels keep; drop = "al_bh" / "ah_bl" leaves that cross term out."""
    ah, bh = bf16_round(A), bf16_round(B)
    al, bl = bf16_round(A - ah), bf16_round(B - bh)
    ah, al, bh, bl = (x.astype(np.float64) for x in (ah, al, bh, bl))
    out = ah.T @ bh
    if drop != "al_bh":
        out = out + al.T @ bh
    if drop != "ah_bl":
        out = out + ah.T @ bl
    return out


# The products of an LSTM layer in miniature (cn_api.cpp, lstm_backward): Hp = 32, two directions, R = 2 * 4 * Hp = 256 delta
# columns, Pp = Lp = 64, PS parallel sequences; the parents hold K + PS frames.
HP, R, PP, LP, PS = 32, 256, 64, 64, 8


def lstm_group_views(K):
    """(name, a_row, a_col, b_row, b_col, M, N, K, B parent) of dWin, dWrec[0] (skipFirstPattern: delta from frame PS, y from
    frame 0) and dWrec[1] (skipLastPattern: y from frame PS; the delta view ENDS PS frames before its parent does)."""
    return [("dWin", 0, 0, 0, 0, R, PP, K + PS, "x"),
            ("dWrec0", PS, 0, 0, 0, 4 * HP, HP, K, "y"),
            ("dWrec1", 0, 4 * HP, PS, HP, 4 * HP, HP, K, "y")]


def lstm_group_parents(rng, K, kind):
    """delta [K + PS][R], x [K + PS][Pp], y [K + PS][Lp]: N(0,1) floats or integers in [-3, 3]."""
    def draw(cols):
        if kind == "randn":
            return rng.randn(K + PS, cols).astype(np.float32)
        return rng.randint(-3, 4, (K + PS, cols)).astype(np.float32)
    return {"delta": draw(R), "x": draw(PP), "y": draw(LP)}


K_BOUND = 200       # frames of the random-operand case (see the module docstring)
