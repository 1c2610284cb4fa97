"""-m gpu: the grouped weight-gradient products as the layers launch them (launch_gemm_tn_group through cn_dbg_gemm_tn_group)
and fold_kernel on its own (cn_dbg_fold), held to EXACT sums.

Operands of the exact tests are integers in [-3, 3] drawn per frame (exact in bf16, zero lo half in bf16x3; no two frames
alike), or the unit-impulse A / k-dependent B of test_gemm_tn_big_sees_every_frame_once.  Every product and every fp32 partial
sum is an integer below 2^24, so the order of atomics, splits and folds cannot change a bit and ONE assertion serves bf16, f32,
bf16x3 and both settings of "deterministic": C[:, :N] EQUALS the integer product of the views (float64 BLAS product of integers
below 2^53 = the int64 product, spot-checked against numpy's int64 matmul), C's pitch columns keep their sentinel (-7), and in
the deferred form the workspace keeps the hook's sentinel in its pitch columns and in every slot at split >= the splits used.
Parent rows / columns outside a view hold 64 where the item has a parent of its own ("own" layout); in the "shared" layout the
three products read one delta / x / y parent like a layer, and what lies outside a view is another product's data.  No launch
reads or writes outside a parent: the hook checks every view, the kernels read in-view elements only (the 256 x 256 kernel's
buffer resource may END behind the parent, no load lands there).

Which path a case reaches, and how that is known (dispatch is steered with cn_ctx_set_option only; split counts come back from
the deferred form, flags & 1):

 1 test_lstm_layer_in_miniature      gemm_tn_kernel<.,64,64>, one grouped launch of three products through first_block[]: 8
                                     tiles, K = 344 / 352 -> two splits of 192 + 152 / 160 frames (deferred: [2, 2, 2]); views
                                     with lda = 256 != M, ldb = 64 != N, row offsets PS, one ends PS frames before its parent;
                                     deterministic: per-split stores, fold behind the launch with the layer's bias fold as `extra`
 2 test_partial_tiles_and_short_k    64 x 64 tiles, 96 x 160 (partial last tile row and column), ldc = 192; tn_blocks = 4096;
                                     K = 257 is cut into 192 + 65 (deferred: 2 splits, each partial EQUALS its frames' product),
                                     K <= 256 is not (deferred: 1)
 3 test_ws_splits_cap                tn_blocks = 100000 at K = 2500 asks for 10 splits: atomics take them, the workspace form is
                                     held to 2 <= splits <= DET_MAX_SPLITS and leaves no slot beyond them written
 4 test_huge_product_runs_alone      2080 x 4128 at K = 100 (2145 tiles of 64 x 64 >= 2048): launch_gemm_tn on its own,
                                     gemm_tn_kernel<.,128,128>, 17 x 33 tiles with 32-wide last row and column, one split
                                     (cap_atomic == 0); the two dWrec products still share a 64 x 64 launch
 5 test_degenerate_members           K == 0 / M == 0 items are skipped (C untouched); a group of only such items still runs `extra`
 6 test_ride_along_group             tnbig_group_mink = 4096: 1024 x 448 (K = 4141) and 512 x 192 (K = 4133, column slices at row
                                     offset PS, ldb = 256, B view ends PS frames before its parent) total 557056 >= 2^19 outputs and
                                     go to ONE gemm_tn_big_kernel launch (8 + 2 tiles, 192-wide last tile column, K = 4096 + 45 / 37);
                                     512 x 64 (refused by gemm_tn_big_can) follows on 64 x 64 tiles.  tnbig_blocks = 80 -> 8 splits,
                                     64 and 16 blocks; = 30 -> 3 splits, 24 and 6 blocks (padded to 8) -- deferred: [8, 8, 8] /
                                     [3, 3, 8] (the small path would cut the pair into 4).  Off, on (+ `extra` on the last launch),
                                     deferred; impulse operands once
 7 test_cu_budget_of_one             the same group, cu_budget = 1 < 10 tiles: launch_gemm_tn_big_group hands the pair to the small
                                     tiles (tn_blocks = 272 over 136 tiles -> deferred [2, 2, 8], not tnbig_blocks' 3)
 8 test_cu_budget_cuts_the_splits    cu_budget = 25 (10 tiles < 25 < CUs): 25 / 10 -> 2 splits on the big kernel (8 without a budget)
 9 test_no_big_tn                    no_big_tn = 1: all three on 64 x 64 tiles, same bits as case 6 (both exact; pins the option)
10 test_deferred_partials_add_up     N(0,1) operands, small and big group: the partials added on the host in split order in fp32
                                     EQUAL the non-deferred deterministic result bit for bit, and two such calls equal each other
11 test_fold                         fold_kernel: nparts 1, 3, 4, 5, 9 (four-at-a-time and remainder loops), accumulate, clear,
                                     cols < ld, rows * cols not a multiple of 1024, 5 items in one call (FOLD_MAX = 4: two launches)
12 test_random_operands_stay_inside_the_derived_bound
                                     case 1's group at K = 200 on N(0,1) operands against the float64 product: integers cannot see
                                     a lost bf16x3 cross term.  Bound per element gamma * (|A|^T |B|)[m][n], derived in
                                     gemm_tn_bound.py (fp32 summation constant for K + 8 terms; bf16x3: 3 K + 8 terms plus
                                     3 * 2^-16 for the dropped lo * lo and split-residual terms).  Checked on the CPU at these
                                     operands (test_gemm_tn_bound.py): a float32 numpy product sits at 0.022 of the bound, a bf16x3
                                     model that lost one cross term at 7.4 x to 7.8 x of it.  (On an MI355X the kernels sit at
                                     0.022 (f32), 0.0075 (bf16) and 0.026 (bf16x3) of their bounds, deterministic or not.)

Not reachable from here: a 4 GB operand (gemm_tn_big_can's 32-bit fill offsets).
"""
import ctypes as C
import functools
from contextlib import contextmanager

import numpy as np
import pytest

import gemm_tn_bound as gb

pytestmark = pytest.mark.gpu

OUTSIDE = 64.0          # parent rows / columns outside a view
PITCH = -7.0            # C's pitch columns
PRECS = [0, 1, 2]       # f32, bf16, bf16x3


@pytest.fixture(scope="module")
def lib(pkg):
    from lstm_rnn_amd import binding as B
    return pkg.load_library(), B


@contextmanager
def context(lib, prec, det, **options):
    L, B = lib
    ctx = C.c_void_p(); B.check(L.cn_ctx_create(0, prec, None, C.byref(ctx)))
    try:
        B.check(L.cn_ctx_set_option(ctx, b"deterministic", 1 if det else 0), ctx)
        for name, value in options.items():
            B.check(L.cn_ctx_set_option(ctx, name.encode(), value), ctx)
        yield ctx
    finally:
        L.cn_ctx_destroy(ctx)


class Item:
    """One product: views into host parents, the pitch of its C, and (integers) its exact result."""

    def __init__(self, A, a_row, a_col, B, b_row, b_col, M, N, K, ldc=None):
        self.A, self.B = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)
        self.a_row, self.a_col, self.b_row, self.b_col, self.M, self.N, self.K = a_row, a_col, b_row, b_col, M, N, K
        self.ldc = N if ldc is None else ldc

    def views(self):
        return (self.A[self.a_row:self.a_row + self.K, self.a_col:self.a_col + self.M],
                self.B[self.b_row:self.b_row + self.K, self.b_col:self.b_col + self.N])

    def exact(self, k0=0, k1=None):
        """the integer product of the views' frames k0 .. k1 - 1"""
        Av, Bv = self.views()
        Av, Bv = Av[k0:k1], Bv[k0:k1]
        ref = Av.astype(np.float64).T @ Bv.astype(np.float64)
        assert np.abs(ref).max(initial=0) < 1 << 24
        m, n = min(self.M, 48), min(self.N, 48)
        assert np.array_equal(ref[:m, :n], Av[:, :m].astype(np.int64).T @ Bv[:, :n].astype(np.int64))
        return ref.astype(np.int64)


def own(rng, M, N, K, rows_a, lda, a_row, a_col, rows_b, ldb, b_row, b_col, ldc=None, kind="int"):
    """An item with parents of its own: OUTSIDE everywhere but in the views."""
    A = np.full((rows_a, lda), OUTSIDE, np.float32); Bm = np.full((rows_b, ldb), OUTSIDE, np.float32)
    k = np.arange(K)
    if kind == "int":
        Av = rng.randint(-3, 4, (K, M)); Bv = rng.randint(-3, 4, (K, N))
    elif kind == "impulse":
        Av = np.zeros((K, M)); Av[k, k % M] = 1.0
        Bv = (k[:, None] * 7 + np.arange(N)[None, :] * 3) % 13 - 6
    else:
        Av = rng.randn(K, M); Bv = rng.randn(K, N)
    A[a_row:a_row + K, a_col:a_col + M] = Av; Bm[b_row:b_row + K, b_col:b_col + N] = Bv
    return Item(A, a_row, a_col, Bm, b_row, b_col, M, N, K, ldc)


def lstm_group(K, kind, layout, seed=1):
    """Case 1's three products (gemm_tn_bound.lstm_group_views); ldc: dWin 96, dWrec[0] 32 (= N, as in a layer), dWrec[1] 64."""
    rng = np.random.RandomState(seed)
    ldcs = {"dWin": 96, "dWrec0": 32, "dWrec1": 64}
    views = gb.lstm_group_views(K)
    if layout == "shared":
        p = gb.lstm_group_parents(rng, K, kind)
        return [Item(p["delta"], ar, ac, p[bp], br, bc, M, N, k, ldcs[name]) for name, ar, ac, br, bc, M, N, k, bp in views]
    return [own(rng, M, N, k, K + gb.PS, gb.R, ar, ac, K + gb.PS, gb.LP, br, bc, ldcs[name], kind)
            for name, ar, ac, br, bc, M, N, k, bp in views]


def run_group(lib, ctx, items, cu_budget=0, deferred=False, extra=None):
    """-> (C per item, splits per item).  C: [M][ldc], zero with PITCH in the pitch columns going in; deferred: the workspace
    [DBG_MAX_SPLITS][M][ldc]."""
    L, B = lib
    arr = (B.DbgTnItem * max(1, len(items)))()
    outs = []
    for i, it in enumerate(items):
        if deferred:
            out = np.full((B.DBG_MAX_SPLITS, it.M, it.ldc), np.nan, np.float32)
        else:
            out = np.zeros((it.M, it.ldc), np.float32); out[:, it.N:] = PITCH
        outs.append(out)
        arr[i] = B.DbgTnItem(it.A.ctypes.data, it.A.shape[0], it.A.shape[1], it.B.ctypes.data, it.B.shape[0], it.B.shape[1],
                             it.a_row, it.a_col, it.b_row, it.b_col, it.M, it.N, it.K, out.ctypes.data, it.ldc)
    splits = (C.c_int * 3)(-1, -1, -1)
    B.check(L.cn_dbg_gemm_tn_group(ctx, C.addressof(arr), len(items), cu_budget, 1 if deferred else 0, C.addressof(splits),
                                   C.addressof(extra) if extra is not None else None), ctx)
    return outs, list(splits)[:len(items)]


def check_exact(items, outs, refs=None):
    for i, (it, out) in enumerate(zip(items, outs)):
        ref = it.exact() if refs is None else refs[i]
        assert np.array_equal(out[:, :it.N], ref), (i, np.argwhere(out[:, :it.N] != ref)[:4])
        assert np.all(out[:, it.N:] == PITCH), i


def check_deferred(B, items, outs, splits, refs=None):
    for i, (it, ws, s) in enumerate(zip(items, outs, splits)):
        ref = it.exact() if refs is None else refs[i]
        assert 1 <= s <= B.DBG_MAX_SPLITS, (i, s)
        total = ws[0, :, :it.N].copy()
        for p in ws[1:s]:
            total = total + p[:, :it.N]
        assert np.array_equal(total, ref), (i, s, np.argwhere(total != ref)[:4])
        assert np.all(ws[:s, :, it.N:] == B.DBG_WS_SENTINEL), (i, "pitch columns of the workspace")
        assert np.all(ws[s:] == B.DBG_WS_SENTINEL), (i, s, "a slot beyond the splits used was written")


def fold_item(B, dst, part, stride, nparts, rows, cols, ld, accumulate, clear):
    return B.DbgFoldItem(dst.ctypes.data, part.ctypes.data, stride, nparts, rows, cols, ld, accumulate, clear)


def fold_reference(dst, part, stride, nparts, rows, cols, ld, accumulate):
    """numpy's left-to-right float32 sum ((p0 + p1) + p2) + ..., onto dst when accumulate; pitch columns as they were"""
    want = dst.copy()
    p = [part[s * stride:s * stride + rows * ld].reshape(rows, ld)[:, :cols] for s in range(nparts)]
    t = p[0].copy()
    for q in p[1:]:
        t = t + q
    want[:, :cols] = dst[:, :cols] + t if accumulate else t
    return want


def bias_fold(B, rng, nparts=5):
    """The layer's `extra`: workgroup slots of 7 * dirs * Hp bias / peephole sums added onto dbias, cleared behind the read."""
    slot = 7 * 2 * gb.HP
    dst = rng.randn(1, slot).astype(np.float32); part = rng.randn(nparts * slot).astype(np.float32)
    want = fold_reference(dst, part, slot, nparts, 1, slot, slot, 1)
    return dst, part, fold_item(B, dst, part, slot, nparts, 1, slot, slot, 1, 1), want


# ---- small tiles --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["shared", "own"])
@pytest.mark.parametrize("mode", ["atomics", "det", "deferred"])
@pytest.mark.parametrize("prec", PRECS)
def test_lstm_layer_in_miniature(lib, prec, mode, layout):
    L, B = lib
    items = lstm_group(5 * 64 + 24, "int", layout)
    with context(lib, prec, mode != "atomics") as ctx:
        if mode == "deferred":
            outs, splits = run_group(lib, ctx, items, deferred=True)
            print("splits", splits)
            check_deferred(B, items, outs, splits)
            assert splits == [2, 2, 2]
        else:
            dst, part, extra, want = bias_fold(B, np.random.RandomState(3)) if mode == "det" else (None, None, None, None)
            outs, _ = run_group(lib, ctx, items, extra=extra)
            check_exact(items, outs)
            if extra is not None:
                assert np.array_equal(dst, want) and not part.any()


@pytest.mark.parametrize("K", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("prec", PRECS)
def test_partial_tiles_and_short_k(lib, prec, K):
    L, B = lib
    it = own(np.random.RandomState(K), 96, 160, K, K + 16, 128, 8, 16, K + 16, 192, 0, 32, ldc=192)
    for det in (0, 1):
        with context(lib, prec, det, tn_blocks=4096) as ctx:
            outs, _ = run_group(lib, ctx, [it])
            check_exact([it], outs)
            if det:
                ws, splits = run_group(lib, ctx, [it], deferred=True)
                print("K", K, "splits", splits)
                check_deferred(B, [it], ws, splits)
                assert splits == [2 if K == 257 else 1]
                if K == 257:        # 192 + 65 frames, each split's partial in its own slot
                    assert np.array_equal(ws[0][0, :, :160], it.exact(0, 192)) and np.array_equal(ws[0][1, :, :160], it.exact(192, 257))


@pytest.mark.parametrize("prec", PRECS)
def test_ws_splits_cap(lib, prec):
    L, B = lib
    K = 2500
    it = own(np.random.RandomState(K), 96, 160, K, K + 8, 96, 8, 0, K + 8, 160, 0, 0, ldc=192)
    ref = [it.exact()]
    for det in (0, 1):
        with context(lib, prec, det, tn_blocks=100000) as ctx:
            outs, _ = run_group(lib, ctx, [it])
            check_exact([it], outs, ref)
            if det:
                ws, splits = run_group(lib, ctx, [it], deferred=True)
                print("splits", splits)
                check_deferred(B, [it], ws, splits, ref)
                assert 2 <= splits[0] <= B.DBG_MAX_SPLITS


@functools.lru_cache(maxsize=None)
def huge_group():
    rng = np.random.RandomState(4)
    K = 100
    items = [own(rng, 2080, 4128, K, K + 8, 2080 + 32, 4, 16, K + 8, 4128 + 32, 0, 16, ldc=4128 + 32)] + lstm_group(344, "int", "own")[1:]
    return items, [it.exact() for it in items]


@pytest.mark.parametrize("prec,det", [(1, 0), (1, 1), (0, 0)])
def test_huge_product_runs_alone(lib, prec, det):
    items, refs = huge_group()
    with context(lib, prec, det) as ctx:
        outs, _ = run_group(lib, ctx, items)
        check_exact(items, outs, refs)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("prec", PRECS)
def test_degenerate_members(lib, prec, det):
    L, B = lib
    rng = np.random.RandomState(5)
    live = own(rng, 64, 32, 70, 78, 64, 8, 0, 70, 32, 0, 0, ldc=64)
    no_k = own(rng, 64, 32, 0, 8, 64, 0, 0, 8, 32, 0, 0, ldc=64)
    no_m = own(rng, 0, 32, 70, 70, 64, 0, 0, 70, 32, 0, 0, ldc=64)
    with context(lib, prec, det) as ctx:
        dst, part, extra, want = bias_fold(B, rng)
        outs, _ = run_group(lib, ctx, [no_k, live, no_m], extra=extra)
        check_exact([live], [outs[1]])
        assert not outs[0][:, :32].any() and np.all(outs[0][:, 32:] == PITCH)       # as uploaded
        assert np.array_equal(dst, want) and not part.any()
        dst, part, extra, want = bias_fold(B, rng, nparts=4)
        outs, _ = run_group(lib, ctx, [no_k, no_m], extra=extra)
        assert not outs[0][:, :32].any() and np.all(outs[0][:, 32:] == PITCH)
        assert np.array_equal(dst, want) and not part.any()
        if det:
            _, splits = run_group(lib, ctx, [no_k, live, no_m], deferred=True)
            assert splits[0] == 0 and splits[2] == 0 and splits[1] >= 1


# ---- the 256 x 256 kernel -----------------------------------------------------------------------------------------------

BIG_K, BIG_PS = 4133, 8


@functools.lru_cache(maxsize=None)
def big_group(kind):
    """delta parents [4133 + 8][1024], x parent 448 columns, y parents 256 columns.  The first product reads whole parents (a
    layer's dWin), the other two column slices of parents of their own (dWrec[0]: delta from frame PS, y from frame 0; dWrec[1]
    the other way round)."""
    rng = np.random.RandomState(6)
    rows = BIG_K + BIG_PS
    items = [own(rng, 1024, 448, rows, rows, 1024, 0, 0, rows, 448, 0, 0, ldc=448 + 32, kind=kind),
             own(rng, 512, 192, BIG_K, rows, 1024, BIG_PS, 512, rows, 256, 0, 64, ldc=192, kind=kind),
             own(rng, 512, 64, BIG_K, rows, 1024, 0, 0, rows, 256, BIG_PS, 0, ldc=96, kind=kind)]
    return items, ([it.exact() for it in items] if kind != "randn" else None)


@pytest.mark.parametrize("mode", ["atomics", "det", "deferred"])
@pytest.mark.parametrize("tnbig_blocks", [80, 30])
def test_ride_along_group(lib, tnbig_blocks, mode):
    L, B = lib
    items, refs = big_group("int")
    with context(lib, 1, mode != "atomics", tnbig_group_mink=4096, tnbig_blocks=tnbig_blocks) as ctx:
        if mode == "deferred":
            outs, splits = run_group(lib, ctx, items, deferred=True)
            print("splits", splits)
            check_deferred(B, items, outs, splits, refs)
            assert splits == ([8, 8, 8] if tnbig_blocks == 80 else [3, 3, 8])
        else:
            dst, part, extra, want = bias_fold(B, np.random.RandomState(3)) if mode == "det" else (None, None, None, None)
            outs, _ = run_group(lib, ctx, items, extra=extra)
            check_exact(items, outs, refs)
            if extra is not None:
                assert np.array_equal(dst, want) and not part.any()


def test_ride_along_group_sees_every_frame_once(lib):
    items, refs = big_group("impulse")
    with context(lib, 1, 0, tnbig_group_mink=4096, tnbig_blocks=30) as ctx:
        outs, _ = run_group(lib, ctx, items)
        check_exact(items, outs, refs)


def test_cu_budget_of_one(lib):
    L, B = lib
    items, refs = big_group("int")
    for det in (0, 1):
        with context(lib, 1, det, tnbig_group_mink=4096, tnbig_blocks=30, tn_blocks=272) as ctx:
            outs, _ = run_group(lib, ctx, items, cu_budget=1)
            check_exact(items, outs, refs)
            if det:
                ws, splits = run_group(lib, ctx, items, cu_budget=1, deferred=True)
                print("splits", splits)
                check_deferred(B, items, ws, splits, refs)
                assert splits == [2, 2, 8]


def test_cu_budget_cuts_the_splits(lib):
    L, B = lib
    items, refs = big_group("int")
    for det in (0, 1):
        with context(lib, 1, det, tnbig_group_mink=4096) as ctx:
            outs, _ = run_group(lib, ctx, items, cu_budget=25)
            check_exact(items, outs, refs)
            if det:
                ws, splits = run_group(lib, ctx, items, cu_budget=25, deferred=True)
                _, unbudgeted = run_group(lib, ctx, items, deferred=True)
                print("splits", splits, "without a budget", unbudgeted)
                check_deferred(B, items, ws, splits, refs)
                assert splits[:2] == [2, 2] and unbudgeted[:2] == [8, 8]


def test_no_big_tn(lib):
    L, B = lib
    items, refs = big_group("int")
    got = []
    for off in (0, 1):
        with context(lib, 1, 0, tnbig_group_mink=4096, no_big_tn=off) as ctx:
            outs, _ = run_group(lib, ctx, items)
            check_exact(items, outs, refs)
            got.append(outs)
    for a, b in zip(*got):
        assert a.tobytes() == b.tobytes()


# ---- deferred form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group,prec", [("small", 0), ("small", 1), ("small", 2), ("big", 1)])
def test_deferred_partials_add_up(lib, group, prec):
    L, B = lib
    items = lstm_group(344, "randn", "shared", seed=10) if group == "small" else big_group("randn")[0]
    options = {} if group == "small" else {"tnbig_group_mink": 4096, "tnbig_blocks": 30}
    with context(lib, prec, 1, **options) as ctx:
        first, _ = run_group(lib, ctx, items)
        second, _ = run_group(lib, ctx, items)
        ws, splits = run_group(lib, ctx, items, deferred=True)
    print("splits", splits)
    for it, a, b, w, s in zip(items, first, second, ws, splits):
        assert a.tobytes() == b.tobytes()
        assert s >= 2
        total = w[0].copy()
        for p in w[1:s]:
            total = total + p
        assert total[:, :it.N].tobytes() == a[:, :it.N].tobytes(), np.abs(total[:, :it.N] - a[:, :it.N]).max()
        assert np.all(a[:, it.N:] == PITCH)


# ---- fold_kernel --------------------------------------------------------------------------------------------------------

def make_fold(B, rng, nparts, rows, cols, ld, accumulate, clear):
    stride = rows * ld + 16
    dst = rng.randn(rows, ld).astype(np.float32); part = rng.randn(nparts * stride).astype(np.float32)
    return {"dst": dst, "part": part, "before": part.copy(), "want": fold_reference(dst, part, stride, nparts, rows, cols, ld, accumulate),
            "item": fold_item(B, dst, part, stride, nparts, rows, cols, ld, accumulate, clear),
            "geom": (stride, nparts, rows, cols, ld, clear)}


def check_fold(f):
    stride, nparts, rows, cols, ld, clear = f["geom"]
    assert f["dst"].tobytes() == f["want"].tobytes(), np.argwhere(f["dst"] != f["want"])[:4]
    read = np.zeros(nparts * stride, bool)
    for s in range(nparts):
        read[s * stride:s * stride + rows * ld].reshape(rows, ld)[:, :cols] = True
    assert np.array_equal(f["part"][~read], f["before"][~read])          # pitch columns and the gap between partials
    assert not f["part"][read].any() if clear else np.array_equal(f["part"], f["before"])


@pytest.mark.parametrize("clear", [0, 1])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nparts", [1, 3, 4, 5, 9])
def test_fold(lib, nparts, accumulate, clear):
    L, B = lib
    rng = np.random.RandomState(nparts * 4 + accumulate * 2 + clear)
    # 1050 and 3300 outputs (two and four blocks, the last partly filled), cols < ld; one row as the bias fold
    folds = [make_fold(B, rng, nparts, 7, 150, 160, accumulate, clear), make_fold(B, rng, nparts, 33, 100, 104, accumulate, clear),
             make_fold(B, rng, nparts, 1, 448, 448, accumulate, clear)]
    with context(lib, 0, 1) as ctx:
        for f in folds:
            B.check(L.cn_dbg_fold(ctx, C.addressof(f["item"]), 1), ctx)
            check_fold(f)


def test_fold_five_items_in_one_call(lib):
    L, B = lib
    rng = np.random.RandomState(55)
    folds = [make_fold(B, rng, n, rows, cols, ld, acc, clr)
             for n, rows, cols, ld, acc, clr in [(3, 7, 150, 160, 0, 1), (4, 33, 100, 104, 1, 0), (9, 1, 448, 448, 1, 1), (1, 5, 32, 32, 0, 0), (5, 20, 96, 128, 1, 1)]]
    arr = (B.DbgFoldItem * 5)(*[f["item"] for f in folds])
    with context(lib, 0, 1) as ctx:
        B.check(L.cn_dbg_fold(ctx, C.addressof(arr), 5), ctx)
    for f in folds:
        check_fold(f)


# ---- random operands ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("prec", PRECS)
def test_random_operands_stay_inside_the_derived_bound(lib, prec, det):
    rng = np.random.RandomState(12)
    p = gb.lstm_group_parents(rng, gb.K_BOUND, "randn")
    items = [Item(p["delta"], ar, ac, p[bp], br, bc, M, N, k, N + 32) for name, ar, ac, br, bc, M, N, k, bp in gb.lstm_group_views(gb.K_BOUND)]
    with context(lib, prec, det) as ctx:
        outs, _ = run_group(lib, ctx, items)
    for i, (it, out) in enumerate(zip(items, outs)):
        Av, Bv = it.views()
        if prec == 1:
            Av, Bv = gb.bf16_round(Av), gb.bf16_round(Bv)
        ref = Av.astype(np.float64).T @ Bv.astype(np.float64)
        ratio = np.abs(out[:, :it.N] - ref) / gb.bound(prec, Av, Bv)
        print("prec", prec, "det", det, "item", i, "largest |error| / bound", ratio.max())
        assert ratio.max() < 1, (i, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))
        assert np.all(out[:, it.N:] == PITCH)


# ---- the hook refuses what it cannot run --------------------------------------------------------------------------------

def test_hook_validates_before_it_launches(lib):
    L, B = lib
    rng = np.random.RandomState(9)

    def rc(ctx, items, flags=0, splits=True):
        arr = (B.DbgTnItem * len(items))()
        outs = []
        for i, it in enumerate(items):
            out = np.full((max(it.M, 1), it.ldc), PITCH, np.float32); outs.append(out)
            arr[i] = B.DbgTnItem(it.A.ctypes.data, it.A.shape[0], it.A.shape[1], it.B.ctypes.data, it.B.shape[0], it.B.shape[1],
                                 it.a_row, it.a_col, it.b_row, it.b_col, it.M, it.N, it.K, out.ctypes.data, it.ldc)
        s = (C.c_int * 4)()
        code = L.cn_dbg_gemm_tn_group(ctx, C.addressof(arr), len(items), 0, flags, C.addressof(s) if splits else None, None)
        assert all(np.all(o == PITCH) for o in outs)
        return code

    good = own(rng, 64, 32, 70, 78, 64, 8, 0, 70, 32, 0, 0, ldc=64)
    BAD_ARG, SHAPE = -1, -2
    with context(lib, 1, 0) as ctx:
        assert rc(ctx, [good] * 4) == BAD_ARG and b"0 to 3 items" in L.cn_last_error(ctx)
        assert rc(ctx, [good], flags=1) == BAD_ARG                                               # deferred without "deterministic"
        assert rc(ctx, [good], flags=2) == BAD_ARG
        assert rc(ctx, [Item(good.A, 8, 0, good.B, 0, 0, 48, 32, 70, 64)]) == SHAPE              # M not a multiple of 32
        assert rc(ctx, [Item(good.A, 9, 0, good.B, 0, 0, 64, 32, 70, 64)]) == SHAPE              # A view one row past its parent
        assert rc(ctx, [Item(good.A, 8, 32, good.B, 0, 0, 64, 32, 70, 64)]) == SHAPE             # ... 32 columns
        assert rc(ctx, [Item(good.A, 8, 0, good.B, 1, 0, 64, 32, 70, 64)]) == SHAPE              # B view one row
        assert rc(ctx, [Item(good.A, 8, 0, good.B, 0, 0, 64, 32, 70, 16)]) == SHAPE              # ldc < N
        wide = own(rng, 64, 32, 70, 78, 72, 8, 4, 70, 32, 0, 0, ldc=64)
        assert rc(ctx, [wide]) == SHAPE and b"16-byte" in L.cn_last_error(ctx)                   # bf16: column offset 4 = 8 bytes
        bad_fold = B.DbgFoldItem(good.A.ctypes.data, good.B.ctypes.data, 64, 2, 2, 40, 32, 0, 0)
        assert L.cn_dbg_fold(ctx, C.addressof(bad_fold), 1) == SHAPE                             # cols > ld
    with context(lib, 1, 1) as ctx:
        assert rc(ctx, [good], flags=1, splits=False) == BAD_ARG                                 # deferred without splits_out
