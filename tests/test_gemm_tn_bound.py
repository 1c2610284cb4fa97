"""CPU: the derived bound of gemm_tn_bound.py separates what it must, at the operands of the device test
(test_gpu_gemm_tn_group.py::test_random_operands_stay_inside_the_derived_bound): a plain float32 product stays inside it, a
bf16x3 product that lost one cross term falls outside it by at least 4 x."""
import numpy as np

import gemm_tn_bound as gb


def test_bound_holds_for_fp32_and_exposes_a_lost_cross_term():
    parents = gb.lstm_group_parents(np.random.RandomState(12), gb.K_BOUND, "randn")
    worst = {"f32": 0.0, "f32_vs_x3": 0.0, "x3_kept": 0.0}
    least = {"al_bh": np.inf, "ah_bl": np.inf}
    for name, a_row, a_col, b_row, b_col, M, N, K, bp in gb.lstm_group_views(gb.K_BOUND):
        A = parents["delta"][a_row:a_row + K, a_col:a_col + M]
        B = parents[bp][b_row:b_row + K, b_col:b_col + N]
        ref = A.astype(np.float64).T @ B.astype(np.float64)
        f32 = (A.T @ B).astype(np.float64)
        worst["f32"] = max(worst["f32"], (np.abs(f32 - ref) / gb.bound(0, A, B)).max())
        worst["f32_vs_x3"] = max(worst["f32_vs_x3"], (np.abs(f32 - ref) / gb.bound(2, A, B)).max())
        worst["x3_kept"] = max(worst["x3_kept"], (np.abs(gb.x3_model(A, B) - ref) / gb.bound(2, A, B)).max())
        for drop in least:
            least[drop] = min(least[drop], (np.abs(gb.x3_model(A, B, drop) - ref) / gb.bound(2, A, B)).max())
    print(worst, least)
    assert worst["f32"] < 1 and worst["f32_vs_x3"] < 1 and worst["x3_kept"] < 1, worst
    assert min(least.values()) >= 4, least
