"""CPU: the localised GEMM comparison of tests/kernel_checks.py (gemm_slices()) is neither too tight nor too loose.

Not too tight: a rounding-only model of the kernels — the float64 reference (gemm_ref64, which carries the store path's intermediate rounding) rounded
to fp32 (the accumulator) and then to the output type — stays at or under HALF the GPU check's tolerance on EVERY row gemm_slices() emits, for every
case of gemm_kloop, gemm_edges and gemm_forms, and every emitted region holds at least 32 values.  What the kernels add to that model is the fp32
summation order; the other half is theirs.

The fp32 tolerance is measured here: the worst row a float32 restatement (float32 matmul of the bf16 inputs, epilogue in float32) reaches against
float64 over all fp32 and TN cases is GEMM_F32_WORST; the GPU checks allow 8 x that.

Not too loose: five planted errors that the whole-matrix relative L2 cannot see fail their slice.  Each is scaled down (x 1/2 per step) until the
whole-matrix figure passes; scale factors found: last K-tile dropped in the partial row tile 1/32, ragged K remainder dropped in the last column tile
1/16, a column of the partial column tile from its neighbour 1/32, the bias one column late in the last column tile 1/64, one tail row stale 1/8."""
import pytest
import torch

import kernel_checks as kc
from kernel_checks import GemmCase, TnCase

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
DEV = torch.device("cpu")
ALL_CASES = kc.GEMM_KLOOP_CASES + kc.GEMM_EDGE_CASES + kc.GEMM_TN_CASES + kc.GEMM_FORMS


def store_of(c):
    from e4t import _C
    rc, k = kc.gemm_kernel(c)
    assert rc == 0, (c, _C.load().e4t_last_error())
    return _C.STORE_NAMES[k.store], k.tail_rows


def rounded(y, c):
    y = y.to(f32)
    return y if kc.gemm_form(c).get("f32") else y.to(bf16)


def tol_of(c):
    return kc.TOL_GEMM_F32 if kc.gemm_form(c).get("f32") else kc.TOL1


def rows_of(c, got, ref):
    return kc.gemm_slices(kc.gemm_tag(c), got, ref, kc.gemm_plan(c), 1 if isinstance(c, TnCase) else c.batch, tol_of(c))


def f32_restatement(c, v):
    """the descriptor's semantics in float32: a float32 matmul of the bf16 inputs, the epilogue in float32, one addition after the other"""
    f = kc.gemm_form(c)
    if isinstance(c, TnCase):
        y = v["a"].float().t() @ v["b"].float()
    else:
        a = torch.cat([v["a"], v["a2"]], dim=1) if c.K1 else v["a"]
        y = torch.cat([a[i * c.M:(i + 1) * c.M].float() @ v["b"][i * c.N:(i + 1) * c.N].float().t() for i in range(c.batch)])
    y = y * f.get("alpha", 1.0)
    if "bias" in v:
        y = y + v["bias"]
    if "residual" in v:
        y = y + v["residual"].float()
    if "c0" in v:
        y = y + v["c0"].float()
    return y


def test_rounding_only_model_stays_under_half_the_tolerance_and_regions_hold_32_values():
    worst, n_rows, small = (0.0, "", 0.0), 0, []
    for i, c in enumerate(ALL_CASES):
        v = kc.gemm_values(c, 5000 + i, DEV)
        store, tail = store_of(c)
        ref = kc.gemm_ref64(c, v, store, tail)
        rows = rows_of(c, rounded(ref, c), ref)
        n_rows += len(rows)
        for label, e, tol in rows:
            if e / tol > worst[0]:
                worst = (e / tol, label, e)
        # the number of values of every emitted region: the same slices of a matrix of ones against zeros count them
        ones = kc.gemm_slices("", torch.ones_like(ref), torch.zeros_like(ref), kc.gemm_plan(c), 1 if isinstance(c, TnCase) else c.batch)
        small += [(kc.gemm_tag(c), label, e) for label, e, _ in ones if e * e * 1e-300 < 32 * (1 - 1e-9)]
    print(f"{len(ALL_CASES)} cases, {n_rows} rows; worst row at {worst[0]:.3f} of its tolerance: {worst[1]} ({worst[2]:.3e})")
    assert not small, small[:5]
    assert worst[0] <= 0.5, worst


def test_the_fp32_tolerance_is_eight_times_the_float32_restatements_worst_row():
    worst = (0.0, "")
    cases = [c for c in ALL_CASES if kc.gemm_form(c).get("f32") and not kc.gemm_form(c).get("gelu")]
    assert len(cases) >= 40 and any(isinstance(c, TnCase) for c in cases)
    for i, c in enumerate(cases):
        v = kc.gemm_values(c, 9000 + i, DEV)
        ref = kc.gemm_ref64(c, v, *store_of(c))
        for label, e, _ in rows_of(c, f32_restatement(c, v), ref):
            if e > worst[0]:
                worst = (e, label)
    print(f"float32 restatement against float64 over {len(cases)} fp32 / TN cases: worst row {worst[0]:.3e} ({worst[1]})")
    # the constant is what is measured here (1.273e-7 with the BLAS this was written on; another build's float32 summation order moves it a little)
    assert kc.GEMM_F32_WORST / 2 <= worst[0] <= kc.GEMM_F32_WORST * 1.25, worst
    assert kc.TOL_GEMM_F32 == min(8 * kc.GEMM_F32_WORST, kc.TOLF * 50) and kc.TOL_GEMM_F32 <= kc.TOLF * 50


# ---- planted errors: each on the rounding-only model's output of a bias + residual case, where bias and residual dilute the product by sqrt(3)
WIDE = GemmCase(616, 152, 136, 64, 1, "bias+res")        # 10 row tiles (the last one 40 rows) x 3 column tiles (the last one 24 columns), K = 2 K-tiles + 8
TAIL = GemmCase(1152 + 17, 320, 144, 160, 1, "bias+res")


def _product(v, ks):
    return v["a"][:, ks].to(f64) @ v["b"][:, ks].to(f64).t()


def _last_k_tile_in_the_partial_row_tile(c, v, y):
    e = torch.zeros_like(y)
    e[c.M // 64 * 64:] = -_product(v, slice(64, c.K))[c.M // 64 * 64:]
    return e, "the last row tile"


def _ragged_k_remainder_in_the_last_column_tile(c, v, y):
    e = torch.zeros_like(y)
    e[:, c.N // 64 * 64:] = -_product(v, slice(c.K // 64 * 64, c.K))[:, c.N // 64 * 64:]
    return e, "the last column tile"


def _a_column_from_its_neighbour(c, v, y):
    e = torch.zeros_like(y)
    n = c.N // 64 * 64 + 5
    e[:, n] = y[:, n + 1] - y[:, n]
    return e, "the last column tile"


def _bias_one_column_late(c, v, y):
    e = torch.zeros_like(y)
    n0 = c.N // 64 * 64
    b = v["bias"].to(f64)
    e[:, n0 + 1:] = b[n0:c.N - 1] - b[n0 + 1:]
    return e, "the last column tile"


def _a_stale_tail_row(c, v, y):
    e = torch.zeros_like(y)
    e[c.M - 3] = y[c.M - 4] - y[c.M - 3]
    return e, "tail rows"


PLANTED = [("last K-tile dropped in the partial row tile", WIDE, _last_k_tile_in_the_partial_row_tile, 1 / 32),
           ("ragged K remainder dropped in the last column tile", WIDE, _ragged_k_remainder_in_the_last_column_tile, 1 / 16),
           ("a column of the partial column tile taken from its neighbour", WIDE, _a_column_from_its_neighbour, 1 / 32),
           ("the bias of column n applied at n + 1 in the last column tile", WIDE, _bias_one_column_late, 1 / 64),
           ("one tail row stale", TAIL, _a_stale_tail_row, 1 / 8)]


@pytest.mark.parametrize("what,c,plant,scale", PLANTED, ids=[p[0] for p in PLANTED])
def test_a_planted_error_the_whole_matrix_figure_misses_fails_its_slice(what, c, plant, scale):
    v = kc.gemm_values(c, 9500, DEV)
    ref = kc.gemm_ref64(c, v, *store_of(c))
    err, where = plant(c, v, ref)
    s = 1.0
    while True:      # the largest power of 1/2 at which the whole-matrix figure passes
        rows = rows_of(c, rounded(ref + s * err, c), ref)
        if rows[0][1] <= rows[0][2]:
            break
        s /= 2
        assert s > 1e-6
    failing = [label for label, e, tol in rows if e > tol]
    print(f"{what}: scale {s} (1/{round(1 / s)}); whole matrix {rows[0][1]:.3e}; failing: {failing}")
    assert s == scale, s
    assert any(where in label for label in failing), (where, rows)


# ---- the guard check itself: a store into C's gap columns or guard rows is seen, a store into C is not
GAP_CASES = [(GemmCase(104, 88, 136, 64, 1, "bare"), kc.GEMM_GUARD), (GemmCase(104, 88, 320, 64, 2, "f32 bare"), kc.GEMM_GUARD),
             (GemmCase(104, 88, 136, 64, 1, "C slice4"), kc.GEMM_GUARD), (GemmCase(104, 88, 136, 64, 1, "C slice4"), 0), (GemmCase(104, 88, 136, 64, 1, "C slice8"), 0),
             (GemmCase(104, 88, 136, 64, 1, "f32"), kc.GEMM_GUARD), (TnCase(200, 168, 152, 1, "C slice"), 0), (TnCase(300, 168, 152, 2, "bf16"), kc.GEMM_GUARD)]


@pytest.mark.parametrize("c,guard", GAP_CASES, ids=[kc.gemm_tag(c) + (" guarded" if g else "") for c, g in GAP_CASES])
def test_sentinels_changed_sees_a_store_into_the_gap_columns_of_c(c, guard):
    ops = kc._GemmOperands(c, kc.gemm_values(c, 9700, DEV), DEV, guard)
    ldc, rows = ops.L["ldc"], ops.C.shape[0]
    assert ldc > c.N and ops.sentinels_changed() == 0 and ops.c_touched() == 0
    full = ops.cbuf[guard:guard + rows].view(ops.out_dt)      # [rows, ldc] in the output type: C and its gap columns
    ops.C.fill_(1.0)                                           # what a correct kernel does: every valid element, nothing else
    assert ops.sentinels_changed() == 0 and ops.c_touched() > 0
    for r, col in ((0, c.N), (rows - 1, ldc - 1), (rows // 2, c.N)):      # the first and the last gap column, first / last / a middle row
        keep = full[r, col].clone()
        full[r, col] = 2.0
        assert ops.sentinels_changed() > 0, (r, col)
        full[r, col] = keep
        assert ops.sentinels_changed() == 0
    if guard:      # the sentinel rows in front of and behind C
        for r in (guard - 1, guard + rows):
            keep = ops.cbuf[r, 0].clone()
            ops.cbuf[r, 0] = 0
            assert ops.sentinels_changed() > 0, r
            ops.cbuf[r, 0] = keep
    assert ops.sentinels_changed() == 0
