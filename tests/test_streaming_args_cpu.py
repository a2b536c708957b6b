"""CPU: what the activation, layout and pooling entry points of elementwise.hip refuse.  Every call below fails validation on the host, before any
launch, so the dummy pointer is never dereferenced and no GPU is needed (the pattern of test_norm_args_cpu.py); each refusal is -22 with the words
that name it.  Among them the checks that went in with the streaming families of kernel_checks.py: e4t_clip_preprocess tests P, S, Hin and Win
before it forms S % P (P = 0 was an integer division by zero on the host: the process died instead of returning -22; Hin = 0 clamped to row -1),
e4t_spatial_mean and e4t_spatial_mean_bwd keep their column slice inside the row (coff >= 0, ld >= coff + C), e4t_sumpool2, e4t_spatial_mean_bwd
and e4t_im2col_T refuse C <= 0 (im2col_T's was a grid of 0 blocks: -5 from the launch), and batch counts above grid.y / grid.z's 65535 are refused
by name instead of by the launch."""
import pytest

P = 4096      # a non-null, 16-byte aligned "pointer"
N = None


@pytest.fixture(scope="module")
def lib():
    from e4t import _C
    return _C.load()


def refused(lib, rc, words):
    assert rc == -22, rc
    assert words.encode() in lib.e4t_last_error(), (words, lib.e4t_last_error())


def each_null(n, optional=()):
    """pointer lists of length n with one required pointer null at a time"""
    for k in range(n):
        if k not in optional:
            ptrs = [P] * n
            ptrs[k] = N
            yield ptrs


def test_geglu_unary_add_refusals(lib):
    for ptrs in each_null(2):
        refused(lib, lib.e4t_geglu_fwd(*ptrs, 4, 8, N), "geglu_fwd: bad arguments")
    for ptrs in each_null(3):
        refused(lib, lib.e4t_geglu_bwd(*ptrs, 4, 8, N), "geglu_bwd: bad arguments")
        refused(lib, lib.e4t_add(*ptrs, 8, N), "add: bad arguments")
    for M, H in [(0, 8), (-1, 8), (4, 0), (4, 12), (4, -8)]:
        refused(lib, lib.e4t_geglu_fwd(P, P, M, H, N), "geglu_fwd: bad arguments")
        refused(lib, lib.e4t_geglu_bwd(P, P, P, M, H, N), "geglu_bwd: bad arguments")
    for n in (0, -8, 12):
        refused(lib, lib.e4t_add(P, P, P, n, N), "add: bad arguments")
        refused(lib, lib.e4t_unary(P, N, P, n, 0, N), "unary: bad arguments")
    for ptrs in each_null(3, optional=(1,)):
        refused(lib, lib.e4t_unary(*ptrs, 8, 1, N), "unary: bad arguments")
    for op in (-1, 8):
        refused(lib, lib.e4t_unary(P, P, P, 8, op, N), "unary: bad arguments")
    for op in (1, 3, 5, 7):
        refused(lib, lib.e4t_unary(P, N, P, 8, op, N), "unary: backward ops need dy")


def test_transpose_refusals(lib):
    for ptrs in each_null(2):
        refused(lib, lib.e4t_transpose(*ptrs, 1, 8, 8, 8, 8, 0, 0, N), "transpose: bad arguments")
    for batch, R, C, ldi, ldo in [(0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, 0, 8, 8), (1, 8, 8, 7, 8), (1, 8, 8, 8, 7)]:
        refused(lib, lib.e4t_transpose(P, P, batch, R, C, ldi, ldo, 0, 0, N), "transpose: bad arguments")
    refused(lib, lib.e4t_transpose(P, P, 65536, 8, 8, 8, 8, 64, 64, N), "transpose: batch = 65536")
    refused(lib, lib.e4t_transpose(P, P, 1, 65535 * 64 + 1, 8, 8, 65535 * 64 + 1, 0, 0, N), "at most 65535 batches and 65535 row tiles")


def test_conv_weight_prepare_refusals(lib):
    for args in [(N, P, P, 8, 8, 8, 8), (P, N, N, 8, 8, 8, 8), (P, P, P, 0, 8, 8, 8), (P, P, P, 8, 0, 8, 8), (P, P, P, 8, 8, 7, 8), (P, P, P, 8, 8, 8, 7)]:
        refused(lib, lib.e4t_conv_weight_prepare(*args, N), "conv_weight_prepare: bad arguments")


def test_sumpool2_refusals(lib):
    for ptrs in each_null(2):
        refused(lib, lib.e4t_sumpool2(*ptrs, 1, 2, 2, 8, N), "sumpool2: bad arguments")
    for B, H, W, C in [(0, 2, 2, 8), (1, 0, 2, 8), (1, 2, 0, 8), (1, 2, 2, 12), (1, 2, 2, 0), (1, 2, 2, -8)]:      # C <= 0: new
        refused(lib, lib.e4t_sumpool2(P, P, B, H, W, C, N), "sumpool2: bad arguments")


def test_spatial_mean_refusals(lib):
    for ptrs in each_null(2):
        refused(lib, lib.e4t_spatial_mean(*ptrs, 2, 16, 8, 8, 0, N), "spatial_mean: bad arguments")
    for B, HW, C in [(0, 16, 8), (2, 0, 8), (2, 16, 0), (2, 16, 6), (2, 16, -4)]:
        refused(lib, lib.e4t_spatial_mean(P, P, B, HW, C, 64, 0, N), "spatial_mean: bad arguments")
    refused(lib, lib.e4t_spatial_mean(P, P, 2, 16, 8, 64, -4, N), "spatial_mean: coff = -4, ldo = 64")
    refused(lib, lib.e4t_spatial_mean(P, P, 2, 16, 8, 7, 0, N), "ldo >= coff + C = 8")
    refused(lib, lib.e4t_spatial_mean(P, P, 2, 16, 132, 191, 60, N), "ldo >= coff + C = 192")
    refused(lib, lib.e4t_spatial_mean(P, P, 2, 16, 8, 2 ** 31 - 1, 2 ** 31 - 4, N), "the slice lies inside a row of out")      # coff + C past INT_MAX
    refused(lib, lib.e4t_spatial_mean(P, P, 65536, 16, 8, 8, 0, N), "spatial_mean: B = 65536")


def test_spatial_mean_bwd_refusals(lib):
    for ptrs in each_null(3, optional=(1,)):
        refused(lib, lib.e4t_spatial_mean_bwd(*ptrs, 2, 16, 8, 8, 0, N), "spatial_mean_bwd: bad arguments")
    for B, HW, C in [(0, 16, 8), (2, 0, 8), (2, 16, 12), (2, 16, 0), (2, 16, -8)]:      # C <= 0: new
        refused(lib, lib.e4t_spatial_mean_bwd(P, N, P, B, HW, C, 64, 0, N), "spatial_mean_bwd: bad arguments")
    refused(lib, lib.e4t_spatial_mean_bwd(P, N, P, 2, 16, 8, 64, -8, N), "spatial_mean_bwd: coff = -8, ldg = 64")
    refused(lib, lib.e4t_spatial_mean_bwd(P, N, P, 2, 16, 8, 15, 8, N), "ldg >= coff + C = 16")
    refused(lib, lib.e4t_spatial_mean_bwd(P, N, P, 65536, 16, 8, 8, 0, N), "spatial_mean_bwd: B = 65536")


def test_timestep_embedding_refusals(lib):
    for args in [(N, P, 2, 8), (P, N, 2, 8), (P, P, 0, 8), (P, P, 2, 0), (P, P, 2, 7), (P, P, 2, -2)]:
        refused(lib, lib.e4t_timestep_embedding(*args, N), "timestep_embedding: bad arguments")


def test_clip_preprocess_refusals(lib):
    """P = 0 first: before the fix this call divided by zero on the host"""
    refused(lib, lib.e4t_clip_preprocess(P, P, 1, 64, 64, 28, 0, 640, N), "clip_preprocess: P = 0, S = 28, Hin = 64, Win = 64 must be positive")
    for Hin, Win, S, Pp in [(64, 64, 28, -14), (64, 64, 0, 14), (64, 64, -28, 14), (0, 64, 28, 14), (64, 0, 28, 14), (-1, 64, 28, 14), (64, -1, 28, 14)]:
        refused(lib, lib.e4t_clip_preprocess(P, P, 1, Hin, Win, S, Pp, 640, N), "must be positive")
    for ptrs in each_null(2):
        refused(lib, lib.e4t_clip_preprocess(*ptrs, 1, 64, 64, 28, 14, 640, N), "clip_preprocess: bad arguments")
    refused(lib, lib.e4t_clip_preprocess(P, P, 0, 64, 64, 28, 14, 640, N), "clip_preprocess: bad arguments")
    refused(lib, lib.e4t_clip_preprocess(P, P, 1, 64, 64, 30, 14, 640, N), "clip_preprocess: bad arguments (S % P == 0, Kpad >= 3 * P * P)")
    refused(lib, lib.e4t_clip_preprocess(P, P, 1, 64, 64, 28, 14, 587, N), "clip_preprocess: bad arguments (S % P == 0, Kpad >= 3 * P * P)")


def test_softmax_rows_refusals(lib):
    for x, rows, L, ld in [(N, 2, 64, 64), (P, 0, 64, 64), (P, 2, 0, 64), (P, 2, 12, 64), (P, 2, 16392, 16392), (P, 2, 64, 56), (P, 2, 64, 68)]:
        refused(lib, lib.e4t_softmax_rows(x, rows, L, ld, N), "softmax_rows: bad arguments")
    refused(lib, lib.e4t_softmax_rows(P, 2 ** 31, 64, 64, N), "softmax_rows: too many rows")


def test_im2col_refusals(lib):
    for ptrs in each_null(2):
        refused(lib, lib.e4t_im2col3_rgb(*ptrs, 1, 4, 4, N), "im2col3_rgb: bad arguments")
        refused(lib, lib.e4t_im2col(*ptrs, 1, 4, 4, 8, 4, 4, 1, N), "im2col: bad arguments")
        refused(lib, lib.e4t_im2col_T(*ptrs, 1, 4, 4, 8, 4, 4, 16, 1, N), "im2col_T: bad arguments")
    for B, H, W in [(0, 4, 4), (1, 0, 4), (1, 4, 0)]:
        refused(lib, lib.e4t_im2col3_rgb(P, P, B, H, W, N), "im2col3_rgb: bad arguments")
        refused(lib, lib.e4t_im2col(P, P, B, H, W, 8, 4, 4, 1, N), "im2col: bad arguments")
        refused(lib, lib.e4t_im2col(P, P, 1, 4, 4, 8, B * H, W, 1, N), "im2col: bad arguments")      # Hout or Wout 0 (B = 0: Hout = 0)
        refused(lib, lib.e4t_im2col_T(P, P, B, H, W, 8, 4, 4, 16, 1, N), "im2col_T: bad arguments")
    refused(lib, lib.e4t_im2col(P, P, 1, 4, 4, 12, 4, 4, 1, N), "im2col: bad arguments (C must be a multiple of 8)")
    for mode in (0, 4, 5):
        refused(lib, lib.e4t_im2col(P, P, 1, 4, 4, 8, 4, 4, mode, N), "im2col: mode must be S1, S2 or UP2")
        refused(lib, lib.e4t_im2col_T(P, P, 1, 4, 4, 8, 4, 4, 16, mode, N), "im2col_T: mode must be S1, S2 or UP2")
    for C, ldo in [(6, 16), (8, 18), (8, 12), (0, 16), (-4, 16)]:      # C <= 0: new (was a grid of 0 blocks)
        refused(lib, lib.e4t_im2col_T(P, P, 1, 4, 4, C, 4, 4, ldo, 1, N), "im2col_T: C, ldo must be multiples of 4, C > 0, ldo >= B*Hout*Wout")


def test_sumsq_partial_refusals(lib):
    for args in [(N, 8, P, 4), (P, 8, N, 4), (P, 0, P, 4), (P, 8, P, 0), (P, -1, P, 4), (P, 8, P, -1)]:
        refused(lib, lib.e4t_sumsq_partial(*args, N), "sumsq_partial: bad arguments")
