"""CPU: what norm.hip's entry points refuse.  Every call below fails validation on the host, before any launch, so the dummy pointer is never
dereferenced and no GPU is needed (the pattern of test_sampler_step_rejects_bad_arguments); each refusal is -22 with the words that name it.
Plus the three pure queries (chunks, workspace bytes, column-reduce splits) against their closed forms."""
import pytest

import kernel_checks as kc
from test_norm_plan_cpu import GN_BY_HAND

P = 4096      # a non-null, 16-byte aligned "pointer"
N = None


@pytest.fixture(scope="module")
def lib():
    from e4t import _C
    return _C.load()


def refused(lib, rc, words):
    assert rc == -22, rc
    assert words.encode() in lib.e4t_last_error(), (words, lib.e4t_last_error())


# the five GroupNorm entry points with everything but the shape valid (a workspace of no bytes: a shape that passed the common checks would
# stop there, or at a check before it, in every entry but e4t_groupnorm_apply — which only ever sees the shapes below, none of them valid)
GN_ENTRIES = {
    "stats": lambda lib, x1, C1, x2, C2, B, HW, G: lib.e4t_groupnorm_stats(x1, C1, x2, C2, B, HW, G, 1e-5, P, N, 0, N),
    "apply": lambda lib, x1, C1, x2, C2, B, HW, G: lib.e4t_groupnorm_apply(x1, C1, x2, C2, P, P, P, P, B, HW, G, 1, N),
    "fwd": lambda lib, x1, C1, x2, C2, B, HW, G: lib.e4t_groupnorm_fwd(x1, C1, x2, C2, P, P, P, P, B, HW, G, 1e-5, 1, N, 0, N),
    "fwd_cs": lambda lib, x1, C1, x2, C2, B, HW, G: lib.e4t_groupnorm_fwd_cs(x1, C1, P, x2, C2, P if C2 else N, P, P, P, P, B, HW, G, 1e-5, 1, N, 0, N),
    "bwd": lambda lib, x1, C1, x2, C2, B, HW, G: lib.e4t_groupnorm_bwd(x1, C1, x2, C2, P, P, P, P, N, N, P, P if C2 else N, N, B, HW, G, 1, N, 0, N),
}
# (x1, C1, x2, C2, B, HW, G) -> the words of the refusal
GN_COMMON = [
    ((N, 320, N, 0, 2, 256, 32), "groupnorm: bad arguments"),
    ((P, 0, N, 0, 2, 256, 32), "groupnorm: bad arguments"),
    ((P, 320, N, 0, 0, 256, 32), "groupnorm: bad arguments"),
    ((P, 320, N, 0, 2, 0, 32), "groupnorm: bad arguments"),
    ((P, 320, N, 0, 2, 256, 0), "groupnorm: bad arguments"),
    ((P, 320, P, 0, 2, 256, 32), "x2/C2 mismatch"),
    ((P, 320, N, 320, 2, 256, 32), "x2/C2 mismatch"),
    ((P, 320, N, 0, 2, 256, 3), "must divide"),             # 320 % 3 != 0
    ((P, 324, N, 0, 2, 256, 4), "must divide"),             # 324 % 4 == 0 but C1 % 8 != 0
    ((P, 320, P, 12, 2, 256, 4), "must divide"),            # C2 % 8 != 0
    ((P, 4104, N, 0, 2, 256, 8), "C=4104 too large"),       # more than two 16-byte chunks per thread
    ((P, 2056, N, 0, 2, 256, 257), "too large"),            # G = 257 > 256 (2056 = 257 * 8)
]


@pytest.mark.parametrize("entry", list(GN_ENTRIES))
@pytest.mark.parametrize("args, words", GN_COMMON, ids=lambda v: str(v).replace(" ", ""))
def test_every_groupnorm_entry_makes_the_common_checks(lib, entry, args, words):
    refused(lib, GN_ENTRIES[entry](lib, *args), words)


CHUNKED = (2, 260, 320, 32)      # (B, HW, C, G): cpg = 10, no slab kernel; 32 chunks


def _partials(B, HW, G):
    return B * kc.gn_chunks(B, HW) * G * 2 * 4


def test_groupnorm_stats_refusals(lib):
    B, HW, C, G = CHUNKED
    need = _partials(B, HW, G)
    refused(lib, lib.e4t_groupnorm_stats(P, C, N, 0, B, HW, G, 1e-5, P, P, need - 4, N), "groupnorm_stats: workspace too small")
    refused(lib, lib.e4t_groupnorm_stats(P, C, N, 0, B, HW, G, 1e-5, P, N, need, N), "groupnorm_stats: workspace too small")
    refused(lib, lib.e4t_groupnorm_stats(P, 1280, N, 0, 2, 64, 32, 1e-5, P, P, _partials(2, 64, 32) - 4, N), "groupnorm_stats: workspace too small")      # a slab shape: no slab path here


def test_groupnorm_apply_refusals(lib):
    B, HW, C, G = CHUNKED
    for k in range(4):
        ptrs = [P] * 4
        ptrs[k] = N      # mean_rstd, gamma, beta, y
        refused(lib, lib.e4t_groupnorm_apply(P, C, N, 0, *ptrs, B, HW, G, 1, N), "groupnorm_apply: null argument")


def test_groupnorm_fwd_refusals(lib):
    B, HW, C, G = CHUNKED
    need = _partials(B, HW, G)
    for shape in [(C, B, HW, G), (1280, 2, 64, 32)]:      # the null check comes before the slab branch
        for k in range(4):
            ptrs = [P] * 4
            ptrs[k] = N      # gamma, beta, y, mean_rstd
            c, b, hw, g = shape
            refused(lib, lib.e4t_groupnorm_fwd(P, c, N, 0, *ptrs, b, hw, g, 1e-5, 1, P, 1 << 30, N), "groupnorm_fwd: null argument")
    refused(lib, lib.e4t_groupnorm_fwd(P, C, N, 0, P, P, P, P, B, HW, G, 1e-5, 1, P, need - 4, N), "groupnorm_fwd: workspace too small")
    refused(lib, lib.e4t_groupnorm_fwd(P, C, N, 0, P, P, P, P, B, HW, G, 1e-5, 1, N, need, N), "groupnorm_fwd: workspace too small")


def test_groupnorm_fwd_cs_refusals(lib):
    big = 1 << 30
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, 320, N, N, 0, N, P, P, P, P, 2, 256, 32, 1e-5, 1, P, big, N), "groupnorm_fwd_cs: bad arguments")        # cs1 null
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, 320, P, N, 0, P, P, P, P, P, 2, 256, 32, 1e-5, 1, P, big, N), "groupnorm_fwd_cs: bad arguments")        # cs2 without C2
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, 320, P, P, 320, N, P, P, P, P, 2, 256, 32, 1e-5, 1, P, big, N), "groupnorm_fwd_cs: bad arguments")      # C2 without cs2
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, 320, P, N, 0, N, P, P, P, P, 2, 40, 32, 1e-5, 1, P, big, N), "groupnorm_fwd_cs: bad arguments")         # HW = 40: no whole 32-pixel blocks
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, 1280, P, N, 0, N, P, P, P, P, 2, 40, 32, 1e-5, 1, P, big, N), "groupnorm_fwd_cs: bad arguments")        # ... tested before the slab branch (40 * 40 <= 10240)
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, 1280, P, N, 0, N, P, P, N, P, 2, 64, 32, 1e-5, 1, P, big, N), "groupnorm_fwd_cs: bad arguments")        # y null on a slab shape
    # 32 blocks of 32 pixels into min(1024 / 48, 32) = 21 chunks (cpg = 2: no slab); refused before the workspace is looked at
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, 64, P, N, 0, N, P, P, P, P, 48, 1024, 32, 1e-5, 1, N, 0, N), "32 blocks do not split into 21 chunks")
    B, HW, C, G = 2, 256, 2560, 32       # chunked (256 * 80 > 10240), 8 blocks into 8 chunks
    need = B * 8 * G * 2 * 4
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, C, P, N, 0, N, P, P, P, P, B, HW, G, 1e-5, 1, P, need - 4, N), "groupnorm_fwd_cs: workspace too small")
    refused(lib, lib.e4t_groupnorm_fwd_cs(P, C, P, N, 0, N, P, P, P, P, B, HW, G, 1e-5, 1, N, need, N), "groupnorm_fwd_cs: workspace too small")


def test_groupnorm_bwd_refusals(lib):
    B, HW, C, G = CHUNKED
    big = 1 << 30

    def bwd(C1=C, x2=N, C2=0, dy=P, mr=P, ga=P, be=P, add2=N, dx1=P, dx2=N, pg=N, shape=(B, HW, G), ws=P, nb=big):
        return lib.e4t_groupnorm_bwd(P, C1, x2, C2, dy, mr, ga, be, N, add2, dx1, dx2, pg, *shape, 1, ws, nb, N)
    for kw in [dict(dy=N), dict(mr=N), dict(ga=N), dict(be=N), dict(dx1=N), dict(dx2=P), dict(x2=P, C2=320), dict(add2=P),
               dict(C1=1280, shape=(2, 64, 32), dy=N)]:      # the last: a slab shape, the null check comes first
        refused(lib, bwd(**kw), "groupnorm_bwd: null argument")
    # the contract ops.groupnorm_bwd allocates to: the partials plus B * G * 2 floats
    need = _partials(B, HW, G) + B * G * 8
    refused(lib, bwd(nb=need - 4), "groupnorm_bwd: workspace too small (%d < %d)" % (need - 4, need))
    refused(lib, bwd(ws=N, nb=need), "groupnorm_bwd: workspace too small")
    # parameter gradients keep a slab shape on the chunked path, so its workspace is checked
    need = _partials(2, 64, 32) + 2 * 32 * 8
    refused(lib, bwd(C1=1280, shape=(2, 64, 32), pg=P, nb=need - 4), "groupnorm_bwd: workspace too small (%d < %d)" % (need - 4, need))


def test_layernorm_refusals(lib):
    fwds = [lib.e4t_layernorm_fwd, lib.e4t_layernorm_fwd_f32]
    for fwd in fwds:
        for k in range(4):
            ptrs = [P, P, P, P]
            ptrs[k] = N      # x, gamma, beta, y   (mean_rstd may be null)
            refused(lib, fwd(*ptrs, N, 100, 320, 1e-5, N), "layernorm_fwd: null argument")
        refused(lib, fwd(P, P, P, P, P, 0, 320, 1e-5, N), "layernorm_fwd: null argument")
        refused(lib, fwd(P, P, P, P, P, 100, 12, 1e-5, N), "layernorm: D=12 must be a multiple of 8 and <= 1536")
        refused(lib, fwd(P, P, P, P, P, 100, 1544, 1e-5, N), "layernorm: D=1544 must be a multiple of 8 and <= 1536")
    refused(lib, lib.e4t_layernorm_fwd_f32(P + 8, P, P, P, P, 100, 320, 1e-5, N), "layernorm_fwd_f32: x must be 16-byte aligned")
    for k in (0, 1, 2, 3, 5):
        ptrs = [P] * 6
        ptrs[k] = N      # x, dy, gamma, mean_rstd, (add may be null), dx
        refused(lib, lib.e4t_layernorm_bwd(*ptrs, 100, 320, N), "layernorm_bwd: null argument")
    refused(lib, lib.e4t_layernorm_bwd(P, P, P, P, N, P, 0, 320, N), "layernorm_bwd: null argument")
    refused(lib, lib.e4t_layernorm_bwd(P, P, P, P, N, P, 100, 12, N), "layernorm: D=12 must")
    refused(lib, lib.e4t_layernorm_bwd(P, P, P, P, N, P, 100, 1544, N), "layernorm: D=1544 must")


def test_column_reduction_refusals(lib):
    M, C = 5000, 64      # 5 splits
    for args in [(N, 64, M, C, P), (P, 64, M, C, N), (P, 64, 0, C, P), (P, 64, M, 0, P), (P, 64, M, 12, P), (P, 60, M, C, P), (P + 8, 64, M, C, P)]:
        refused(lib, lib.e4t_colsum(*args, 0, P, 1 << 30, N), "colsum: bad arguments")
    need = 5 * C * 4
    refused(lib, lib.e4t_colsum(P, 64, M, C, P, 0, P, need - 4, N), "colsum: workspace too small")
    refused(lib, lib.e4t_colsum(P, 64, M, C, P, 0, N, need, N), "colsum: workspace too small")
    for k in range(5):
        ptrs = [P] * 5
        ptrs[k] = N      # x, dy, mean_rstd, dgamma, dbeta
        refused(lib, lib.e4t_layernorm_param_grad(*ptrs[:3], M, C, *ptrs[3:], 0, P, 1 << 30, N), "layernorm_param_grad: bad arguments")
    refused(lib, lib.e4t_layernorm_param_grad(P, P, P, M, 12, P, P, 0, P, 1 << 30, N), "layernorm_param_grad: bad arguments")
    refused(lib, lib.e4t_layernorm_param_grad(P, P, P, M, C, P, P, 0, P, 2 * need - 4, N), "layernorm_param_grad: workspace too small")
    refused(lib, lib.e4t_layernorm_param_grad(P, P, P, M, C, P, P, 0, N, 2 * need, N), "layernorm_param_grad: workspace too small")


@pytest.mark.parametrize("key", list(GN_BY_HAND), ids=str)
def test_pure_queries(lib, key):
    B, HW, C1, C2 = key
    G = [c.G for c in kc.GN_CASES if (c.B, c.HW, c.C1, c.C2) == key][0]
    ch = GN_BY_HAND[key][2]
    assert lib.e4t_groupnorm_num_chunks(B, HW) == kc.gn_chunks(B, HW) == ch
    assert lib.e4t_groupnorm_workspace_bytes(B, HW, C1 + C2, G, 0) == B * ch * G * 2 * 4
    assert lib.e4t_groupnorm_workspace_bytes(B, HW, C1 + C2, G, 1) == B * ch * G * 2 * 4 + B * ch * (C1 + C2) * 2 * 4
    for M in (B * HW, 1, 1024, 1025, 128 * 1024, 128 * 1024 + 1):
        assert lib.e4t_colreduce_splits(M) == min(max(-(-M // 1024), 1), 128)
