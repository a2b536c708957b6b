"""CPU: kernel_checks.norm_plan() — the restatement of norm.hip's dispatch that check_norms holds the launch log against — reaches every logged
instantiation of norm.hip over GN_CASES + LN_CASES, and gives the hand-worked geometry for the cases chosen to sit on a dispatch edge."""
import os
import re

import pytest

import kernel_checks as kc

# Every kernel symbol norm.hip writes to the launch log (E4T_LOG_LAUNCH), by hand, with the production shape that uses it
# (B = 16 training step of SD-1.x at 64 x 64 latents unless stated).
NORM_SYMBOLS = {
    "gn_stats_kernel<1>": "ResBlock norm1 / norm2 at the 64 x 64 and 32 x 32 levels (C = 320 .. 1920)",
    "gn_stats_kernel<2>": "the 16 x 16 up-block concat 1280 + 1280 (C = 2560, HW = 256)",
    "gn_apply_kernel<true, 1>": "the fused finalize + apply behind gn_stats<1> / gn_stats_cols at the 64 x 64 and 32 x 32 levels",
    "gn_apply_kernel<true, 2>": "... behind gn_stats<2>: the 16 x 16 up-block concat 1280 + 1280",
    "gn_apply_kernel<false, 1>": "e4t_groupnorm_apply on its own statistics call (the unfused entry points, C <= 2048)",
    "gn_apply_kernel<false, 2>": "e4t_groupnorm_apply, C = 2560",
    "gn_stats_cols_kernel": "every GroupNorm whose producing conv / GEMM left column statistics: norm2 of each ResBlock, the up-block concats (640 + 320, 1280 + 640 straddle)",
    "gn_bwd_stats_kernel<1>": "the backward of every chunked GroupNorm, and of every GroupNorm when gamma / beta train (parameter-gradient partials)",
    "gn_bwd_stats_kernel<2>": "... at C = 2560",
    "gn_bwd_apply_kernel<1>": "second pass of the chunked backward, C <= 2048",
    "gn_bwd_apply_kernel<2>": "... at C = 2560",
    "gn_slab_fwd_kernel<3, true>": "8 x 8 level ResBlocks: HW = 64, C = 1280 (640 items)",
    "gn_slab_fwd_kernel<3, false>": "Transformer2DModel.norm (no SiLU) on small maps: HW = 64, C = 1280",
    "gn_slab_fwd_kernel<5, true>": "8 x 8 up-block concat 1280 + 1280 (1280 items)",
    "gn_slab_fwd_kernel<5, false>": "the same shape without SiLU (the tiny test UNet's transformer norm)",
    "gn_slab_fwd_kernel<10, true>": "16 x 16 level ResBlocks: HW = 256, C = 1280 (2560 items, exactly the limit)",
    "gn_slab_fwd_kernel<10, false>": "Transformer2DModel.norm at 16 x 16: HW = 256, C = 1280",
    "gn_slab_bwd_kernel<3, true>": "backward of the 8 x 8 ResBlock norms with frozen gamma / beta (pre-training)",
    "gn_slab_bwd_kernel<3, false>": "backward of the 8 x 8 transformer norm",
    "gn_slab_bwd_kernel<5, true>": "backward of the 8 x 8 up-block concat norm",
    "gn_slab_bwd_kernel<5, false>": "... without SiLU",
    "gn_slab_bwd_kernel<10, true>": "backward of the 16 x 16 ResBlock norms",
    "gn_slab_bwd_kernel<10, false>": "backward of the 16 x 16 transformer norm",
    "ln_fwd_kernel<1, 1, false>": "BasicTransformerBlock norms at D = 320 with few rows (sampling at B = 1), the CLIP text encoder's small tests",
    "ln_fwd_kernel<2, 1, false>": "D = 640 / 768 / 1024 with few rows: text encoder (77 tokens x 768 / 1024)",
    "ln_fwd_kernel<3, 1, false>": "D = 1280 with fewer than 2731 rows: the 16 x 16 transformer at small batch",
    "ln_fwd_kernel<1, 4, false>": "D = 320 at the 64 x 64 level: 65536 rows",
    "ln_fwd_kernel<2, 2, false>": "D = 640 at the 32 x 32 level: 16384 rows",
    "ln_fwd_kernel<3, 2, false>": "D = 1280 at the 16 x 16 level (4096 rows) and the ViT-H's 4112 token rows",
    "ln_fwd_kernel<1, 1, true>": "fp32 residual stream, D <= 512 (the small test ViT)",
    "ln_fwd_kernel<2, 1, true>": "fp32 residual stream, D = 768 / 1024 (ViT-B / ViT-L)",
    "ln_fwd_kernel<3, 1, true>": "fp32 residual stream, D = 1280 (ViT-H: 16 x 257 rows)",
    "ln_bwd_kernel<1>": "backward of the D = 320 transformer norms",
    "ln_bwd_kernel<2>": "... D = 640",
    "ln_bwd_kernel<3>": "... D = 1280",
}


def test_the_cases_reach_every_logged_instantiation():
    reached = set()
    for case in kc.GN_CASES + kc.LN_CASES:
        reached |= kc.norm_plan(case)["symbols"]
    assert reached == set(NORM_SYMBOLS), (sorted(set(NORM_SYMBOLS) - reached), sorted(reached - set(NORM_SYMBOLS)))


def test_the_table_names_every_kernel_norm_hip_logs():
    """the hand-written table against the source: every E4T_LOG_LAUNCH format string of norm.hip, its %d / %s expanded over the values the
    dispatch can pass, is in the table and nothing else is"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "e4t-diffusion_amd", "csrc", "norm.hip")).read()
    fmts = set(re.findall(r'E4T_LOG_LAUNCH\("([^|"]+)\|', src))
    assert fmts == {"gn_slab_fwd_kernel<%d, %s>", "gn_stats_kernel<%d>", "gn_apply_kernel<false, %d>", "gn_stats_cols_kernel", "gn_apply_kernel<true, %d>",
                    "gn_slab_bwd_kernel<%d, %s>", "gn_bwd_stats_kernel<%d>", "gn_bwd_apply_kernel<%d>", "ln_fwd_kernel<%d, %d, %s>", "ln_bwd_kernel<%d>"}
    names = set()
    for f in fmts:
        if f.startswith("gn_slab"):
            names |= {f.replace("%d", str(ni)).replace("%s", t) for ni in (3, 5, 10) for t in ("true", "false")}
        elif f.startswith("ln_fwd"):
            names |= {"ln_fwd_kernel<%d, %d, %s>" % v for v in [(n, 1, "true") for n in (1, 2, 3)] + [(n, 1, "false") for n in (1, 2, 3)] + [(1, 4, "false"), (2, 2, "false"), (3, 2, "false")]}
        elif f.startswith("ln_bwd"):
            names |= {f % n for n in (1, 2, 3)}
        elif "%d" in f:
            names |= {f % n for n in (1, 2)}
        else:
            names.add(f)
    assert names == set(NORM_SYMBOLS)


def _gn(B, HW, C1, C2):
    hit = [c for c in kc.GN_CASES if (c.B, c.HW, c.C1, c.C2) == (B, HW, C1, C2) and not c.shift]
    assert hit, (B, HW, C1, C2)
    return hit[-1]


# worked by hand from norm.hip: (B, HW, C1, C2) -> slots, slab quads per thread (0 = chunked), chunks, pixels per chunk, empty chunks, colstats precondition
GN_BY_HAND = {
    (2, 256, 1280, 1280): (2, 0, 32, 8, 0, True),      # HW * cpg = 20480 > 10240; ch = min(512, 256 / 8, 256) = 32
    (2, 256, 1280, 640): (1, 0, 32, 8, 0, True),       # cpg = 60: 1280 % 60 != 0 (a group straddles the concat); 8 blocks % min(32, 8) == 0
    (2, 260, 320, 0): (1, 0, 32, 9, 3, False),         # cpg = 10: no quads; ceil(260 / 32) = 9, ceil(260 / 9) = 29 chunks hold pixels
    (1, 257, 1280, 0): (1, 0, 32, 9, 3, False),        # 257 * 40 = 10280 > 10240
    (1, 256, 640, 640): (1, 10, 32, 8, 0, True),       # 256 * 40 = 10240: on the limit, slab; 2560 items = 10 x 256
    (2, 16, 320, 320): (1, 3, 2, 8, 0, False),         # 16 * 5 = 80 items -> 1 trip -> the NI = 3 kernel
    (2, 100, 640, 640): (1, 5, 12, 9, 0, False),       # 100 * 10 = 1000 items -> 4 trips -> NI = 5
    (2, 100, 1280, 1280): (2, 10, 12, 9, 0, False),    # 100 * 20 = 2000 items -> 8 trips -> NI = 10
    (2, 64, 64, 0): (1, 0, 8, 8, 0, True),             # cpg = 2: no quads
    (48, 1024, 64, 0): (1, 0, 21, 49, 0, False),       # ch = 1024 / 48 = 21; 32 blocks % 21 != 0: ops.groupnorm_fwd falls back
}


@pytest.mark.parametrize("key", list(GN_BY_HAND), ids=str)
def test_groupnorm_geometry_by_hand(key):
    c = _gn(*key)
    pl = kc.norm_plan(c)
    assert (pl["ns"], pl["ni"], pl["ch"], pl["ppc"], pl["empty"], pl["colstats"]) == GN_BY_HAND[key]
    assert (kc.gn_chunks(c.B, c.HW), kc.gn_slab_ni(c.C1, c.C2, c.HW, c.G)) == (pl["ch"], pl["ni"])


def test_named_paths():
    p = kc.norm_plan(_gn(2, 256, 1280, 1280))["calls"]
    assert p["fwd"] == ["gn_stats_kernel<2>", "gn_apply_kernel<true, 2>"] and p["fwd_cs"] == ["gn_stats_cols_kernel", "gn_apply_kernel<true, 2>"]
    assert p["unfused"] == ["gn_stats_kernel<2>", "gn_apply_kernel<false, 2>"] and p["bwd"] == p["bwd_pg"] == ["gn_bwd_stats_kernel<2>", "gn_bwd_apply_kernel<2>"]
    assert kc.norm_plan(_gn(2, 256, 1280, 640))["calls"]["fwd_cs"] == ["gn_stats_cols_kernel", "gn_apply_kernel<true, 1>"]
    p = kc.norm_plan(_gn(2, 16, 320, 320))["calls"]
    assert p["fwd"] == ["gn_slab_fwd_kernel<3, false>"] and p["bwd"] == ["gn_slab_bwd_kernel<3, false>"] and "fwd_cs" not in p
    assert p["bwd_pg"] == ["gn_bwd_stats_kernel<1>", "gn_bwd_apply_kernel<1>"]      # parameter gradients: never the slab kernel
    p = kc.norm_plan(_gn(48, 1024, 64, 0))["calls"]
    assert p["fwd_cs"] == p["fwd"] == ["gn_stats_kernel<1>", "gn_apply_kernel<true, 1>"]      # the fallback: no gn_stats_cols_kernel
    assert kc.norm_plan(_gn(1, 257, 1280, 0))["calls"]["fwd"] == ["gn_stats_kernel<1>", "gn_apply_kernel<true, 1>"]
    assert kc.norm_plan(_gn(1, 256, 640, 640))["calls"]["fwd_cs"] == ["gn_slab_fwd_kernel<10, false>"]      # slab: the column statistics are not read


@pytest.mark.parametrize("case, ncl, rpw, fwd", [
    ((300, 1280), 3, 1, "ln_fwd_kernel<3, 1, false>"),      # 300 * 3 = 900 < 8192
    ((5, 1536), 3, 1, "ln_fwd_kernel<3, 1, false>"),
    ((4101, 200), 1, 1, "ln_fwd_kernel<1, 1, false>"),      # 25 chunks: one per lane; 4101 < 8192
    ((4101, 640), 2, 2, "ln_fwd_kernel<2, 2, false>"),      # 80 chunks: two per lane; 8202 >= 8192
    ((8195, 320), 1, 4, "ln_fwd_kernel<1, 4, false>"),
    ((4112, 1280), 3, 2, "ln_fwd_kernel<3, 2, false>"),
], ids=str)
def test_layernorm_geometry_by_hand(case, ncl, rpw, fwd):
    assert case in kc.LN_CASES
    pl = kc.norm_plan(case)
    assert (pl["ncl"], pl["rpw"], pl["calls"]["fwd"]) == (ncl, rpw, [fwd])
    assert pl["calls"]["fwd_f32"] == [f"ln_fwd_kernel<{ncl}, 1, true>"] and pl["calls"]["bwd"] == [f"ln_bwd_kernel<{ncl}>"]
    assert kc.ln_rows_per_wave(2730, 1280) == (3, 1) and kc.ln_rows_per_wave(2731, 1280) == (3, 2)      # the threshold itself


def test_the_first_cases_keep_their_seeds_and_shortcut_gradients():
    """the eleven GroupNorm cases check_norms has always run: seeds 140 + i, add1 on the even ones, add2 on every two-source one but case 3"""
    assert [c.seed for c in kc.GN_CASES[:11]] == list(range(140, 151)) and not any(c.new for c in kc.GN_CASES[:11])
    assert [c.adds for c in kc.GN_CASES[:4]] == [((True, False),), ((False, False),), ((True, True),), ((False, False),)]
    assert all(c.new and c.seed >= 1400 for c in kc.GN_CASES[11:]) and len(kc.GN_CASES) == 22
