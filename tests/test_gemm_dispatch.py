"""The GEMM / 3x3-conv planner (csrc/gemm.hip: plan_gemm and the variant table behind it) decides for a broad corpus of descriptors what
the record says: tests/gemm_dispatch_record.txt holds one SHA-256 per corpus group (one tile hint x {gemm, conv}, and the TN planner)
over the lines `descriptor -> tile tile_m tile_n splitk workspace_bytes tail_rows stages`, and the plans of the training step's own
shapes in clear text.  Corpus and record come from tools/gemm_dispatch_dump.py; after an INTENTIONAL planner change

    python tools/gemm_dispatch_dump.py --record

rewrites the record (on a machine without a GPU: it anchors the step shapes through the launch log).  Only the plan entry points are
called here — pure host code, safe on any machine; the launch half of the tool is never part of a test.

The attention launchers (csrc/attention.hip: plan_fwd / plan_bwd, exported as e4t_attention_plan) are held to the same record: group `attn` hashes
`shape ws -> forward | dQ | dK/dV kernel | tsplit tchunk | workspace_floats` over both sides of every dispatch threshold and four workspace sizes,
and the step's attention shapes stand in clear text.  A slipped threshold passes every numeric check and only costs time; here it fails.

Which KERNEL a conv launch gets is decided after the plan (the strip predicates, the channel-major K order, the GENERAL epilogue, the automatic
split-K fallback); e4t_conv3x3_kernel reports it from the launcher's own decision.  Every case of the conv checks stands here with its kernel symbol
and split-K in clear text, and the symbols x conv modes the checks reach are held against everything the query returns over the corpus.

The dense GEMM gets the same: e4t_gemm_kernel / e4t_gemm_tn_kernel report symbol, split-K, store path, reduce kernel and tail rows from the function the
launch itself calls; every case of the GEMM checks, old and new, is pinned in clear text, and the (symbol, store path) pairs and reduce kernels the
checks reach are held against everything the query returns over the corpus."""
import ctypes as C
import importlib.util
import os
import re

import pytest

from e4t import _C

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gemm_dispatch_dump", os.path.join(R, "tools", "gemm_dispatch_dump.py"))
dump = importlib.util.module_from_spec(spec)
spec.loader.exec_module(dump)


def _cu_count():
    """CU count the planner sees: the device's where there is one, else its 256 fallback"""
    n = C.c_int(0)
    return n.value if _C.load().e4t_device_info(None, 0, C.byref(n)) == 0 else 256


def _record():
    groups, step, attn = {}, [], []
    for line in open(dump.RECORD):
        if line.startswith("group "):
            g, n, hx = (s.strip() for s in line[len("group "):].split("|"))
            groups[g] = (int(n), hx)
        elif line.startswith("step "):
            step.append(line[len("step "):].rstrip("\n"))
        elif line.startswith("attn "):
            attn.append(line.rstrip("\n"))
    return groups, step, attn


@pytest.fixture(scope="module")
def dumper():
    # the record is made where the planner sees 256 CUs: an MI355X, or no device at all (its fallback)
    if _cu_count() != 256:
        pytest.skip("the plan record is for 256 CUs (MI355X, or no device); this device has %d" % _cu_count())
    d = dump.Dumper(launches=False)
    yield d
    d.close()


def test_record_covers_the_corpus():
    groups, step, attn = _record()
    want = {"%s t%d" % (k, t) for k in ("gemm", "conv") for t in dump.HINTS} | {"tn", "attn"}
    assert set(groups) == want
    assert [a.split(" -> ")[0] for a in attn] == ["attn " + dump.describe(dict(zip(("B", "H", "T", "S", "DH", "causal"), sh), ws="full")) for sh in dump.attn_step_shapes()]
    rows = dump.step_rows()
    assert len(step) == len(rows) == 167 and sum(1 for s, _ in rows if not s.startswith("splitk_reduce")) == 153
    assert [s.split(" | ")[0] for s in step] == ["%s|%s" % r for r in rows]      # every recorded launch of the step table, in its order


def test_plans_match_the_record(dumper):
    groups, _, _ = _record()
    got, _ = dump.plan_digests(dumper)
    bad = [g for g in sorted(groups) if got.get(g) != groups[g]]
    assert not bad, ("the planner decides differently for corpus group(s) %s: compare `python tools/gemm_dispatch_dump.py --plans --group '%s'` of this "
                     "library and of the one the record was made from (E4T_LIB=...), or re-record an intentional change with --record" % (bad, bad[0]))


# the tile codes of the variants that were measured, rejected and removed -> the tile that answers them (gemm.hip, decode_hint)
RETIRED_HINTS = {256: 5256, 640: 128, 1128: 128, 1160: 160, 5064: 64, 5128: 128}
# a stage (3xxx / 4xxx) or K-tile (5xxx) prefix on a tile that never had such a row: accepted, and answered like this, as long as those codes existed
PREFIXED_HINTS = {3256: 5256, 4256: 5256, 3640: 128, 4640: 128, 5640: 128, 5160: 160, 5512: 512}


def test_retired_hints_plan_as_their_product_tile(dumper):
    """a retired code is an alias: over its whole corpus group, GEMM and conv, the plan is that of the same descriptor with the alias as the hint"""
    assert set(RETIRED_HINTS) <= set(dump.HINTS)
    groups = {"%s t%d" % (k, t) for k in ("gemm", "conv") for t in RETIRED_HINTS}
    n = 0
    for item in dump.corpus():
        if item.group in groups:
            alias = dump.Item(item.group, item.kind, dict(item.kw, tile=RETIRED_HINTS[item.kw["tile"]]))
            assert dumper.plan(item) == dumper.plan(alias), dump.describe(item.kw)
            n += 1
    assert n == sum(_record()[0][g][0] for g in groups)      # every line of the twelve groups
    # the prefixed spellings are in no corpus group: the training step's GEMM / conv shapes and the first 500 descriptors of two groups
    some = [it for it in dump.step_items() if it.kind != "tn"]
    for g in ("gemm t0", "conv t0"):
        some += [it for it, _ in zip((it for it in dump.corpus() if it.group == g), range(500))]
    for hint, alias in PREFIXED_HINTS.items():
        for item in some:
            assert dumper.plan(dump.Item("x", item.kind, dict(item.kw, tile=hint))) == dumper.plan(dump.Item("x", item.kind, dict(item.kw, tile=alias))), (hint, dump.describe(item.kw))
    # ... and none of them means "automatic" (what an unknown code gets) on a shape whose automatic tile is another one
    auto = dump.Item("x", "gemm", dict(M=65536, N=320, K=1280))
    assert dumper.plan(auto).split()[0] == "2320"
    assert all(dumper.plan(dump.Item("x", "gemm", dict(auto.kw, tile=h))).split()[0] == str(a) for h, a in PREFIXED_HINTS.items())


def test_step_shapes_get_the_recorded_plans(dumper):
    """the step's 153 GEMM / conv / TN launches (and the 14 split-K reduces behind them), descriptor and plan in clear text"""
    _, step, _ = _record()
    for line in step:
        sym_shape, rest = line.split(" | ", 1)
        desc, plan = rest.split(" -> ")
        kind, *kv = desc.split(" ")
        item = dump.Item("step", kind, {k: int(v) for k, v in (s.split("=") for s in kv)})
        assert dumper.plan(item) == plan, (sym_shape, desc)


def test_step_attention_shapes_get_the_recorded_kernels(dumper):
    """every attention shape of the step: the three kernels, the query split and the workspace in clear text; and every attention kernel the step
    table (profiles/r06_roofline_per_shape.csv) saw on hardware for a shape is one of the three the plan names for it"""
    _, _, attn = _record()
    assert len(attn) == 11
    for line, (shape, seen) in zip(attn, dump.attn_step_shapes().items()):
        desc, plan = line.split(" -> ")
        kw = dict(s.split("=") for s in desc.split(" ")[1:])
        kw = {k: v if k == "ws" else int(v) for k, v in kw.items()}
        assert tuple(kw[k] for k in ("B", "H", "T", "S", "DH", "causal")) == shape
        assert dumper.attn_plan(kw) == plan, desc
        assert set(seen) <= set(plan.split(" | ")[:3]), (desc, seen)
    by_shape = {a.split(" ws=")[0]: a.split(" -> ")[1].split(" | ") for a in attn}
    assert by_shape["attn B=16 H=8 T=4096 S=4096 DH=40 causal=0"][:4] == ["attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>", "1 4096"]
    assert by_shape["attn B=16 H=8 T=4096 S=77 DH=40 causal=0"][:4] == ["attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 2>", "8 512"]


# (B, H, T, S, DH[, causal]) of tests/kernel_checks.py::check_attention -> the kernels it gets with the workspace the library asks for (the
# first 30 as the launch log named them at b388eee, the last commit before e4t_attention_plan) [, "tsplit tchunk" where the case is there for its
# query split].  The keys are held against the check's own case lists, the kernel symbols against everything the plan can return.
CHECK_ATTENTION_KERNELS = {
    (2, 2, 64, 64, 32): ("attn_fwd_kernel<32>", "attn_bwd_dq_kernel<32>", "attn_bwd_dkv_kernel<32, 2>"),
    (2, 3, 200, 200, 40): ("attn_fwd_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),
    (1, 2, 128, 77, 40): ("attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (2, 2, 96, 77, 80): ("attn_fwd_kernel<80>", "attn_bwd_dq_kernel<80>", "attn_bwd_dkv_kernel<80, 1>"),
    (1, 2, 64, 64, 160): ("attn_fwd_kernel<160>", "attn_bwd_dq_kernel<160>", "attn_bwd_dkv_kernel<160, 1>"),
    (1, 2, 257, 257, 80): ("attn_fwd_kernel<80>", "attn_bwd_dq_kernel<80>", "attn_bwd_dkv_kernel<80, 1>"),
    (2, 2, 130, 33, 64): ("attn_fwd_kernel<64>", "attn_bwd_dq_kernel<64>", "attn_bwd_dkv_kernel<64, 2>"),
    (1, 8, 1024, 1024, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (3, 5, 300, 300, 40): ("attn_fwd_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),
    (2, 8, 4096, 4096, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),
    (1, 2, 300, 2100, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),
    (1, 1, 2050, 2050, 64): ("attn_fwd_kernel<64>", "attn_bwd_dq_dma_kernel<64>", "attn_bwd_dkv_kernel<64, 2>"),
    (3, 12, 77, 77, 64, True): ("attn_fwd_kernel<64>", "attn_bwd_dq_kernel<64>", "attn_bwd_dkv_kernel<64, 2>"),
    (2, 3, 200, 200, 40, True): ("attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (1, 2, 128, 128, 80, True): ("attn_fwd_kernel<80>", "attn_bwd_dq_kernel<80>", "attn_bwd_dkv_kernel<80, 1>"),
    (2, 8, 4096, 77, 40): ("attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (1, 2, 1000, 77, 40): ("attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (2, 2, 1024, 77, 80): ("attn_fwd_kernel<80>", "attn_bwd_dq_kernel<80>", "attn_bwd_dkv_kernel<80, 1>"),
    (1, 2, 600, 33, 64): ("attn_fwd_kernel<64>", "attn_bwd_dq_kernel<64>", "attn_bwd_dkv_kernel<64, 2>"),
    (1, 4, 1024, 1024, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (1, 2, 520, 520, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (2, 3, 700, 545, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (1, 1, 40, 512, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),
    (2, 2, 256, 640, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),
    (4, 8, 600, 2000, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),
    (2, 16, 1100, 2090, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),
    (1, 2, 130, 2100, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 3>"),
    (1, 1, 2080, 2080, 40, True): ("attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 3>", "7 320"),
    (1, 2, 200, 2100, 32): ("attn_fwd_kernel<32>", "attn_bwd_dq_dma_kernel<32>", "attn_bwd_dkv_kernel<32, 3>"),
    (2, 2, 256, 256, 32): ("attn_fwd_kernel<32>", "attn_bwd_dq_dma_kernel<32>", "attn_bwd_dkv_kernel<32, 2>"),
    (2, 2, 256, 256, 160): ("attn_fwd_kernel<160>", "attn_bwd_dq_kernel<160>", "attn_bwd_dkv_kernel<160, 1>"),
    (1, 2, 200, 77, 160): ("attn_fwd_kernel<160>", "attn_bwd_dq_kernel<160>", "attn_bwd_dkv_kernel<160, 1>"),
    (1, 1, 300, 130, 160): ("attn_fwd_kernel<160>", "attn_bwd_dq_kernel<160>", "attn_bwd_dkv_kernel<160, 1>"),
    (1, 2, 600, 77, 160): ("attn_fwd_kernel<160>", "attn_bwd_dq_kernel<160>", "attn_bwd_dkv_kernel<160, 1>", "2 320"),
    (2, 2, 200, 233, 64): ("attn_fwd_kernel<64>", "attn_bwd_dq_dma_kernel<64>", "attn_bwd_dkv_kernel<64, 2>"),
    (16, 8, 4096, 4096, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),      # the bitwise determinism check
    (4, 8, 4096, 4096, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),       # ... and its four batch chunks
    (1, 1, 64, 160, 64): ("attn_fwd_kernel<64>", "attn_bwd_dq_kernel<64>", "attn_bwd_dkv_kernel<64, 2>"),                 # peaked scores
    (1, 1, 96, 840, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),           # ... on the long-key forward
    (1, 1, 256, 840, 40): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_dma_kernel<40>"),         # ... and the LDS-DMA dK/dV kernel
    (1, 2, 96, 77, 80): ("attn_fwd_kernel<80>", "attn_bwd_dq_kernel<80>", "attn_bwd_dkv_kernel<80, 1>"),                  # ... the row sum in the MFMA's spare row
    (1, 1, 96, 200, 40): ("attn_fwd_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>"),             # ... the short-key dh-40 forward
    (2, 8, 1024, 77, 40): ("attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 2>", "4 256"),       # the full-workspace side of a small-workspace case
}

# (case, workspace label of tools/gemm_dispatch_dump.py) -> what a workspace smaller than the stated size gives: the backward calls check_attention makes
# through the raw ABI (kernel_checks.ATTENTION_WS_CASES, and the peaked T256 input with a Delta-only workspace).  One query chunk, no {L, Delta} pairs.
CHECK_ATTENTION_WS_KERNELS = {
    ((1, 2, 300, 2100, 40), "delta"): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 3>", "1 320"),
    ((2, 3, 200, 200, 40), "delta"): ("attn_fwd_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>", "1 256"),
    ((2, 3, 200, 200, 40), "short"): ("attn_fwd_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>", "1 256"),
    ((2, 8, 1024, 77, 40), "delta"): ("attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 2>", "1 256"),
    ((1, 1, 2080, 2080, 40, True), "delta"): ("attn_fwd_kernel<40>", "attn_bwd_dq_kernel<40>", "attn_bwd_dkv_kernel<40, 3>", "1 320"),
    ((1, 2, 600, 77, 160), "delta"): ("attn_fwd_kernel<160>", "attn_bwd_dq_kernel<160>", "attn_bwd_dkv_kernel<160, 1>", "1 320"),
    ((1, 1, 256, 840, 40), "delta"): ("attn_fwd64_kernel<40>", "attn_bwd_dq_dma_kernel<40>", "attn_bwd_dkv_kernel<40, 2>", "1 256"),
}


def _plan_kw(case, ws):
    return dict(zip(("B", "H", "T", "S", "DH"), case[:5]), causal=int(len(case) > 5 and bool(case[5])), ws=ws)


def test_the_pinned_tables_cover_exactly_what_check_attention_runs():
    """one case list (tests/kernel_checks.py, importable without a GPU) behind the GPU check and these tables"""
    import kernel_checks as kc
    peaked = [shape for _, shape, _ in kc.ATTENTION_PEAKED.values()]
    small_ws = [case for case, _, _ in kc.ATTENTION_WS_CASES]
    assert len(set(kc.ATTENTION_CASES)) == len(kc.ATTENTION_CASES)
    assert set(CHECK_ATTENTION_KERNELS) == set(kc.ATTENTION_CASES) | set(kc.ATTENTION_DETERMINISM_CASES) | set(peaked) | set(small_ws)
    assert set(CHECK_ATTENTION_WS_KERNELS) == {(case, ws) for case, labels, _ in kc.ATTENTION_WS_CASES for ws in labels} | {((1, 1, 256, 840, 40), "delta")}
    for group in (kc.ATTENTION_NEW_CASES, kc.ATTENTION_GAP_CASES, kc.ATTENTION_NULL_LSE_CASES):
        assert set(group) <= set(kc.ATTENTION_CASES)
    assert all(entry == "plain" or entry == "ws" for _, _, entry in kc.ATTENTION_WS_CASES) and any(entry == "plain" for _, _, entry in kc.ATTENTION_WS_CASES)


def test_check_attention_shapes_keep_their_kernels(dumper):
    for case, kernels in CHECK_ATTENTION_KERNELS.items():
        plan = dumper.attn_plan(_plan_kw(case, "full")).split(" | ")
        assert tuple(plan[:len(kernels)]) == kernels, case
    for (case, ws), kernels in CHECK_ATTENTION_WS_KERNELS.items():
        assert tuple(dumper.attn_plan(_plan_kw(case, ws)).split(" | ")[:4]) == kernels, (case, ws)
        assert tuple(dumper.attn_plan(_plan_kw(case, "full")).split(" | ")[:4]) != kernels, (case, ws)      # the small workspace changes the plan


def test_check_attention_reaches_every_kernel_the_plan_can_name(dumper):
    """the kernel symbols of the pinned full-workspace table == the symbols e4t_attention_plan returns anywhere in the `attn` corpus with the
    workspace the library asks for: an instantiation added to the dispatch (or a threshold moved so that one is newly reached) fails here until
    check_attention has a shape that executes it"""
    reachable = set()
    for item in dump.attn_corpus():
        if item.kw["ws"] == "full":
            reachable |= set(dumper.attn_plan(item.kw).split(" | ")[:3])
    assert len(reachable) == 22
    pinned = {sym for kernels in CHECK_ATTENTION_KERNELS.values() for sym in kernels[:3]}
    assert pinned == reachable, (sorted(reachable - pinned), sorted(pinned - reachable))
    # a smaller workspace selects among the same kernels: nothing is reachable only that way
    assert {sym for kernels in CHECK_ATTENTION_WS_KERNELS.values() for sym in kernels[:3]} <= reachable


# ---- 3x3 conv: case of tests/kernel_checks.py (B, Hin, Win, Cin, Cout, mode, Hout, Wout, tile, splitk) -> what e4t_conv3x3 launches for it, "<kernel
# symbol> splitk<n>" as e4t_conv3x3_kernel reports it, in the full form (bias + row bias + residual) and the bare form (none of them).  The two differ
# where Hout * Wout % 32 != 0: the row bias then needs the GENERAL epilogue, which the 3- and 4-stage 128 / 160 tiles, the 4-stage 64 tile, the
# 32-wide-K tile and the 256 x 320 tile do not have (the plan answers with the 2-stage tile of that width).
from kernel_checks import CONV_S1, CONV_S2, CONV_UP2, CONV_S2T, CONV_S2A  # noqa: E402

CHECK_CONV_KERNELS = {
    (2, 16, 16, 64, 64, CONV_S1, 16, 16, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 8, 8, 128, 192, CONV_S1, 8, 8, 64, 3): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk3", "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk3"),
    (3, 16, 16, 64, 128, CONV_S2, 8, 8, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 64, CONV_S2, 5, 5, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 8, 8, 64, 64, CONV_UP2, 16, 16, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 8, 8, 128, 64, CONV_S2T, 16, 16, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 5, 5, 64, 64, CONV_S2T, 9, 9, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (4, 32, 32, 320, 320, CONV_S1, 32, 32, 128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1"),
    (2, 16, 16, 64, 4, CONV_S1, 16, 16, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 24, 24, 64, 192, CONV_S1, 24, 24, 256, 1): ("gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1"),
    (3, 24, 24, 64, 320, CONV_S1, 24, 24, 160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk1"),
    (2, 16, 16, 128, 128, CONV_S2A, 8, 8, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (1, 64, 64, 128, 128, CONV_S2A, 32, 32, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 24, 24, 64, 320, CONV_S1, 24, 24, 512, 1): ("gemm_pp_kernel<1, false, true> splitk1", "gemm_pp_kernel<1, false, true> splitk1"),
    (2, 32, 32, 128, 256, CONV_S1, 32, 32, 512, 1): ("gemm_pps_kernel<false> splitk1", "gemm_pps_kernel<false> splitk1"),
    (2, 16, 16, 256, 512, CONV_S1, 16, 16, 512, 2): ("gemm_pps_kernel<false> splitk2", "gemm_pps_kernel<false> splitk2"),
    (3, 16, 16, 64, 128, CONV_S2, 8, 8, 512, 1): ("gemm_pp_kernel<1, false, false> splitk1", "gemm_pp_kernel<1, false, false> splitk1"),
    (2, 8, 8, 64, 64, CONV_UP2, 16, 16, 512, 1): ("gemm_pp_kernel<1, false, false> splitk1", "gemm_pp_kernel<1, false, false> splitk1"),
    (2, 8, 8, 128, 64, CONV_S2T, 16, 16, 512, 1): ("gemm_pp_kernel<1, false, false> splitk1", "gemm_pp_kernel<1, false, false> splitk1"),
    (1, 64, 64, 128, 128, CONV_S2A, 32, 32, 512, 1): ("gemm_pp_kernel<1, false, false> splitk1", "gemm_pp_kernel<1, false, false> splitk1"),
    (2, 48, 40, 64, 320, CONV_S1, 48, 40, 5256, 1): ("gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1"),
    (2, 20, 12, 192, 128, CONV_S1, 20, 12, 5256, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1"),
    (4, 32, 32, 320, 320, CONV_S1, 32, 32, 2320, 1): ("gemm_pq_kernel<1, 320, false> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (2, 16, 16, 256, 640, CONV_S1, 16, 16, 2320, 2): ("gemm_pq_kernel<1, 320, false> splitk2", "gemm_pq_kernel<1, 320, false> splitk2"),
    (2, 8, 8, 128, 320, CONV_S2T, 16, 16, 2320, 1): ("gemm_pq_kernel<1, 320, false> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (3, 16, 16, 64, 320, CONV_S2, 8, 8, 2320, 1): ("gemm_pq_kernel<1, 320, false> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (2, 8, 8, 64, 320, CONV_UP2, 16, 16, 2320, 1): ("gemm_pq_kernel<1, 320, false> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (16, 64, 64, 64, 320, CONV_S1, 64, 64, 2320, 1): ("gemm_pq_kernel<1, 320, false> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (2, 6, 256, 64, 128, CONV_S1, 6, 256, 5256, 1): ("conv_strip_kernel<2> splitk1", "conv_strip_kernel<2> splitk1"),
    (1, 3, 768, 192, 256, CONV_S1, 3, 768, 5256, 1): ("conv_strip_kernel<2> splitk1", "conv_strip_kernel<2> splitk1"),
    (3, 1, 256, 64, 128, CONV_S1, 1, 256, 5256, 1): ("conv_strip_kernel<2> splitk1", "conv_strip_kernel<2> splitk1"),
    (2, 5, 512, 128, 128, CONV_S1, 5, 512, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 64, 64, 64, 256, CONV_S1, 64, 64, 512, 1): ("gemm_pps_kernel<false> splitk1", "gemm_pps_kernel<false> splitk1"),
    (1, 4, 256, 128, 320, CONV_S1, 4, 256, 512, 1): ("gemm_pps_kernel<false> splitk1", "gemm_pps_kernel<false> splitk1"),
    (1, 2, 512, 64, 256, CONV_S1, 2, 512, 512, 1): ("gemm_pps_kernel<false> splitk1", "gemm_pps_kernel<false> splitk1"),
    (2, 16, 16, 192, 256, CONV_S1, 16, 16, 512, 3): ("gemm_pps_kernel<false> splitk3", "gemm_pps_kernel<false> splitk3"),
    (3, 128, 128, 64, 128, CONV_S1, 128, 128, 512, 1): ("gemm_pps_kernel<false> splitk1", "gemm_pps_kernel<false> splitk1"),
    (2, 9, 9, 64, 72, CONV_S1, 9, 9, 64, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_S2, 5, 5, 64, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_UP2, 18, 18, 64, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk1"),
    (2, 5, 5, 64, 72, CONV_S2T, 9, 9, 64, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_S2A, 4, 4, 64, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_S1, 9, 9, 3064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_S2, 5, 5, 3064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_UP2, 18, 18, 3064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 3, false, 64> splitk1"),
    (2, 5, 5, 64, 72, CONV_S2T, 9, 9, 3064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_S2A, 4, 4, 3064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_S1, 9, 9, 4064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_S2, 5, 5, 4064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_UP2, 18, 18, 4064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 5, 5, 64, 72, CONV_S2T, 9, 9, 4064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 72, CONV_S2A, 4, 4, 4064, 1): ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S1, 9, 9, 128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S2, 5, 5, 128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_UP2, 18, 18, 128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1"),
    (2, 5, 5, 64, 136, CONV_S2T, 9, 9, 128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S2A, 4, 4, 128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S1, 9, 9, 3128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S2, 5, 5, 3128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_UP2, 18, 18, 3128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 3, false, 64> splitk1"),
    (2, 5, 5, 64, 136, CONV_S2T, 9, 9, 3128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S2A, 4, 4, 3128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S1, 9, 9, 4128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S2, 5, 5, 4128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_UP2, 18, 18, 4128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 4, false, 64> splitk1"),
    (2, 5, 5, 64, 136, CONV_S2T, 9, 9, 4128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S2A, 4, 4, 4128, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S1, 9, 9, 160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S2, 5, 5, 160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_UP2, 18, 18, 160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk1"),
    (2, 5, 5, 64, 168, CONV_S2T, 9, 9, 160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S2A, 4, 4, 160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S1, 9, 9, 3160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S2, 5, 5, 3160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_UP2, 18, 18, 3160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 3, false, 64> splitk1"),
    (2, 5, 5, 64, 168, CONV_S2T, 9, 9, 3160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S2A, 4, 4, 3160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 3, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S1, 9, 9, 4160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S2, 5, 5, 4160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_UP2, 18, 18, 4160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 4, false, 64> splitk1"),
    (2, 5, 5, 64, 168, CONV_S2T, 9, 9, 4160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 168, CONV_S2A, 4, 4, 4160, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 4, false, 64> splitk1"),
    (2, 9, 9, 64, 136, CONV_S1, 9, 9, 5256, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1"),
    (2, 9, 9, 64, 136, CONV_S2, 5, 5, 5256, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1"),
    (2, 9, 9, 64, 136, CONV_UP2, 18, 18, 5256, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1"),
    (2, 5, 5, 64, 136, CONV_S2T, 9, 9, 5256, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1"),
    (2, 9, 9, 64, 136, CONV_S2A, 4, 4, 5256, 1): ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1"),
    (2, 9, 9, 64, 264, CONV_S1, 9, 9, 512, 1): ("gemm_pp_kernel<1, true, true> splitk1", "gemm_pp_kernel<1, false, true> splitk1"),
    (2, 9, 9, 64, 264, CONV_S2, 5, 5, 512, 1): ("gemm_pp_kernel<1, true, false> splitk1", "gemm_pp_kernel<1, false, false> splitk1"),
    (2, 9, 9, 64, 264, CONV_UP2, 18, 18, 512, 1): ("gemm_pp_kernel<1, true, false> splitk1", "gemm_pp_kernel<1, false, false> splitk1"),
    (2, 5, 5, 64, 264, CONV_S2T, 9, 9, 512, 1): ("gemm_pp_kernel<1, true, false> splitk1", "gemm_pp_kernel<1, false, false> splitk1"),
    (2, 9, 9, 64, 264, CONV_S2A, 4, 4, 512, 1): ("gemm_pp_kernel<1, true, false> splitk1", "gemm_pp_kernel<1, false, false> splitk1"),
    (2, 9, 9, 64, 320, CONV_S1, 9, 9, 2320, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (2, 9, 9, 64, 320, CONV_S2, 5, 5, 2320, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (2, 9, 9, 64, 320, CONV_UP2, 18, 18, 2320, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (2, 5, 5, 64, 320, CONV_S2T, 9, 9, 2320, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (2, 9, 9, 64, 320, CONV_S2A, 4, 4, 2320, 1): ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64> splitk1", "gemm_pq_kernel<1, 320, false> splitk1"),
    (3, 1, 1, 64, 64, CONV_S1, 1, 1, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 1, 7, 64, 64, CONV_S1, 1, 7, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 7, 1, 64, 64, CONV_S1, 7, 1, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 2, 2, 64, 64, CONV_S1, 2, 2, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 1, 1, 64, 64, CONV_S2, 1, 1, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 2, 3, 64, 64, CONV_S2, 1, 2, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 1, 1, 64, 64, CONV_UP2, 2, 2, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 1, 1, 64, 64, CONV_S2T, 1, 1, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 2, 2, 64, 64, CONV_S2T, 3, 3, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 9, 7, 64, 64, CONV_S2A, 4, 3, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 2, 2, 64, 64, CONV_S2A, 1, 1, 0, 0): ("gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1"),
    (3, 16, 16, 64, 136, CONV_S1, 16, 16, 5256, 1): ("conv_strip_kernel<2> splitk1", "conv_strip_kernel<2> splitk1"),
    (2, 16, 16, 64, 264, CONV_S1, 16, 16, 512, 1): ("gemm_pps_kernel<false> splitk1", "gemm_pps_kernel<false> splitk1"),
}

# check_conv_forms: family -> the kernel of every single-pass form (colstats, fp32 output, accumulate, row-bias slice), and of the explicit split-K call
CHECK_CONV_FORM_KERNELS = {
    "64": ("gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk1", "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk3"),
    "128": ("gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1", "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk3"),
    "160": ("gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk1", "gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64> splitk3"),
    "5256": ("gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk3"),
    "5256 strip": ("conv_strip_kernel<2> splitk1", "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32> splitk3"),
    "512": ("gemm_pp_kernel<1, false, true> splitk1", "gemm_pp_kernel<1, false, true> splitk3"),
    "512 pps": ("gemm_pps_kernel<false> splitk1", "gemm_pps_kernel<false> splitk3"),
    "2320": ("gemm_pq_kernel<1, 320, false> splitk1", "gemm_pq_kernel<1, 320, false> splitk3"),
}
# ... and with E4T_ACT_GELU through the raw ABI.  The strip geometries make Hout * Wout a multiple of 256, so a row bias never asks a strip kernel for the
# GENERAL epilogue: the flag is the only way to gemm_pps_kernel<true>.
CHECK_CONV_GELU_KERNELS = {"512": "gemm_pp_kernel<1, true, true> splitk1", "512 pps": "gemm_pps_kernel<true> splitk1"}

CHECK_CONV_OUT_KERNELS = {
    (2, 16, 16, 64, 4, CONV_S1, 16, 16, 0, 0): "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64> splitk1",
    (2, 16, 16, 64, 4, CONV_S1, 16, 16, 64, 0): "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64> splitk1",
    (2, 16, 16, 64, 4, CONV_S1, 16, 16, 128, 0): "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64> splitk1",
}


# Every kernel symbol e4t_conv3x3_kernel returns over the conv groups of the corpus and conv_geometry_corpus() (tools/gemm_dispatch_dump.py), with the
# conv modes it is returned for.  The mode is a run-time branch of the gather, so symbol x mode is the unit the checks must reach.
ALL_MODES = (CONV_S1, CONV_S2, CONV_UP2, CONV_S2T, CONV_S2A)
CONV_KERNEL_MODES = {
    "conv_strip_kernel<2>": (CONV_S1,),
    "gemm_dma_kernel<64, 64, 2, 2, 1, 2, false, 64>": ALL_MODES, "gemm_dma_kernel<64, 64, 2, 2, 1, 2, true, 64>": ALL_MODES,
    "gemm_dma_kernel<64, 64, 2, 2, 1, 3, false, 64>": ALL_MODES, "gemm_dma_kernel<64, 64, 2, 2, 1, 3, true, 64>": ALL_MODES,
    "gemm_dma_kernel<64, 64, 2, 2, 1, 4, false, 64>": ALL_MODES,
    "gemm_dma_kernel<128, 128, 4, 2, 1, 2, false, 64>": ALL_MODES, "gemm_dma_kernel<128, 128, 4, 2, 1, 2, true, 64>": ALL_MODES,
    "gemm_dma_kernel<128, 128, 4, 2, 1, 3, false, 64>": ALL_MODES, "gemm_dma_kernel<128, 128, 4, 2, 1, 4, false, 64>": ALL_MODES,
    "gemm_dma_kernel<128, 160, 4, 1, 1, 2, false, 64>": ALL_MODES, "gemm_dma_kernel<128, 160, 4, 1, 1, 2, true, 64>": ALL_MODES,
    "gemm_dma_kernel<128, 160, 4, 1, 1, 3, false, 64>": ALL_MODES, "gemm_dma_kernel<128, 160, 4, 1, 1, 4, false, 64>": ALL_MODES,
    "gemm_dma_kernel<256, 128, 4, 2, 1, 3, false, 32>": ALL_MODES,
    "gemm_pp_kernel<1, false, false>": (CONV_S2, CONV_UP2, CONV_S2T, CONV_S2A), "gemm_pp_kernel<1, true, false>": (CONV_S2, CONV_UP2, CONV_S2T, CONV_S2A),
    "gemm_pp_kernel<1, false, true>": (CONV_S1,), "gemm_pp_kernel<1, true, true>": (CONV_S1,),      # stride 1 walks K channel-major: a template argument here
    "gemm_pps_kernel<false>": (CONV_S1,), "gemm_pps_kernel<true>": (CONV_S1,),
    "gemm_pq_kernel<1, 320, false>": ALL_MODES,
    "gemm_kernel": ALL_MODES,
}
# symbol -> why no check executes it (in any of its modes)
CONV_KERNELS_NOT_REACHED = {
    "gemm_kernel": "the register-staged fallback: chosen only for an input map beyond 4 GB (or under the E4T_GEMM_REGSTAGE switch, read once per process)",
}


def _conv_checks():
    """(what, case, form, split-K override) -> pinned "<symbol> splitk<n>", for everything the conv checks launch"""
    import kernel_checks as kc
    rows = {}
    for case, (full, bare) in CHECK_CONV_KERNELS.items():
        rows[("case", case, "full", None)], rows[("case", case, "bare", None)] = full, bare
    for fam, (single, split) in CHECK_CONV_FORM_KERNELS.items():
        for form in kc.CONV_FORMS:
            if form not in ("full", "bare", "gelu"):
                rows[(fam, kc.CONV_FORM_CASES[fam], form, None)] = single
        rows[(fam, kc.CONV_FORM_CASES[fam], "colstats", kc.CONV_FORM_SPLITK)] = split
    for fam, sym in CHECK_CONV_GELU_KERNELS.items():
        rows[(fam, kc.CONV_FORM_CASES[fam], "gelu", None)] = sym
    for case, sym in CHECK_CONV_OUT_KERNELS.items():
        rows[("conv_out", case, "f32 bias", None)] = sym
    return rows


def test_the_pinned_conv_tables_cover_exactly_what_the_conv_checks_run():
    """one set of case lists (tests/kernel_checks.py, importable without a GPU) behind the GPU checks and these tables"""
    import kernel_checks as kc
    every = kc.CONV_ALL_CASES + kc.CONV_GUARD_CASES
    assert len(set(kc.CONV_ALL_CASES)) == len(kc.CONV_ALL_CASES) == len(kc.CONV_CASES) + len(kc.CONV_REACH_CASES) + len(kc.CONV_DEGENERATE_CASES)
    assert set(CHECK_CONV_KERNELS) == set(every)
    assert set(CHECK_CONV_FORM_KERNELS) == set(kc.CONV_FORM_CASES)
    assert set(CHECK_CONV_OUT_KERNELS) == set(kc.CONV_OUT_CASES) and set(CHECK_CONV_GELU_KERNELS) == set(kc.CONV_GELU_FAMILIES)
    assert len(kc.CONV_REACH_CASES) == 5 * len(kc.CONV_REACH_TILES) and {c[8] for c in kc.CONV_REACH_CASES} == {t for t, _ in kc.CONV_REACH_TILES}
    # the forms the model calls are all there: colstats with and without residual, three fp32 outputs, accumulate into both types, the row-bias slice
    assert set(kc.CONV_FORMS) == {"full", "bare", "colstats", "colstats+res", "f32 bias", "f32 res32", "f32 res16", "accum16", "accum32", "rowbias slice", "gelu"}
    assert all(c[0] * c[6] * c[7] % 32 == 0 for c in kc.CONV_FORM_CASES.values())      # column statistics need M % 32 == 0


def test_conv_check_cases_keep_their_kernels(dumper):      # (the fixture: the tables are for 256 CUs)
    import kernel_checks as kc
    for (what, case, form, sk), pinned in _conv_checks().items():
        assert kc.conv_kernel(case, form, sk) == pinned, (what, case, form, sk)
    # the families of check_conv_forms are the eight conv kernel families, one kernel each; the strip kernel takes no split-K
    assert len({single.split(" splitk")[0] for single, _ in CHECK_CONV_FORM_KERNELS.values()}) == 8
    assert all(single.endswith(" splitk1") and split.endswith(" splitk%d" % kc.CONV_FORM_SPLITK) for single, split in CHECK_CONV_FORM_KERNELS.values())
    # the automatic split-K falls back to ONE pass without a workspace, and the query says so; an explicit one is refused like the launch (-12)
    case = (2, 8, 8, 1280, 1280, CONV_S1, 8, 8, 0, 0)
    assert int(kc.conv_kernel(case, "bare").split(" splitk")[1]) > 1
    d = kc.conv_desc(case, "bare")
    d.workspace, d.workspace_bytes = None, 0
    sym, sk = C.c_char_p(), C.c_int(0)
    assert _C.load().e4t_conv3x3_kernel(C.byref(d), C.byref(sym), C.byref(sk)) == 0 and sk.value == 1
    d.splitk = 3
    assert _C.load().e4t_conv3x3_kernel(C.byref(d), C.byref(sym), C.byref(sk)) == -12
    d.Cin = 65
    assert _C.load().e4t_conv3x3_kernel(C.byref(d), C.byref(sym), C.byref(sk)) == -22 and b"multiple of 64" in _C.load().e4t_last_error()


def test_conv_checks_reach_every_kernel_the_launcher_can_choose(dumper):
    """symbol x mode over the conv corpus == the clear-text set above, and the checks execute each of them but the listed exceptions: a kernel added to
    the variant table (or a predicate changed so that one is no longer reached) fails here until a conv check has a shape that executes it"""
    import itertools
    reachable = {}
    for item in itertools.chain(dump.corpus(), dump.conv_geometry_corpus()):
        if item.kind == "conv":
            said = dumper.conv_kernel(item)
            if not said.startswith("rc "):
                reachable.setdefault(said.split(" splitk")[0], set()).add(item.kw["mode"])
    assert {s: tuple(sorted(m)) for s, m in reachable.items()} == CONV_KERNEL_MODES
    reached = {(pinned.split(" splitk")[0], case[5]) for (_, case, _, _), pinned in _conv_checks().items()}
    units = {(s, m) for s, modes in CONV_KERNEL_MODES.items() for m in modes}
    excluded = {(s, m) for s, m in units if s in CONV_KERNELS_NOT_REACHED}
    assert set(CONV_KERNELS_NOT_REACHED) <= set(CONV_KERNEL_MODES) and not (reached & excluded)
    assert reached | excluded == units, (sorted(units - reached - excluded), sorted(reached - units))


# ---- dense GEMM: what e4t_gemm_kernel / e4t_gemm_tn_kernel (the launcher's own decision: gemm.hip, decide_launch / resolve_tn) say every case of the
# GEMM checks runs, "<kernel symbol> splitk<n> <store path> [<reduce symbol>] [tail<r>]" -> the cases (kernel_checks.gemm_tag) it is pinned for.
# A planner or table change that moves a case off its kernel, its store path or its reduce kernel fails here.
CHECK_GEMM_KERNELS = {
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk1 bf16-staged": [
        "gemm 168x152x64 t128 s1 bare", "gemm 168x152x128 t128 s1 bare", "gemm 168x152x192 t128 s1 bare", "gemm 168x152x256 t128 s1 bare",
        "gemm 168x152x320 t128 s1 bare", "gemm 168x152x72 t128 s1 bare", "gemm 168x152x168 t128 s1 bare", "gemm 168x152x64 t128 s1 bias+res",
        "gemm 168x152x128 t128 s1 bias+res", "gemm 168x152x192 t128 s1 bias+res", "gemm 168x152x256 t128 s1 bias+res", "gemm 168x152x320 t128 s1 bias+res",
        "gemm 168x152x72 t128 s1 bias+res", "gemm 168x152x168 t128 s1 bias+res", "gemm 1x168x136 t128 s1 bare", "gemm 1x168x136 t128 s1 bias+res",
        "gemm 127x152x136 t128 s1 bare", "gemm 127x152x136 t128 s1 bias+res", "gemm 168x8x136 t128 s1 bare", "gemm 168x8x136 t128 s1 bias+res",
        "gemm 1192x280x136 t128 s1 bare", "gemm 1192x280x136 t128 s1 bias+res", "gemm 168x152x104 t128 s1 bare K1=64", "gemm 168x152x104 t128 s1 bias+res K1=64",
        "gemm 168x152x136 t128 s1 bare batch2", "gemm 168x152x136 t128 s1 bias batch2", "gemm 168x152x136 t128 s1 bare", "gemm 168x152x136 t128 s1 bias",
        "gemm 168x152x136 t128 s1 bias+res", "gemm 168x152x136 t128 s1 full", "gemm 168x152x136 t128 s1 alpha", "gemm 168x152x136 t128 s1 rowbias slice",
        "gemm 168x152x136 t128 s1 C slice8", "gemm 168x152x136 t128 s1 res slice", "gemm 160x152x136 t128 s1 colstats", "gemm 160x152x136 t128 s1 colstats+res",
        "gemm 168x152x136 t128 s1 bias misaligned",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk1 f32-direct": [
        "gemm 168x152x136 t128 s1 f32", "gemm 168x152x136 t128 s1 f32 res32", "gemm 168x152x136 t128 s1 f32 bare",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk1 scalar": [
        "gemm 168x148x136 t128 s1 bare", "gemm 168x148x136 t128 s1 bias+res", "gemm 168x152x136 t128 s1 f32 res16", "gemm 168x152x136 t128 s1 accum16",
        "gemm 168x152x136 t128 s1 accum32", "gemm 168x152x136 t128 s1 C slice4",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce4f_kernel": [
        "gemm 168x152x320 t128 s2 f32 bare",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x152x320 t128 s2 bare", "gemm 168x152x320 t128 s2 bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce_kernel": [
        "gemm 168x152x320 t128 s2 bias misaligned",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x152x192 t128 s3 bare", "gemm 168x152x192 t128 s3 bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, true, 64> splitk1 bf16-staged": [
        "gemm 168x152x64 t128 s1 gelu", "gemm 168x152x128 t128 s1 gelu", "gemm 168x152x192 t128 s1 gelu", "gemm 168x152x256 t128 s1 gelu",
        "gemm 168x152x320 t128 s1 gelu", "gemm 168x152x72 t128 s1 gelu", "gemm 168x152x168 t128 s1 gelu", "gemm 168x152x64 t128 s1 gelu+bias+res",
        "gemm 168x152x128 t128 s1 gelu+bias+res", "gemm 168x152x192 t128 s1 gelu+bias+res", "gemm 168x152x256 t128 s1 gelu+bias+res",
        "gemm 168x152x320 t128 s1 gelu+bias+res", "gemm 168x152x72 t128 s1 gelu+bias+res", "gemm 168x152x168 t128 s1 gelu+bias+res", "gemm 168x152x136 t128 s1 gelu",
        "gemm 168x152x136 t128 s1 gelu+bias+res", "gemm 168x152x136 t128 s1 general full", "gemm 168x152x136 t128 s1 rowbias24",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, true, 64> splitk1 scalar": [
        "gemm 168x152x136 t128 s1 gelu C slice4",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, true, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x152x320 t128 s2 gelu", "gemm 168x152x320 t128 s2 gelu+bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, true, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x152x192 t128 s3 gelu", "gemm 168x152x192 t128 s3 gelu+bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 3, false, 64> splitk1 bf16-staged": [
        "gemm 168x152x64 t3128 s1 bare", "gemm 168x152x128 t3128 s1 bare", "gemm 168x152x192 t3128 s1 bare", "gemm 168x152x256 t3128 s1 bare",
        "gemm 168x152x320 t3128 s1 bare", "gemm 168x152x384 t3128 s1 bare", "gemm 168x152x72 t3128 s1 bare", "gemm 168x152x232 t3128 s1 bare",
        "gemm 168x152x64 t3128 s1 bias+res", "gemm 168x152x128 t3128 s1 bias+res", "gemm 168x152x192 t3128 s1 bias+res", "gemm 168x152x256 t3128 s1 bias+res",
        "gemm 168x152x320 t3128 s1 bias+res", "gemm 168x152x384 t3128 s1 bias+res", "gemm 168x152x72 t3128 s1 bias+res", "gemm 168x152x232 t3128 s1 bias+res",
        "gemm 1x168x136 t3128 s1 bare", "gemm 1x168x136 t3128 s1 bias+res", "gemm 127x152x136 t3128 s1 bare", "gemm 127x152x136 t3128 s1 bias+res",
        "gemm 168x8x136 t3128 s1 bare", "gemm 168x8x136 t3128 s1 bias+res", "gemm 1192x280x136 t3128 s1 bare", "gemm 1192x280x136 t3128 s1 bias+res",
        "gemm 168x152x104 t3128 s1 bare K1=64", "gemm 168x152x104 t3128 s1 bias+res K1=64", "gemm 168x152x136 t3128 s1 bare batch2",
        "gemm 168x152x136 t3128 s1 bias batch2", "gemm 168x152x136 t3128 s1 bare", "gemm 168x152x136 t3128 s1 full",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 3, false, 64> splitk1 f32-direct": [
        "gemm 168x152x136 t3128 s1 f32 res32",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 3, false, 64> splitk1 scalar": [
        "gemm 168x148x136 t3128 s1 bare", "gemm 168x148x136 t3128 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 3, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x152x320 t3128 s2 bare", "gemm 168x152x320 t3128 s2 bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 3, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x152x192 t3128 s3 bare", "gemm 168x152x192 t3128 s3 bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 4, false, 64> splitk1 bf16-staged": [
        "gemm 168x152x64 t4128 s1 bare", "gemm 168x152x128 t4128 s1 bare", "gemm 168x152x192 t4128 s1 bare", "gemm 168x152x256 t4128 s1 bare",
        "gemm 168x152x320 t4128 s1 bare", "gemm 168x152x384 t4128 s1 bare", "gemm 168x152x448 t4128 s1 bare", "gemm 168x152x72 t4128 s1 bare",
        "gemm 168x152x296 t4128 s1 bare", "gemm 168x152x64 t4128 s1 bias+res", "gemm 168x152x128 t4128 s1 bias+res", "gemm 168x152x192 t4128 s1 bias+res",
        "gemm 168x152x256 t4128 s1 bias+res", "gemm 168x152x320 t4128 s1 bias+res", "gemm 168x152x384 t4128 s1 bias+res", "gemm 168x152x448 t4128 s1 bias+res",
        "gemm 168x152x72 t4128 s1 bias+res", "gemm 168x152x296 t4128 s1 bias+res", "gemm 1x168x136 t4128 s1 bare", "gemm 1x168x136 t4128 s1 bias+res",
        "gemm 127x152x136 t4128 s1 bare", "gemm 127x152x136 t4128 s1 bias+res", "gemm 168x8x136 t4128 s1 bare", "gemm 168x8x136 t4128 s1 bias+res",
        "gemm 1192x280x136 t4128 s1 bare", "gemm 1192x280x136 t4128 s1 bias+res", "gemm 168x152x104 t4128 s1 bare K1=64", "gemm 168x152x104 t4128 s1 bias+res K1=64",
        "gemm 168x152x136 t4128 s1 bare batch2", "gemm 168x152x136 t4128 s1 bias batch2", "gemm 168x152x136 t4128 s1 bare", "gemm 168x152x136 t4128 s1 full",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 4, false, 64> splitk1 f32-direct": [
        "gemm 168x152x136 t4128 s1 f32 res32",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 4, false, 64> splitk1 scalar": [
        "gemm 168x148x136 t4128 s1 bare", "gemm 168x148x136 t4128 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 4, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x152x320 t4128 s2 bare", "gemm 168x152x320 t4128 s2 bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 4, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x152x192 t4128 s3 bare", "gemm 168x152x192 t4128 s3 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 bf16-staged": [
        "gemm 168x184x64 t160 s1 bare", "gemm 168x184x128 t160 s1 bare", "gemm 168x184x192 t160 s1 bare", "gemm 168x184x256 t160 s1 bare",
        "gemm 168x184x320 t160 s1 bare", "gemm 168x184x72 t160 s1 bare", "gemm 168x184x168 t160 s1 bare", "gemm 168x184x64 t160 s1 bias+res",
        "gemm 168x184x128 t160 s1 bias+res", "gemm 168x184x192 t160 s1 bias+res", "gemm 168x184x256 t160 s1 bias+res", "gemm 168x184x320 t160 s1 bias+res",
        "gemm 168x184x72 t160 s1 bias+res", "gemm 168x184x168 t160 s1 bias+res", "gemm 1x200x136 t160 s1 bare", "gemm 1x200x136 t160 s1 bias+res",
        "gemm 127x184x136 t160 s1 bare", "gemm 127x184x136 t160 s1 bias+res", "gemm 168x8x136 t160 s1 bare", "gemm 168x8x136 t160 s1 bias+res",
        "gemm 1192x344x136 t160 s1 bare", "gemm 1192x344x136 t160 s1 bias+res", "gemm 168x184x104 t160 s1 bare K1=64", "gemm 168x184x104 t160 s1 bias+res K1=64",
        "gemm 168x184x136 t160 s1 bare batch2", "gemm 168x184x136 t160 s1 bias batch2", "gemm 168x184x136 t160 s1 bare", "gemm 168x184x136 t160 s1 bias",
        "gemm 168x184x136 t160 s1 bias+res", "gemm 168x184x136 t160 s1 full", "gemm 168x184x136 t160 s1 alpha", "gemm 168x184x136 t160 s1 rowbias slice",
        "gemm 168x184x136 t160 s1 C slice8", "gemm 168x184x136 t160 s1 res slice", "gemm 160x184x136 t160 s1 colstats", "gemm 160x184x136 t160 s1 colstats+res",
        "gemm 168x184x136 t160 s1 bias misaligned",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 bf16-staged tail1": [
        "gemm 1153x320x144 t160 s1 bare", "gemm 1153x320x144 t160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 bf16-staged tail17": [
        "gemm 1169x320x144 t160 s1 bare", "gemm 1169x320x144 t160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 bf16-staged tail32": [
        "gemm 1184x320x144 t160 s1 bare", "gemm 1184x320x144 t160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 f32-direct": [
        "gemm 168x184x136 t160 s1 f32", "gemm 168x184x136 t160 s1 f32 res32", "gemm 168x184x136 t160 s1 f32 bare",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 scalar": [
        "gemm 168x180x136 t160 s1 bare", "gemm 168x180x136 t160 s1 bias+res", "gemm 168x184x136 t160 s1 f32 res16", "gemm 168x184x136 t160 s1 accum16",
        "gemm 168x184x136 t160 s1 accum32", "gemm 168x184x136 t160 s1 C slice4",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce4f_kernel": [
        "gemm 168x184x320 t160 s2 f32 bare",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x184x320 t160 s2 bare", "gemm 168x184x320 t160 s2 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce_kernel": [
        "gemm 168x184x320 t160 s2 bias misaligned",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x184x192 t160 s3 bare", "gemm 168x184x192 t160 s3 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, true, 64> splitk1 bf16-staged": [
        "gemm 168x184x64 t160 s1 gelu", "gemm 168x184x128 t160 s1 gelu", "gemm 168x184x192 t160 s1 gelu", "gemm 168x184x256 t160 s1 gelu",
        "gemm 168x184x320 t160 s1 gelu", "gemm 168x184x72 t160 s1 gelu", "gemm 168x184x168 t160 s1 gelu", "gemm 168x184x64 t160 s1 gelu+bias+res",
        "gemm 168x184x128 t160 s1 gelu+bias+res", "gemm 168x184x192 t160 s1 gelu+bias+res", "gemm 168x184x256 t160 s1 gelu+bias+res",
        "gemm 168x184x320 t160 s1 gelu+bias+res", "gemm 168x184x72 t160 s1 gelu+bias+res", "gemm 168x184x168 t160 s1 gelu+bias+res", "gemm 168x184x136 t160 s1 gelu",
        "gemm 168x184x136 t160 s1 gelu+bias+res", "gemm 168x184x136 t160 s1 general full", "gemm 168x184x136 t160 s1 rowbias24",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, true, 64> splitk1 scalar": [
        "gemm 168x184x136 t160 s1 gelu C slice4",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, true, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x184x320 t160 s2 gelu", "gemm 168x184x320 t160 s2 gelu+bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, true, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x184x192 t160 s3 gelu", "gemm 168x184x192 t160 s3 gelu+bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk1 bf16-staged": [
        "gemm 168x184x64 t3160 s1 bare", "gemm 168x184x128 t3160 s1 bare", "gemm 168x184x192 t3160 s1 bare", "gemm 168x184x256 t3160 s1 bare",
        "gemm 168x184x320 t3160 s1 bare", "gemm 168x184x384 t3160 s1 bare", "gemm 168x184x72 t3160 s1 bare", "gemm 168x184x232 t3160 s1 bare",
        "gemm 168x184x64 t3160 s1 bias+res", "gemm 168x184x128 t3160 s1 bias+res", "gemm 168x184x192 t3160 s1 bias+res", "gemm 168x184x256 t3160 s1 bias+res",
        "gemm 168x184x320 t3160 s1 bias+res", "gemm 168x184x384 t3160 s1 bias+res", "gemm 168x184x72 t3160 s1 bias+res", "gemm 168x184x232 t3160 s1 bias+res",
        "gemm 1x200x136 t3160 s1 bare", "gemm 1x200x136 t3160 s1 bias+res", "gemm 127x184x136 t3160 s1 bare", "gemm 127x184x136 t3160 s1 bias+res",
        "gemm 168x8x136 t3160 s1 bare", "gemm 168x8x136 t3160 s1 bias+res", "gemm 1192x344x136 t3160 s1 bare", "gemm 1192x344x136 t3160 s1 bias+res",
        "gemm 168x184x104 t3160 s1 bare K1=64", "gemm 168x184x104 t3160 s1 bias+res K1=64", "gemm 168x184x136 t3160 s1 bare batch2",
        "gemm 168x184x136 t3160 s1 bias batch2", "gemm 168x184x136 t3160 s1 bare", "gemm 168x184x136 t3160 s1 full",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk1 bf16-staged tail1": [
        "gemm 1153x320x144 t3160 s1 bare", "gemm 1153x320x144 t3160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk1 bf16-staged tail17": [
        "gemm 1169x320x144 t3160 s1 bare", "gemm 1169x320x144 t3160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk1 bf16-staged tail32": [
        "gemm 1184x320x144 t3160 s1 bare", "gemm 1184x320x144 t3160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk1 f32-direct": [
        "gemm 168x184x136 t3160 s1 f32 res32",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk1 scalar": [
        "gemm 168x180x136 t3160 s1 bare", "gemm 168x180x136 t3160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x184x320 t3160 s2 bare", "gemm 168x184x320 t3160 s2 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x184x192 t3160 s3 bare", "gemm 168x184x192 t3160 s3 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64> splitk1 bf16-staged": [
        "gemm 168x184x64 t4160 s1 bare", "gemm 168x184x128 t4160 s1 bare", "gemm 168x184x192 t4160 s1 bare", "gemm 168x184x256 t4160 s1 bare",
        "gemm 168x184x320 t4160 s1 bare", "gemm 168x184x384 t4160 s1 bare", "gemm 168x184x448 t4160 s1 bare", "gemm 168x184x72 t4160 s1 bare",
        "gemm 168x184x296 t4160 s1 bare", "gemm 168x184x64 t4160 s1 bias+res", "gemm 168x184x128 t4160 s1 bias+res", "gemm 168x184x192 t4160 s1 bias+res",
        "gemm 168x184x256 t4160 s1 bias+res", "gemm 168x184x320 t4160 s1 bias+res", "gemm 168x184x384 t4160 s1 bias+res", "gemm 168x184x448 t4160 s1 bias+res",
        "gemm 168x184x72 t4160 s1 bias+res", "gemm 168x184x296 t4160 s1 bias+res", "gemm 1x200x136 t4160 s1 bare", "gemm 1x200x136 t4160 s1 bias+res",
        "gemm 127x184x136 t4160 s1 bare", "gemm 127x184x136 t4160 s1 bias+res", "gemm 168x8x136 t4160 s1 bare", "gemm 168x8x136 t4160 s1 bias+res",
        "gemm 1192x344x136 t4160 s1 bare", "gemm 1192x344x136 t4160 s1 bias+res", "gemm 168x184x104 t4160 s1 bare K1=64", "gemm 168x184x104 t4160 s1 bias+res K1=64",
        "gemm 168x184x136 t4160 s1 bare batch2", "gemm 168x184x136 t4160 s1 bias batch2", "gemm 168x184x136 t4160 s1 bare", "gemm 168x184x136 t4160 s1 full",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64> splitk1 bf16-staged tail1": [
        "gemm 1153x320x144 t4160 s1 bare", "gemm 1153x320x144 t4160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64> splitk1 bf16-staged tail17": [
        "gemm 1169x320x144 t4160 s1 bare", "gemm 1169x320x144 t4160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64> splitk1 bf16-staged tail32": [
        "gemm 1184x320x144 t4160 s1 bare", "gemm 1184x320x144 t4160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64> splitk1 f32-direct": [
        "gemm 168x184x136 t4160 s1 f32 res32",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64> splitk1 scalar": [
        "gemm 168x180x136 t4160 s1 bare", "gemm 168x180x136 t4160 s1 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x184x320 t4160 s2 bare", "gemm 168x184x320 t4160 s2 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 168x184x192 t4160 s3 bare", "gemm 168x184x192 t4160 s3 bias+res",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk1 bf16-staged": [
        "gemm 296x152x32 t5256 s1 bare", "gemm 296x152x64 t5256 s1 bare", "gemm 296x152x96 t5256 s1 bare", "gemm 296x152x128 t5256 s1 bare",
        "gemm 296x152x160 t5256 s1 bare", "gemm 296x152x192 t5256 s1 bare", "gemm 296x152x72 t5256 s1 bare", "gemm 296x152x232 t5256 s1 bare",
        "gemm 296x152x88 t5256 s1 bare", "gemm 296x152x112 t5256 s1 bare", "gemm 296x152x32 t5256 s1 bias+res", "gemm 296x152x64 t5256 s1 bias+res",
        "gemm 296x152x96 t5256 s1 bias+res", "gemm 296x152x128 t5256 s1 bias+res", "gemm 296x152x160 t5256 s1 bias+res", "gemm 296x152x192 t5256 s1 bias+res",
        "gemm 296x152x72 t5256 s1 bias+res", "gemm 296x152x232 t5256 s1 bias+res", "gemm 296x152x88 t5256 s1 bias+res", "gemm 296x152x112 t5256 s1 bias+res",
        "gemm 1x168x136 t5256 s1 bare", "gemm 1x168x136 t5256 s1 bias+res", "gemm 255x152x136 t5256 s1 bare", "gemm 255x152x136 t5256 s1 bias+res",
        "gemm 296x8x136 t5256 s1 bare", "gemm 296x8x136 t5256 s1 bias+res", "gemm 2344x280x136 t5256 s1 bare", "gemm 2344x280x136 t5256 s1 bias+res",
        "gemm 296x152x104 t5256 s1 bare K1=64", "gemm 296x152x104 t5256 s1 bias+res K1=64", "gemm 296x152x136 t5256 s1 bare batch2",
        "gemm 296x152x136 t5256 s1 bias batch2", "gemm 296x152x136 t5256 s1 bare", "gemm 296x152x136 t5256 s1 bias", "gemm 296x152x136 t5256 s1 bias+res",
        "gemm 296x152x136 t5256 s1 full", "gemm 296x152x136 t5256 s1 alpha", "gemm 296x152x136 t5256 s1 rowbias slice", "gemm 296x152x136 t5256 s1 C slice8",
        "gemm 296x152x136 t5256 s1 res slice", "gemm 288x152x136 t5256 s1 colstats", "gemm 288x152x136 t5256 s1 colstats+res",
        "gemm 296x152x136 t5256 s1 bias misaligned",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk1 f32-direct": [
        "gemm 296x152x136 t5256 s1 f32", "gemm 296x152x136 t5256 s1 f32 res32", "gemm 296x152x136 t5256 s1 f32 bare",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk1 scalar": [
        "gemm 296x148x136 t5256 s1 bare", "gemm 296x148x136 t5256 s1 bias+res", "gemm 296x152x136 t5256 s1 f32 res16", "gemm 296x152x136 t5256 s1 accum16",
        "gemm 296x152x136 t5256 s1 accum32", "gemm 296x152x136 t5256 s1 C slice4",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk2 splitk-partial splitk_reduce4f_kernel": [
        "gemm 296x152x320 t5256 s2 f32 bare",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x152x320 t5256 s2 bare", "gemm 296x152x320 t5256 s2 bias+res",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk2 splitk-partial splitk_reduce_kernel": [
        "gemm 296x152x320 t5256 s2 bias misaligned",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x152x192 t5256 s3 bare", "gemm 296x152x192 t5256 s3 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk1 bf16-staged": [
        "gemm 104x88x64 t64 s1 bare", "gemm 104x88x128 t64 s1 bare", "gemm 104x88x192 t64 s1 bare", "gemm 104x88x256 t64 s1 bare", "gemm 104x88x320 t64 s1 bare",
        "gemm 104x88x72 t64 s1 bare", "gemm 104x88x168 t64 s1 bare", "gemm 104x88x64 t64 s1 bias+res", "gemm 104x88x128 t64 s1 bias+res",
        "gemm 104x88x192 t64 s1 bias+res", "gemm 104x88x256 t64 s1 bias+res", "gemm 104x88x320 t64 s1 bias+res", "gemm 104x88x72 t64 s1 bias+res",
        "gemm 104x88x168 t64 s1 bias+res", "gemm 1x104x136 t64 s1 bare", "gemm 1x104x136 t64 s1 bias+res", "gemm 63x88x136 t64 s1 bare",
        "gemm 63x88x136 t64 s1 bias+res", "gemm 104x8x136 t64 s1 bare", "gemm 104x8x136 t64 s1 bias+res", "gemm 616x152x136 t64 s1 bare",
        "gemm 616x152x136 t64 s1 bias+res", "gemm 104x88x104 t64 s1 bare K1=64", "gemm 104x88x104 t64 s1 bias+res K1=64", "gemm 104x88x136 t64 s1 bare batch2",
        "gemm 104x88x136 t64 s1 bias batch2", "gemm 104x88x136 t64 s1 bare", "gemm 104x88x136 t64 s1 bias", "gemm 104x88x136 t64 s1 bias+res",
        "gemm 104x88x136 t64 s1 full", "gemm 104x88x136 t64 s1 alpha", "gemm 104x88x136 t64 s1 rowbias slice", "gemm 104x88x136 t64 s1 C slice8",
        "gemm 104x88x136 t64 s1 res slice", "gemm 96x88x136 t64 s1 colstats", "gemm 96x88x136 t64 s1 colstats+res", "gemm 104x88x136 t64 s1 bias misaligned",
        "gemm 104x88x104 t64 s1 full K1=64",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk1 f32-direct": [
        "gemm 104x88x136 t64 s1 f32", "gemm 104x88x136 t64 s1 f32 res32", "gemm 104x88x136 t64 s1 f32 bare",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk1 scalar": [
        "gemm 104x84x136 t64 s1 bare", "gemm 104x84x136 t64 s1 bias+res", "gemm 104x88x136 t64 s1 f32 res16", "gemm 104x88x136 t64 s1 accum16",
        "gemm 104x88x136 t64 s1 accum32", "gemm 104x88x136 t64 s1 C slice4",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce4f_kernel": [
        "gemm 104x88x320 t64 s2 f32 bare",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x320 t64 s2 bare", "gemm 104x88x320 t64 s2 bias+res", "gemm 104x88x320 t64 s2 full", "gemm 104x88x2048 t64 s0 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce_kernel": [
        "gemm 104x88x320 t64 s2 bias misaligned",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x192 t64 s3 bare", "gemm 104x88x192 t64 s3 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, true, 64> splitk1 bf16-staged": [
        "gemm 104x88x64 t64 s1 gelu", "gemm 104x88x128 t64 s1 gelu", "gemm 104x88x192 t64 s1 gelu", "gemm 104x88x256 t64 s1 gelu", "gemm 104x88x320 t64 s1 gelu",
        "gemm 104x88x72 t64 s1 gelu", "gemm 104x88x168 t64 s1 gelu", "gemm 104x88x64 t64 s1 gelu+bias+res", "gemm 104x88x128 t64 s1 gelu+bias+res",
        "gemm 104x88x192 t64 s1 gelu+bias+res", "gemm 104x88x256 t64 s1 gelu+bias+res", "gemm 104x88x320 t64 s1 gelu+bias+res", "gemm 104x88x72 t64 s1 gelu+bias+res",
        "gemm 104x88x168 t64 s1 gelu+bias+res", "gemm 104x88x136 t64 s1 gelu", "gemm 104x88x136 t64 s1 gelu+bias+res", "gemm 104x88x136 t64 s1 general full",
        "gemm 104x88x136 t64 s1 rowbias24",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, true, 64> splitk1 scalar": [
        "gemm 104x88x136 t64 s1 gelu C slice4",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, true, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x320 t64 s2 gelu", "gemm 104x88x320 t64 s2 gelu+bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, true, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x192 t64 s3 gelu", "gemm 104x88x192 t64 s3 gelu+bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, false, 64> splitk1 bf16-staged": [
        "gemm 104x88x64 t3064 s1 bare", "gemm 104x88x128 t3064 s1 bare", "gemm 104x88x192 t3064 s1 bare", "gemm 104x88x256 t3064 s1 bare",
        "gemm 104x88x320 t3064 s1 bare", "gemm 104x88x384 t3064 s1 bare", "gemm 104x88x72 t3064 s1 bare", "gemm 104x88x232 t3064 s1 bare",
        "gemm 104x88x64 t3064 s1 bias+res", "gemm 104x88x128 t3064 s1 bias+res", "gemm 104x88x192 t3064 s1 bias+res", "gemm 104x88x256 t3064 s1 bias+res",
        "gemm 104x88x320 t3064 s1 bias+res", "gemm 104x88x384 t3064 s1 bias+res", "gemm 104x88x72 t3064 s1 bias+res", "gemm 104x88x232 t3064 s1 bias+res",
        "gemm 1x104x136 t3064 s1 bare", "gemm 1x104x136 t3064 s1 bias+res", "gemm 63x88x136 t3064 s1 bare", "gemm 63x88x136 t3064 s1 bias+res",
        "gemm 104x8x136 t3064 s1 bare", "gemm 104x8x136 t3064 s1 bias+res", "gemm 616x152x136 t3064 s1 bare", "gemm 616x152x136 t3064 s1 bias+res",
        "gemm 104x88x104 t3064 s1 bare K1=64", "gemm 104x88x104 t3064 s1 bias+res K1=64", "gemm 104x88x136 t3064 s1 bare batch2", "gemm 104x88x136 t3064 s1 bias batch2",
        "gemm 104x88x136 t3064 s1 bare", "gemm 104x88x136 t3064 s1 full",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, false, 64> splitk1 f32-direct": [
        "gemm 104x88x136 t3064 s1 f32 res32",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, false, 64> splitk1 scalar": [
        "gemm 104x84x136 t3064 s1 bare", "gemm 104x84x136 t3064 s1 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x320 t3064 s2 bare", "gemm 104x88x320 t3064 s2 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x192 t3064 s3 bare", "gemm 104x88x192 t3064 s3 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, true, 64> splitk1 bf16-staged": [
        "gemm 104x88x64 t3064 s1 gelu", "gemm 104x88x128 t3064 s1 gelu", "gemm 104x88x192 t3064 s1 gelu", "gemm 104x88x256 t3064 s1 gelu",
        "gemm 104x88x320 t3064 s1 gelu", "gemm 104x88x384 t3064 s1 gelu", "gemm 104x88x72 t3064 s1 gelu", "gemm 104x88x232 t3064 s1 gelu",
        "gemm 104x88x64 t3064 s1 gelu+bias+res", "gemm 104x88x128 t3064 s1 gelu+bias+res", "gemm 104x88x192 t3064 s1 gelu+bias+res",
        "gemm 104x88x256 t3064 s1 gelu+bias+res", "gemm 104x88x320 t3064 s1 gelu+bias+res", "gemm 104x88x384 t3064 s1 gelu+bias+res",
        "gemm 104x88x72 t3064 s1 gelu+bias+res", "gemm 104x88x232 t3064 s1 gelu+bias+res", "gemm 104x88x136 t3064 s1 gelu", "gemm 104x88x136 t3064 s1 general full",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, true, 64> splitk1 scalar": [
        "gemm 104x88x136 t3064 s1 gelu C slice4",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, true, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x320 t3064 s2 gelu", "gemm 104x88x320 t3064 s2 gelu+bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, true, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x192 t3064 s3 gelu", "gemm 104x88x192 t3064 s3 gelu+bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64> splitk1 bf16-staged": [
        "gemm 104x88x64 t4064 s1 bare", "gemm 104x88x128 t4064 s1 bare", "gemm 104x88x192 t4064 s1 bare", "gemm 104x88x256 t4064 s1 bare",
        "gemm 104x88x320 t4064 s1 bare", "gemm 104x88x384 t4064 s1 bare", "gemm 104x88x448 t4064 s1 bare", "gemm 104x88x72 t4064 s1 bare",
        "gemm 104x88x296 t4064 s1 bare", "gemm 104x88x64 t4064 s1 bias+res", "gemm 104x88x128 t4064 s1 bias+res", "gemm 104x88x192 t4064 s1 bias+res",
        "gemm 104x88x256 t4064 s1 bias+res", "gemm 104x88x320 t4064 s1 bias+res", "gemm 104x88x384 t4064 s1 bias+res", "gemm 104x88x448 t4064 s1 bias+res",
        "gemm 104x88x72 t4064 s1 bias+res", "gemm 104x88x296 t4064 s1 bias+res", "gemm 1x104x136 t4064 s1 bare", "gemm 1x104x136 t4064 s1 bias+res",
        "gemm 63x88x136 t4064 s1 bare", "gemm 63x88x136 t4064 s1 bias+res", "gemm 104x8x136 t4064 s1 bare", "gemm 104x8x136 t4064 s1 bias+res",
        "gemm 616x152x136 t4064 s1 bare", "gemm 616x152x136 t4064 s1 bias+res", "gemm 104x88x104 t4064 s1 bare K1=64", "gemm 104x88x104 t4064 s1 bias+res K1=64",
        "gemm 104x88x136 t4064 s1 bare batch2", "gemm 104x88x136 t4064 s1 bias batch2", "gemm 104x88x136 t4064 s1 bare", "gemm 104x88x136 t4064 s1 full",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64> splitk1 f32-direct": [
        "gemm 104x88x136 t4064 s1 f32 res32",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64> splitk1 scalar": [
        "gemm 104x84x136 t4064 s1 bare", "gemm 104x84x136 t4064 s1 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x320 t4064 s2 bare", "gemm 104x88x320 t4064 s2 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 104x88x192 t4064 s3 bare", "gemm 104x88x192 t4064 s3 bias+res",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 bf16-staged": [
        "gemm 296x280x64 t512 s1 bare", "gemm 296x280x128 t512 s1 bare", "gemm 296x280x192 t512 s1 bare", "gemm 296x280x256 t512 s1 bare",
        "gemm 296x280x320 t512 s1 bare", "gemm 296x280x64 t512 s1 bias+res", "gemm 296x280x128 t512 s1 bias+res", "gemm 296x280x192 t512 s1 bias+res",
        "gemm 296x280x256 t512 s1 bias+res", "gemm 296x280x320 t512 s1 bias+res", "gemm 1x296x128 t512 s1 bare", "gemm 1x296x128 t512 s1 bias+res",
        "gemm 255x280x128 t512 s1 bare", "gemm 255x280x128 t512 s1 bias+res", "gemm 296x8x128 t512 s1 bare", "gemm 296x8x128 t512 s1 bias+res",
        "gemm 2344x536x128 t512 s1 bare", "gemm 2344x536x128 t512 s1 bias+res", "gemm 296x280x128 t512 s1 bare K1=64", "gemm 296x280x128 t512 s1 bias+res K1=64",
        "gemm 296x280x128 t512 s1 bare batch2", "gemm 296x280x128 t512 s1 bias batch2", "gemm 296x280x128 t512 s1 bias", "gemm 296x280x128 t512 s1 full",
        "gemm 296x280x128 t512 s1 alpha", "gemm 296x280x128 t512 s1 rowbias slice", "gemm 296x280x128 t512 s1 C slice8", "gemm 296x280x128 t512 s1 res slice",
        "gemm 288x280x128 t512 s1 colstats", "gemm 288x280x128 t512 s1 colstats+res", "gemm 296x280x128 t512 s1 bias misaligned", "gemm 296x280x128 t512 s1 full K1=64",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 bf16-staged tail1": [
        "gemm 1153x320x128 t512 s1 bare", "gemm 1153x320x128 t512 s1 bias+res",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 bf16-staged tail17": [
        "gemm 1169x320x128 t512 s1 bare", "gemm 1169x320x128 t512 s1 bias+res",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 bf16-staged tail32": [
        "gemm 1184x320x128 t512 s1 bare", "gemm 1184x320x128 t512 s1 bias+res",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 f32-direct": [
        "gemm 296x280x128 t512 s1 f32", "gemm 296x280x128 t512 s1 f32 res32", "gemm 296x280x128 t512 s1 f32 bare",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 scalar": [
        "gemm 296x276x128 t512 s1 bare", "gemm 296x276x128 t512 s1 bias+res", "gemm 296x280x128 t512 s1 f32 res16", "gemm 296x280x128 t512 s1 accum16",
        "gemm 296x280x128 t512 s1 accum32", "gemm 296x280x128 t512 s1 C slice4",
    ],
    "gemm_pp_kernel<0, false, false> splitk2 splitk-partial splitk_reduce4f_kernel": [
        "gemm 296x280x320 t512 s2 f32 bare",
    ],
    "gemm_pp_kernel<0, false, false> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x280x320 t512 s2 bare", "gemm 296x280x320 t512 s2 bias+res",
    ],
    "gemm_pp_kernel<0, false, false> splitk2 splitk-partial splitk_reduce_kernel": [
        "gemm 296x280x320 t512 s2 bias misaligned",
    ],
    "gemm_pp_kernel<0, false, false> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x280x192 t512 s3 bare", "gemm 296x280x192 t512 s3 bias+res",
    ],
    "gemm_pp_kernel<0, true, false> splitk1 bf16-staged": [
        "gemm 296x280x64 t512 s1 gelu", "gemm 296x280x128 t512 s1 gelu", "gemm 296x280x192 t512 s1 gelu", "gemm 296x280x256 t512 s1 gelu",
        "gemm 296x280x320 t512 s1 gelu", "gemm 296x280x64 t512 s1 gelu+bias+res", "gemm 296x280x128 t512 s1 gelu+bias+res", "gemm 296x280x192 t512 s1 gelu+bias+res",
        "gemm 296x280x256 t512 s1 gelu+bias+res", "gemm 296x280x320 t512 s1 gelu+bias+res", "gemm 296x280x128 t512 s1 general full",
        "gemm 296x280x128 t512 s1 rowbias24",
    ],
    "gemm_pp_kernel<0, true, false> splitk1 scalar": [
        "gemm 296x280x128 t512 s1 gelu C slice4",
    ],
    "gemm_pp_kernel<0, true, false> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x280x320 t512 s2 gelu", "gemm 296x280x320 t512 s2 gelu+bias+res",
    ],
    "gemm_pp_kernel<0, true, false> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x280x192 t512 s3 gelu", "gemm 296x280x192 t512 s3 gelu+bias+res",
    ],
    "gemm_pq_kernel<0, 320, false> splitk1 bf16-staged": [
        "gemm 296x640x64 t2320 s1 bare", "gemm 296x640x128 t2320 s1 bare", "gemm 296x640x192 t2320 s1 bare", "gemm 296x640x256 t2320 s1 bare",
        "gemm 296x640x320 t2320 s1 bare", "gemm 296x640x64 t2320 s1 bias+res", "gemm 296x640x128 t2320 s1 bias+res", "gemm 296x640x192 t2320 s1 bias+res",
        "gemm 296x640x256 t2320 s1 bias+res", "gemm 296x640x320 t2320 s1 bias+res", "gemm 1x640x128 t2320 s1 bare", "gemm 1x640x128 t2320 s1 bias+res",
        "gemm 255x640x128 t2320 s1 bare", "gemm 255x640x128 t2320 s1 bias+res", "gemm 2344x960x128 t2320 s1 bare", "gemm 2344x960x128 t2320 s1 bias+res",
        "gemm 296x640x128 t2320 s1 bare K1=64", "gemm 296x640x128 t2320 s1 bias+res K1=64", "gemm 296x640x128 t2320 s1 bare batch2",
        "gemm 296x640x128 t2320 s1 bias batch2", "gemm 296x640x128 t2320 s1 bias", "gemm 296x640x128 t2320 s1 full", "gemm 296x640x128 t2320 s1 alpha",
        "gemm 296x640x128 t2320 s1 rowbias slice", "gemm 296x640x128 t2320 s1 C slice8", "gemm 296x640x128 t2320 s1 res slice", "gemm 288x640x128 t2320 s1 colstats",
        "gemm 288x640x128 t2320 s1 colstats+res", "gemm 296x640x128 t2320 s1 bias misaligned",
    ],
    "gemm_pq_kernel<0, 320, false> splitk1 bf16-staged tail1": [
        "gemm 1153x320x128 t2320 s1 bare", "gemm 1153x320x128 t2320 s1 bias+res",
    ],
    "gemm_pq_kernel<0, 320, false> splitk1 bf16-staged tail17": [
        "gemm 1169x320x128 t2320 s1 bare", "gemm 1169x320x128 t2320 s1 bias+res",
    ],
    "gemm_pq_kernel<0, 320, false> splitk1 bf16-staged tail32": [
        "gemm 1184x320x128 t2320 s1 bare", "gemm 1184x320x128 t2320 s1 bias+res",
    ],
    "gemm_pq_kernel<0, 320, false> splitk1 f32-direct": [
        "gemm 296x640x128 t2320 s1 f32", "gemm 296x640x128 t2320 s1 f32 res32", "gemm 296x640x128 t2320 s1 f32 bare",
    ],
    "gemm_pq_kernel<0, 320, false> splitk1 scalar": [
        "gemm 296x640x128 t2320 s1 f32 res16", "gemm 296x640x128 t2320 s1 accum16", "gemm 296x640x128 t2320 s1 accum32", "gemm 296x640x128 t2320 s1 C slice4",
    ],
    "gemm_pq_kernel<0, 320, false> splitk2 splitk-partial splitk_reduce4f_kernel": [
        "gemm 296x640x320 t2320 s2 f32 bare",
    ],
    "gemm_pq_kernel<0, 320, false> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x640x320 t2320 s2 bare", "gemm 296x640x320 t2320 s2 bias+res",
    ],
    "gemm_pq_kernel<0, 320, false> splitk2 splitk-partial splitk_reduce_kernel": [
        "gemm 296x640x320 t2320 s2 bias misaligned",
    ],
    "gemm_pq_kernel<0, 320, false> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x640x192 t2320 s3 bare", "gemm 296x640x192 t2320 s3 bias+res",
    ],
    "gemm_pq_kernel<0, 320, true> splitk1 bf16-staged": [
        "gemm 296x640x64 t2320 s1 gelu", "gemm 296x640x128 t2320 s1 gelu", "gemm 296x640x192 t2320 s1 gelu", "gemm 296x640x256 t2320 s1 gelu",
        "gemm 296x640x320 t2320 s1 gelu", "gemm 296x640x64 t2320 s1 gelu+bias+res", "gemm 296x640x128 t2320 s1 gelu+bias+res", "gemm 296x640x192 t2320 s1 gelu+bias+res",
        "gemm 296x640x256 t2320 s1 gelu+bias+res", "gemm 296x640x320 t2320 s1 gelu+bias+res", "gemm 296x640x128 t2320 s1 general full",
        "gemm 296x640x128 t2320 s1 rowbias24",
    ],
    "gemm_pq_kernel<0, 320, true> splitk1 scalar": [
        "gemm 296x640x128 t2320 s1 gelu C slice4",
    ],
    "gemm_pq_kernel<0, 320, true> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x640x320 t2320 s2 gelu", "gemm 296x640x320 t2320 s2 gelu+bias+res",
    ],
    "gemm_pq_kernel<0, 320, true> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 296x640x192 t2320 s3 gelu", "gemm 296x640x192 t2320 s3 gelu+bias+res",
    ],
    "gemm_tn_kernel splitk1 bf16-staged": [
        "gemm_tn K200 M168 N152 s1 bf16",
    ],
    "gemm_tn_kernel splitk1 scalar": [
        "gemm_tn K200 M168 N152 s1 f32", "gemm_tn K136 M8 N152 s1 f32", "gemm_tn K200 M168 N152 s1 lda", "gemm_tn K200 M168 N152 s1 C slice",
        "gemm_tn K200 M168 N152 s1 accum", "gemm_tn K200 M168 N152 s1 alpha",
    ],
    "gemm_tn_kernel splitk2 splitk-partial splitk_reduce4f_kernel": [
        "gemm_tn K300 M168 N152 s2 f32", "gemm_tn K2048 M136 N136 s0 f32", "gemm_tn K300 M168 N152 s2 accum",
    ],
    "gemm_tn_kernel splitk2 splitk-partial splitk_reduce_kernel": [
        "gemm_tn K300 M168 N152 s2 bf16",
    ],
}

CHECK_GEMM_EXISTING_KERNELS = {
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk1 bf16-staged": [
        "gemm 1000x320x320 t128 s1 bias+res", "gemm 300x200x64 t2320 s1 bias+res", "gemm 1024x640x1280 t128 colstats + residual",
        "gemm 8192x256x128 t128 colstats + residual", "gemm 34816x128x64 t128 colstats + residual", "gemm two-source A t2320",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 513x1000x1152 t2320 s2 bias+res",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 2056x1280x5120 tail bias",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, true, 64> splitk1 bf16-staged": [
        "gemm gelu t2320",
    ],
    "gemm_dma_kernel<128, 128, 4, 2, 0, 4, false, 64> splitk1 bf16-staged": [
        "gemm 4096x640x2560 t0 s0 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 bf16-staged": [
        "gemm 900x320x384 t160 s1 bias+res", "gemm 513x200x72 t160 s1 bias+res", "gemm 4096x320x320 t160 colstats", "gemm 66560x640x192 t160 colstats",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 bf16-staged tail32": [
        "gemm 8224x1280x1280 tail bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk1 f32-direct": [
        "gemm 1000x1280x320 t160 fp32 out + fp32 residual",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 300x480x128 t160 s2 bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk1 bf16-staged tail1": [
        "gemm 4097x1280x1280 tail bias+res",
    ],
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64> splitk1 f32-direct tail16": [
        "gemm 4112x1280x1280 tail f32 res32", "gemm 4112x1280x5120 tail f32 res32", "gemm 4112x1280x1296 tail f32 res32",
        "gemm 4112x1280x1280 t0 fp32 out + fp32 residual", "gemm 4112x1280x5120 t0 fp32 out + fp32 residual",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk1 bf16-staged": [
        "gemm 1000x200x328 t256 s1 bias+res", "gemm 2048x256x64 t256 s1 bias+res", "gemm 900x384x512 t5256 s1 bias+res", "gemm 5000x640x320 t5256 s1 bias+res",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk1 f32-direct": [
        "gemm 900x384x96 t5256 fp32 out + fp32 residual",
    ],
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 700x320x1280 t256 s2 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk1 bf16-staged": [
        "gemm 192x72x64 t64 colstats + residual", "gemm batched", "gemm batched broadcast A",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk1 f32-direct": [
        "gemm 513x200x64 t64 fp32 out + fp32 residual",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk1 splitk-partial splitk_reduce4f_kernel": [
        "gemm batched reduce (mean over slots)",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 130x200x1032 t64 s3 bias+res",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, false, 64> splitk1 bf16-staged": [
        "gemm two-source A t3064",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, true, 64> splitk1 bf16-staged": [
        "gemm gelu", "gemm gelu t3064",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64> splitk1 bf16-staged": [
        "gemm 256x256x128 t0 s0 bias+res", "gemm 200x72x64 t0 s0 bias+res", "gemm 16x1280x1280 t0 s0 bias+res", "gemm 256x128x128 t0 colstats + residual",
        "gemm two-source A", "gemm rowbias", "gemm strided A view",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64> splitk1 scalar": [
        "gemm fp32 out + accumulate + alpha",
    ],
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64> splitk11 splitk-partial splitk_reduce8_kernel": [
        "gemm 64x64x4096 t0 s0 bias+res",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 bf16-staged": [
        "gemm 512x512x512 t512 s1 bias+res", "gemm 700x520x256 t512 s1 bias+res", "gemm 300x256x64 t512 s1 bias+res", "gemm 2048x1280x1920 t512 s0 bias+res",
        "gemm 257x64x192 t512 s1 bias+res", "gemm 4096x2560x8192 t0 s0 bias+res", "gemm 2048x512x2304 t512 colstats", "gemm two-source A t512", "gemm batched t512",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 bf16-staged tail16": [
        "gemm 4112x3840x1280 tail bias",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 bf16-staged tail31": [
        "gemm 4127x3840x1280 tail bias",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 f32-direct": [
        "gemm 700x512x256 t512 fp32 out + fp32 residual",
    ],
    "gemm_pp_kernel<0, false, false> splitk1 scalar": [
        "gemm 1000x300x128 t512 s1 bias+res",
    ],
    "gemm_pp_kernel<0, false, false> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 513x1000x1152 t512 s2 bias+res",
    ],
    "gemm_pp_kernel<0, false, false> splitk3 splitk-partial splitk_reduce8_kernel": [
        "gemm 4096x1280x10240 t0 s0 bias+res",
    ],
    "gemm_pp_kernel<0, true, false> splitk1 bf16-staged": [
        "gemm gelu t512",
    ],
    "gemm_pp_kernel<0, true, false> splitk1 f32-direct": [
        "gemm gelu fp32-out t512",
    ],
    "gemm_pq_kernel<0, 320, false> splitk1 bf16-staged": [
        "gemm 1000x320x320 t2320 s1 bias+res", "gemm 700x640x256 t2320 s1 bias+res", "gemm 65536x320x320 t2320 s1 bias+res", "gemm 16384x640x640 t2320 s0 bias+res",
        "gemm 4096x320x320 t2320 colstats", "gemm 8192x640x640 t2320 colstats + residual", "gemm batched t2320",
    ],
    "gemm_pq_kernel<0, 320, false> splitk1 f32-direct": [
        "gemm 1000x640x320 t2320 fp32 out + fp32 residual", "gemm row panels B2 T520 N320 K64",
    ],
    "gemm_pq_kernel<0, 320, false> splitk2 splitk-partial splitk_reduce8_kernel": [
        "gemm 4096x1280x2560 t2320 s0 bias+res",
    ],
    "gemm_pq_kernel<0, 320, true> splitk1 bf16-staged": [
        "gemm 1000x640x320 t2320 gelu", "gemm 970x640x320 t2320 row bias, rows_per_batch 97", "gemm 4096x320x1280 t2320 gelu",
        "gemm 4074x320x1280 t2320 row bias, rows_per_batch 97", "gemm 513x960x64 t2320 gelu", "gemm 485x960x64 t2320 row bias, rows_per_batch 97",
        "gemm row panels B3 T257 N640 K128", "gemm row panels B16 T257 N5120 K1280", "gemm row panels B5 T257 N960 K192",
    ],
    "gemm_pq_kernel<0, 320, true> splitk1 bf16-staged tail16": [
        "gemm 4112x5120x1280 tail gelu+bias",
    ],
    "gemm_pq_kernel<0, 320, true> splitk1 bf16-staged tail32": [
        "gemm 8224x5120x1280 tail gelu+bias",
    ],
    "gemm_tn_kernel splitk1 scalar": [
        "gemm_tn K64 M128 N128 s1", "gemm_tn K1000 M320 N320 s0", "gemm_tn K1232 M2560 N768 s0", "gemm_tn K130 M8 N1280 s1", "gemm_tn fp32 accumulate",
        "gemm_tn into a column slice",
    ],
    "gemm_tn_kernel splitk3 splitk-partial splitk_reduce4f_kernel": [
        "gemm_tn K777 M200 N72 s3",
    ],
    "gemm_tn_kernel splitk32 splitk-partial splitk_reduce4f_kernel": [
        "gemm_tn K65536 M320 N320 s0",
    ],
    "gemm_tn_kernel splitk4 splitk-partial splitk_reduce4f_kernel": [
        "gemm_tn K4096 M960 N320 s0",
    ],
}


def _gemm_said(c, override=None):
    import kernel_checks as kc
    d = kc.gemm_desc(c)
    for k, v in (override or {}).items():
        setattr(d, k, v)
    rc, k = kc.gemm_kernel(c, d)
    assert rc == 0, (c, override, _C.load().e4t_last_error())
    return kc.gemm_kernel_text(k)


def _new_gemm_cases():
    import kernel_checks as kc
    return kc.GEMM_KLOOP_CASES + kc.GEMM_EDGE_CASES + kc.GEMM_FORMS + kc.GEMM_TN_CASES + kc.GEMM_GUARD_CASES + kc.GEMM_TN_GUARD_CASES + kc.GEMM_AUTO_SPLIT_CASES


def test_the_pinned_gemm_tables_cover_exactly_what_the_gemm_checks_run():
    """one set of case lists (tests/kernel_checks.py, importable without a GPU) behind the GPU checks and these tables"""
    import kernel_checks as kc
    pinned = [t for tags in CHECK_GEMM_KERNELS.values() for t in tags]
    assert len(pinned) == len(set(pinned)) and set(pinned) == {kc.gemm_tag(c) for c in _new_gemm_cases()}
    old = [t for tags in CHECK_GEMM_EXISTING_KERNELS.values() for t in tags]
    assert len(old) == len(set(old)) and set(old) == {label for label, _, _ in kc.check_gemm_pinned()}
    # the lists are what the issue of the checks asks for: every DMA row, the K-tile counts around the stage count, both ragged remainders, both splits
    for hint, (tm, tn, kt, st, whole_k, whole_n, general, tail) in kc.GEMM_TILES.items():
        ks = {c.K for c in kc.GEMM_KLOOP_CASES if c.tile == hint and c.sk == 1 and c.form == "bare"}
        assert {kt * n for n in (1, 2, 3, st, st + 1, st + 2, st + 3)} <= ks and (whole_k or {72, 64 * st + 40} <= ks), hint
        assert {(c.K, c.sk) for c in kc.GEMM_KLOOP_CASES if c.tile == hint and c.sk > 1} == {(320, 2), (192, 3)}
        assert general == any(c.form == "gelu" for c in kc.GEMM_KLOOP_CASES if c.tile == hint)
        assert tail == ({c.M for c in kc.GEMM_EDGE_CASES if c.tile == hint} >= {1153, 1169, 1184})
    assert all(c.M <= 2400 and c.N <= 960 and (c.K <= 704 or c in kc.GEMM_AUTO_SPLIT_CASES or c.K == 2048) for c in _new_gemm_cases())
    assert {"bare", "bias", "full", "gelu", "f32", "f32 res32", "f32 res16", "accum16", "accum32", "alpha", "rowbias slice", "C slice8", "C slice4",
            "res slice", "colstats", "colstats+res"} <= {c.form for c in kc.GEMM_FORMS}


def test_gemm_check_cases_keep_their_kernels(dumper):      # (the fixture: the tables are for 256 CUs)
    import kernel_checks as kc
    want = {t: text for text, tags in CHECK_GEMM_KERNELS.items() for t in tags}
    for c in _new_gemm_cases():
        assert _gemm_said(c) == want[kc.gemm_tag(c)], c
    want = {t: text for text, tags in CHECK_GEMM_EXISTING_KERNELS.items() for t in tags}
    for label, c, override in kc.check_gemm_pinned():
        assert _gemm_said(c, override) == want[label], label
    # every new case runs on the row its tile hint names, in the instantiation its form asks for
    for c in kc.GEMM_KLOOP_CASES + kc.GEMM_EDGE_CASES + kc.GEMM_FORMS:
        pl, form = kc.gemm_plan(c), kc.gemm_form(c)
        tm, tn, kt, st = kc.GEMM_TILES[c.tile][:4]
        general = bool(form.get("gelu")) or form.get("rowbias", 32) % 32 != 0
        assert (pl.tile_m, pl.tile_n) == (tm, tn) and pl.stages in (0, st) and pl.splitk == max(c.sk, 1), c
        assert ((", true, 64>" in _gemm_said(c)) or ("_kernel<0, true, false>" in _gemm_said(c)) or ("320, true>" in _gemm_said(c))) == general, c
    # the three reduce kernels are each named for the split-K forms, on every kernel family
    for c in kc.GEMM_FORMS:
        if c.sk > 1:
            assert _gemm_said(c).split(" ")[-1] == kc.GEMM_FORM_SPLITK[c.form], c
    # the automatic split-K falls back to ONE pass without its workspace and the query says so; an explicit one is refused like the launch (-12)
    c = kc.GEMM_AUTO_SPLIT_CASES[0]
    d, k = kc.gemm_desc(c), _C.GemmKernel()
    assert _C.load().e4t_gemm_kernel(C.byref(d), C.byref(k)) == 0 and k.splitk == 2 and k.reduce == b"splitk_reduce8_kernel" and k.store == 3
    d.workspace, d.workspace_bytes = None, 0
    assert _C.load().e4t_gemm_kernel(C.byref(d), C.byref(k)) == 0 and k.splitk == 1 and k.reduce is None and k.store == 0
    d.splitk = 2
    assert _C.load().e4t_gemm_kernel(C.byref(d), C.byref(k)) == -12 and _C.load().e4t_gemm_tn_kernel(C.byref(kc.gemm_desc(kc.TnCase(300, 168, 152, 2, "f32"), ws_bytes=16, ws=1 << 24)), C.byref(k)) == -12
    # a fused GEGLU descriptor the launch would refuse: E4T_ERR_NO_FUSED with the launch's message (here: a shape whose plan is the 256 x 256 tile)
    d = _C.GemmDesc(A=1 << 24, B=1 << 24, C=1 << 24, aux=1 << 24, M=4096, N=2560, K=8192, K1=8192, lda=8192, ldb=8192, ldc=2560, ldaux=1280, batch=1, alpha=1.0,
                    flags=_C.EPI_GEGLU)
    assert _C.load().e4t_gemm_kernel(C.byref(d), C.byref(k)) == _C.ERR_NO_FUSED and b"fused GEGLU" in _C.load().e4t_last_error()
    assert _C.load().e4t_gemm_plan(C.byref(d), C.byref(_C.GemmPlan())) == _C.ERR_NO_FUSED


# Every (kernel symbol, store path) e4t_gemm_kernel / e4t_gemm_tn_kernel return over the gemm and tn items of the dispatch corpus, the step table's
# included, and every reduce kernel.  The store path is a run-time branch of write_tile, so symbol x store path is the unit the checks must reach.
ALL_STORES = ("bf16-staged", "f32-direct", "scalar", "splitk-partial")
GEMM_KERNEL_STORES = {
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, false, 64>": ALL_STORES,
    "gemm_dma_kernel<128, 128, 4, 2, 0, 2, true, 64>": ("bf16-staged", "scalar", "splitk-partial"),
    "gemm_dma_kernel<128, 128, 4, 2, 0, 3, false, 64>": ALL_STORES,
    "gemm_dma_kernel<128, 128, 4, 2, 0, 4, false, 64>": ALL_STORES,
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, false, 64>": ALL_STORES,
    "gemm_dma_kernel<128, 160, 4, 1, 0, 2, true, 64>": ("bf16-staged", "splitk-partial"),
    "gemm_dma_kernel<128, 160, 4, 1, 0, 3, false, 64>": ALL_STORES,
    "gemm_dma_kernel<128, 160, 4, 1, 0, 4, false, 64>": ALL_STORES,
    "gemm_dma_kernel<256, 128, 4, 2, 0, 3, false, 32>": ALL_STORES,
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, false, 64>": ALL_STORES,
    "gemm_dma_kernel<64, 64, 2, 2, 0, 2, true, 64>": ("bf16-staged", "splitk-partial"),
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, false, 64>": ALL_STORES,
    "gemm_dma_kernel<64, 64, 2, 2, 0, 3, true, 64>": ("bf16-staged", "scalar", "splitk-partial"),
    "gemm_dma_kernel<64, 64, 2, 2, 0, 4, false, 64>": ALL_STORES,
    "gemm_kernel": ("bf16-staged",),
    "gemm_pp_kernel<0, false, false>": ALL_STORES,
    "gemm_pp_kernel<0, true, false>": ("bf16-staged", "splitk-partial"),
    "gemm_pq_kernel<0, 320, false>": ALL_STORES,
    "gemm_pq_kernel<0, 320, true>": ("bf16-staged", "splitk-partial"),
    "gemm_tn_kernel": ("bf16-staged", "scalar", "splitk-partial"),
}
GEMM_REDUCE_KERNELS = {"splitk_reduce_kernel", "splitk_reduce8_kernel", "splitk_reduce4f_kernel"}
# the eleven fused-GEGLU instantiations (gemm.hip, kVariants: CAP_GEGLU): reached through the shapes of tests/test_ff_fused_gpu.py, always bf16-staged
GEMM_GEGLU_KERNELS = {
    "gemm_dma_geglu_kernel<128, 128, 4, 2, 2, 64, 1>",
    "gemm_dma_geglu_kernel<128, 128, 4, 2, 2, 64, 2>",
    "gemm_dma_geglu_kernel<128, 128, 4, 2, 4, 64, 2>",
    "gemm_dma_geglu_kernel<128, 160, 4, 1, 2, 64, 1>",
    "gemm_dma_geglu_kernel<128, 160, 4, 1, 3, 64, 2>",
    "gemm_dma_geglu_kernel<256, 128, 4, 2, 3, 32, 1>",
    "gemm_dma_geglu_kernel<256, 128, 4, 2, 3, 32, 2>",
    "gemm_dma_geglu_kernel<64, 64, 2, 2, 3, 64, 1>",
    "gemm_dma_geglu_kernel<64, 64, 2, 2, 4, 64, 2>",
    "gemm_pq_geglu_kernel<320, 1>",
    "gemm_pq_geglu_kernel<320, 2>",
}
# symbol -> why no check of this file's tables executes it
GEMM_KERNELS_NOT_REACHED = {
    "gemm_kernel": "the register-staged fallback: chosen only for an operand beyond 4 GB or under the E4T_GEMM_REGSTAGE switch (read once per process); "
                   "tests/test_gemm_regstage_gpu.py runs it in a child process",
}


def _geglu_symbols():
    """the kernels the fused feed-forward launches of tests/test_ff_fused_gpu.py get: forward u = x . W1^T (N = 8 dim), backward dh = dy . W2 (N = 4 dim)"""
    import test_ff_fused_gpu as ff
    got = set()
    for M, dim in ff.STEP + ff.SD2:
        H, k, fake = 4 * dim, _C.GemmKernel(), 1 << 24
        for d in (_C.GemmDesc(A=fake, B=fake, C=fake, aux=fake, bias=fake, M=M, N=2 * H, K=dim, K1=dim, lda=dim, ldb=dim, ldc=2 * H, ldaux=H, batch=1, alpha=1.0, flags=_C.EPI_GEGLU),
                  _C.GemmDesc(A=fake, B=fake, C=fake, aux=fake, M=M, N=H, K=dim, K1=dim, lda=dim, ldb=dim, ldc=2 * H, ldaux=2 * H, batch=1, alpha=1.0, flags=_C.EPI_GEGLU_BWD)):
            assert _C.load().e4t_gemm_kernel(C.byref(d), C.byref(k)) == 0, (M, dim, _C.load().e4t_last_error())
            assert k.store == 0 and k.splitk == 1 and k.reduce is None
            got.add(k.symbol.decode())
    return got


def test_gemm_checks_reach_every_kernel_the_launcher_can_choose(dumper):
    """(symbol, store path) and the reduce kernels over the corpus == the clear-text sets above, and the checks execute each of them but the listed
    exceptions: a kernel added to the variant table (or a rule changed so that one is no longer reached) fails here until a check has a shape for it"""
    reachable, reduces = {}, set()
    for item in dump.corpus():
        if item.kind in ("gemm", "tn"):
            f = dumper.gemm_kernel(item).split(" ")
            if f[0] != "rc":
                i = next(j for j, w in enumerate(f) if w.startswith("splitk") and w[6:].isdigit())
                reachable.setdefault(" ".join(f[:i]), set()).add(f[i + 1])
                reduces |= {w for w in f[i + 2:] if w.startswith("splitk_reduce")}
    assert {s: tuple(p for p in ALL_STORES if p in st) for s, st in reachable.items()} == GEMM_KERNEL_STORES
    assert reduces == GEMM_REDUCE_KERNELS
    reached, reached_reduces = set(), set()
    for text in list(CHECK_GEMM_KERNELS) + list(CHECK_GEMM_EXISTING_KERNELS):
        sym, store, rest = re.match(r"(.*) splitk\d+ (\S+)(.*)$", text).groups()
        reached.add((sym, store))
        reached_reduces |= {w for w in rest.split() if w.startswith("splitk_reduce")}
    units = {(s, p) for s, stores in GEMM_KERNEL_STORES.items() for p in stores}
    excluded = {(s, p) for s, p in units if s in GEMM_KERNELS_NOT_REACHED}
    assert set(GEMM_KERNELS_NOT_REACHED) <= set(GEMM_KERNEL_STORES) and not (reached & excluded)
    # (the checks also run pairs the corpus does not hold, e.g. a GENERAL instantiation storing fp32 directly: reached may be the larger set)
    assert units <= reached | excluded, sorted(units - reached - excluded)
    assert reached_reduces == GEMM_REDUCE_KERNELS
    assert _geglu_symbols() == GEMM_GEGLU_KERNELS and len(GEMM_GEGLU_KERNELS) == 11
