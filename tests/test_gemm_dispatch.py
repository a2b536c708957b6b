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
and split-K in clear text, and the symbols x conv modes the checks reach are held against everything the query returns over the corpus."""
import ctypes as C
import importlib.util
import os

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
