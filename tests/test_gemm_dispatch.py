"""The GEMM / 3x3-conv planner (csrc/gemm.hip: plan_gemm and the variant table behind it) decides for a broad corpus of descriptors what
the record says: tests/gemm_dispatch_record.txt holds one SHA-256 per corpus group (one tile hint x {gemm, conv}, and the TN planner)
over the lines `descriptor -> tile tile_m tile_n splitk workspace_bytes tail_rows stages`, and the plans of the training step's own
shapes in clear text.  Corpus and record come from tools/gemm_dispatch_dump.py; after an INTENTIONAL planner change

    python tools/gemm_dispatch_dump.py --record

rewrites the record (on a machine without a GPU: it anchors the step shapes through the launch log).  Only the plan entry points are
called here — pure host code, safe on any machine; the launch half of the tool is never part of a test."""
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
    groups, step = {}, []
    for line in open(dump.RECORD):
        if line.startswith("group "):
            g, n, hx = (s.strip() for s in line[len("group "):].split("|"))
            groups[g] = (int(n), hx)
        elif line.startswith("step "):
            step.append(line[len("step "):].rstrip("\n"))
    return groups, step


@pytest.fixture(scope="module")
def dumper():
    # the record is made where the planner sees 256 CUs: an MI355X, or no device at all (its fallback)
    if _cu_count() != 256:
        pytest.skip("the plan record is for 256 CUs (MI355X, or no device); this device has %d" % _cu_count())
    d = dump.Dumper(launches=False)
    yield d
    d.close()


def _checked_groups(groups):
    if _C.load().e4t_build_flags() == 0:
        return sorted(groups)
    # an E4T_EXPERIMENTAL=1 library answers the experimental tile codes with kernels the default build does not carry
    skipped = {"%s t%d" % (k, t) for k in ("gemm", "conv") for t in dump.EXPERIMENTAL_HINTS}
    print("experimental library: checking only the groups whose hint is a product code (not %s)" % sorted(skipped))
    return sorted(set(groups) - skipped)


def test_record_covers_the_corpus():
    groups, step = _record()
    want = {"%s t%d" % (k, t) for k in ("gemm", "conv") for t in dump.HINTS} | {"tn"}
    assert set(groups) == want
    rows = dump.step_rows()
    assert len(step) == len(rows) == 167 and sum(1 for s, _ in rows if not s.startswith("splitk_reduce")) == 153
    assert [s.split(" | ")[0] for s in step] == ["%s|%s" % r for r in rows]      # every recorded launch of the step table, in its order


def test_plans_match_the_record(dumper):
    groups, _ = _record()
    checked = _checked_groups(groups)
    got, _ = dump.plan_digests(dumper, only_groups=set(checked))
    bad = [g for g in checked if got.get(g) != groups[g]]
    assert not bad, ("the planner decides differently for corpus group(s) %s: compare `python tools/gemm_dispatch_dump.py --plans --group '%s'` of this "
                     "library and of the one the record was made from (E4T_LIB=...), or re-record an intentional change with --record" % (bad, bad[0]))


def test_step_shapes_get_the_recorded_plans(dumper):
    """the step's 153 GEMM / conv / TN launches (and the 14 split-K reduces behind them), descriptor and plan in clear text"""
    _, step = _record()
    for line in step:
        sym_shape, rest = line.split(" | ", 1)
        desc, plan = rest.split(" -> ")
        kind, *kv = desc.split(" ")
        item = dump.Item("step", kind, {k: int(v) for k, v in (s.split("=") for s in kv)})
        assert dumper.plan(item) == plan, (sym_shape, desc)
