"""CPU: what the sampling entry points of sampler.hip refuse (e4t_guided_step, e4t_guidance_stats, e4t_sampler_step, _edit, _guided).  Every call below
fails validation on the host, before any launch, so the dummy pointers are never dereferenced and no GPU is needed (the pattern of
test_streaming_args_cpu.py); each refusal is -22 with the words that name it.  The three sampler_step entries share one validator and one launcher, so
the words pin that each still speaks under its own name and keeps its own x_in_copies limit.  test_sampler_plan.py, test_sampler_edit_plan.py and
test_guidance_host_logic.py hold the refusals that came with their features; the rest are here."""
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


def test_guided_step_refusals(lib):
    for pred, sample, out, coef in [(N, P, P, P), (P, N, P, P), (P, P, N, P), (P, P, P, N)]:
        refused(lib, lib.e4t_guided_step(pred, sample, N, out, coef, 2, 4, 6, 1, 0, N), "guided_step: bad arguments")
    for B, C, HW in [(0, 4, 6), (-1, 4, 6), (2, 0, 6), (2, -4, 6), (2, 4, 0), (2, 4, -6)]:
        refused(lib, lib.e4t_guided_step(P, P, P, P, P, B, C, HW, 1, 0, N), "guided_step: bad arguments")


def test_guidance_stats_refusals(lib):
    def call(pred=P, gp=P, gstat=P, B=2, C=4, HW=6, branches=2):
        return lib.e4t_guidance_stats(pred, gp, gstat, B, C, HW, branches, 0, N)
    for name in ("pred", "gp", "gstat"):
        refused(lib, call(**{name: N}), "guidance_stats: %s is null" % name)
    refused(lib, call(branches=1), "guidance_stats: branches = 1 (2: [u | c], 3: [u | k | c])")
    refused(lib, call(branches=4), "guidance_stats: branches = 4 (2: [u | c], 3: [u | k | c])")
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-4), dict(HW=0), dict(HW=-6)):
        refused(lib, call(**kw), "guidance_stats: B = %d, C = %d, HW = %d" % (kw.get("B", 2), kw.get("C", 4), kw.get("HW", 6)))
    refused(lib, call(C=65536, HW=32768), "guidance_stats: B = 2, C = 65536, HW = 32768")      # C*HW = 2^31 > INT_MAX
    refused(lib, call(C=1, HW=1), "guidance_stats: N = C*HW = 1 values per image (an unbiased deviation needs N >= 2)")


def step_entries(lib):
    """(name, x_in_copies limit, call) of the three entries; the optional pointers default to null, keep / x0 / n0 to what lets the entry pass"""
    def plain(pred=P, x=P, out=P, hist=N, x_in=N, row=P, B=2, C=4, HW=6, K=0, copies=0):
        return lib.e4t_sampler_step(pred, x, out, hist, N, N, x_in, row, B, C, HW, K, 1, 0, copies, N)

    def edit(pred=P, x=P, out=P, hist=N, x_in=N, row=P, B=2, C=4, HW=6, K=0, copies=0, keep=P, x0=P, n0=P, kpi=0, xpi=0):
        return lib.e4t_sampler_step_edit(pred, x, out, hist, N, N, x_in, row, keep, x0, n0, B, C, HW, K, 1, 0, copies, kpi, xpi, N)

    def guided(pred=P, x=P, out=P, hist=N, x_in=N, row=P, B=2, C=4, HW=6, K=0, copies=0, keep=N, x0=N, n0=N, kpi=0, xpi=0, gp=P, branches=2):
        return lib.e4t_sampler_step_guided(pred, x, out, hist, N, N, x_in, row, gp, N, keep, x0, n0, B, C, HW, K, branches, 0, copies, kpi, xpi, N)
    return [("sampler_step", 2, plain), ("sampler_step_edit", 2, edit), ("sampler_step_guided", 3, guided)]


def test_sampler_step_shared_refusals(lib):
    for name, limit, call in step_entries(lib):
        for kw in (dict(pred=N), dict(x=N), dict(out=N), dict(row=N), dict(B=0), dict(B=-1), dict(C=0), dict(C=-4), dict(HW=0), dict(HW=-6)):
            refused(lib, call(**kw), name + ": bad arguments")
        for K, hist in [(-1, P), (5, P), (1, N), (4, N)]:
            refused(lib, call(K=K, hist=hist), "%s: K = %d history slots (0..4, hist required when K > 0)" % (name, K))
        for copies, x_in in [(-1, P), (limit + 1, P), (1, N), (limit, N)]:
            refused(lib, call(copies=copies, x_in=x_in), "%s: x_in_copies = %d (0..%d, x_in required when > 0)" % (name, copies, limit))


def test_sampler_step_edit_refusals(lib):
    _, _, call = step_entries(lib)[1]
    for kw in (dict(keep=N), dict(x0=N), dict(n0=N), dict(keep=N, x0=N, n0=N)):
        refused(lib, call(**kw), "sampler_step_edit: keep, x0 and n0 are required")
    for kpi, xpi in [(2, 0), (-1, 0), (0, 2), (0, -1)]:
        refused(lib, call(kpi=kpi, xpi=xpi), "sampler_step_edit: keep_per_image = %d, x0_per_image = %d (0 or 1)" % (kpi, xpi))


def test_sampler_step_guided_refusals(lib):
    _, _, call = step_entries(lib)[2]
    refused(lib, call(gp=N), "sampler_step_guided: bad arguments")
    for br in (1, 4):
        refused(lib, call(branches=br), "sampler_step_guided: branches = %d (2: [u | c], 3: [u | k | c])" % br)
    for keep, x0, n0 in [(P, N, N), (N, P, N), (N, N, P), (P, P, N), (P, N, P), (N, P, P)]:
        refused(lib, call(keep=keep, x0=x0, n0=n0), "sampler_step_guided: keep, x0 and n0 are given together or not at all")
    for kpi, xpi in [(2, 0), (-1, 0), (0, 2), (0, -1)]:
        refused(lib, call(kpi=kpi, xpi=xpi), "sampler_step_guided: keep_per_image = %d, x0_per_image = %d (0 or 1)" % (kpi, xpi))
        refused(lib, call(keep=P, x0=P, n0=P, kpi=kpi, xpi=xpi), "sampler_step_guided: keep_per_image = %d, x0_per_image = %d (0 or 1)" % (kpi, xpi))
