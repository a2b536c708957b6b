"""CPU: what the optimiser entry points of optim.hip refuse (e4t_adamw, _hyper, _ema, _rank, _rank_ema, e4t_adamw8, e4t_ema_update).  Every call
below fails validation on the host, before any launch, so the dummy pointers are never dereferenced and no GPU is needed (the pattern of
test_streaming_args_cpu.py, which also holds e4t_sumsq_partial's refusals); each refusal is -22 with the words that name it.  The entries share their
launch paths, so the words pin that each still speaks under its own name."""
import pytest

P = 4096      # a non-null, 16-byte aligned "pointer"
N = None
HP = (1e-3, 0.9, 0.999, 1e-8, 0.01)      # lr, beta1, beta2, eps, weight_decay


@pytest.fixture(scope="module")
def lib():
    from e4t import _C
    return _C.load()


def refused(lib, rc, words):
    assert rc == -22, rc
    assert words.encode() in lib.e4t_last_error(), (words, lib.e4t_last_error())


def each_with(n, value, skip=()):
    """pointer lists of length n with one pointer replaced by value at a time"""
    for k in range(n):
        if k not in skip:
            ptrs = [P] * n
            ptrs[k] = value
            yield ptrs


def test_adamw_refusals(lib):
    for ptrs in each_with(4, N):
        refused(lib, lib.e4t_adamw(*ptrs, 64, *HP, 1, 1.0, N), "adamw: bad arguments")
    for n, step in [(0, 1), (-4, 1), (64, 0), (64, -1)]:
        refused(lib, lib.e4t_adamw(P, P, P, P, n, *HP, step, 1.0, N), "adamw: bad arguments")
    for ptrs in each_with(4, P + 4):
        refused(lib, lib.e4t_adamw(*ptrs, 64, *HP, 1, 1.0, N), "adamw: buffers must be 16-B aligned")


def test_adamw_hyper_refusals(lib):
    for p, g, m, v, h in each_with(5, N):
        refused(lib, lib.e4t_adamw_hyper(p, g, m, v, 64, h, *HP[1:], N), "adamw_hyper: bad arguments")
    for n in (0, -4):
        refused(lib, lib.e4t_adamw_hyper(P, P, P, P, n, P, *HP[1:], N), "adamw_hyper: bad arguments")
    for p, g, m, v, h in each_with(5, P + 4):
        refused(lib, lib.e4t_adamw_hyper(p, g, m, v, 64, h, *HP[1:], N), "adamw_hyper: buffers must be 16-B aligned")


def test_adamw_ema_refusals(lib):
    def call(ptrs=(P,) * 5, n=64, step=1, hyper=N):
        return lib.e4t_adamw_ema(*ptrs, n, *HP, step, 1.0, 1e-4, hyper, N)
    for ptrs in each_with(5, N):
        refused(lib, call(ptrs), "adamw_ema: bad arguments")
    for kw in (dict(n=0), dict(n=-4), dict(step=0), dict(step=-1)):
        refused(lib, call(**kw), "adamw_ema: bad arguments")
    refused(lib, call(n=0, step=0, hyper=P), "adamw_ema: bad arguments")      # hyper_dev lifts the step rule only
    for ptrs in each_with(5, P + 4):
        refused(lib, call(ptrs), "adamw_ema: buffers must be 16-B aligned")
    refused(lib, call(hyper=P + 4), "adamw_ema: buffers must be 16-B aligned")


def rank_entries(lib):
    """(name, call) of the two rank entries; ptrs = p, m, v, [ema,] G, Z"""
    def plain(ptrs, n=2, rows=9, cols=68, K=17, ldg=9, ldz=136, step=1, hyper=N):
        return lib.e4t_adamw_rank(*ptrs, n, rows, cols, K, ldg, ldz, *HP, step, 1.0, hyper, N)

    def ema(ptrs, n=2, rows=9, cols=68, K=17, ldg=9, ldz=136, step=1, hyper=N):
        return lib.e4t_adamw_rank_ema(*ptrs, n, rows, cols, K, ldg, ldz, *HP, step, 1.0, 1e-4, hyper, N)
    return [("adamw_rank", 5, plain), ("adamw_rank_ema", 6, ema)]


def test_adamw_rank_refusals(lib):
    for name, np_, call in rank_entries(lib):
        ok = [P] * np_
        for ptrs in each_with(np_, N):
            refused(lib, call(ptrs), name + ": bad arguments")
        for kw in (dict(n=0), dict(n=-1), dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-4), dict(K=0), dict(K=-1), dict(step=0), dict(step=-1)):
            refused(lib, call(ok, **kw), name + ": bad arguments")
        refused(lib, call(ok, K=0, step=0, hyper=P), name + ": bad arguments")      # hyper_dev lifts the step rule only
        for kw in (dict(cols=66, ldz=132), dict(ldz=138), dict(ldg=8), dict(ldz=132)):      # cols % 4, ldz % 4, ldg < rows, ldz < n * cols
            refused(lib, call(ok, **kw), name + ": cols and the Z row stride must be multiples of 4")
        words = name + ": buffers must be 16-B (factors 8-B) aligned"
        for ptrs in each_with(np_ - 2, P + 4):      # p, m, v (and ema): 16 bytes
            refused(lib, call(ptrs + [P, P]), words)
        refused(lib, call(ok[:-1] + [P + 2]), words)      # Z: 8 bytes
        refused(lib, call(ok[:-1] + [P + 4]), words)
        refused(lib, call(ok, hyper=P + 4), words)


def test_adamw8_refusals(lib):
    def call(ptrs=(P,) * 6, ema=N, n=1027, codes=(P, P), step=1, hyper=N):
        return lib.e4t_adamw8(*ptrs, ema, n, *codes, *HP, step, 1.0, 1e-4, hyper, N)
    for ptrs in each_with(6, N):
        refused(lib, call(ptrs), "adamw8: bad arguments")
    for codes in each_with(2, N):
        refused(lib, call(codes=codes), "adamw8: bad arguments")
    for kw in (dict(n=0), dict(n=-1), dict(step=0), dict(step=-1)):
        refused(lib, call(**kw), "adamw8: bad arguments")
        refused(lib, call(ema=P, **kw), "adamw8: bad arguments")
    refused(lib, call(n=0, step=0, hyper=P), "adamw8: bad arguments")
    wide = "adamw8: p, g, ema and hyper_dev must be 16-B aligned"
    refused(lib, call((P + 4, P, P, P, P, P)), wide)
    refused(lib, call((P, P + 4, P, P, P, P)), wide)
    refused(lib, call(ema=P + 4), wide)
    refused(lib, call(hyper=P + 4), wide)
    narrow = "adamw8: codes, scales and codebooks must be 4-B aligned"
    for ptrs in each_with(6, P + 2, skip=(0, 1)):      # qm, qv, absmax_m, absmax_v
        refused(lib, call(ptrs), narrow)
    for codes in each_with(2, P + 2):
        refused(lib, call(codes=codes), narrow)


def test_ema_update_refusals(lib):
    for ptrs in each_with(2, N):
        refused(lib, lib.e4t_ema_update(*ptrs, 64, 1e-4, N, N), "ema_update: bad arguments")
    for n in (0, -4):
        refused(lib, lib.e4t_ema_update(P, P, n, 1e-4, N, N), "ema_update: bad arguments")
    for ptrs in each_with(2, P + 4):
        refused(lib, lib.e4t_ema_update(*ptrs, 64, 1e-4, N, N), "ema_update: buffers must be 16-B aligned")
    refused(lib, lib.e4t_ema_update(P, P, 64, 1e-4, P + 2, N), "ema_update: buffers must be 16-B aligned")
