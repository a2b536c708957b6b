"""CPU: what the training-objective entry points of objective.hip refuse (e4t_diffuse, e4t_masked_mse_fwd, e4t_weighted_mse_fwd,
e4t_robust_loss_fwd, e4t_masked_mse_bwd).  Every call below fails validation on the host, before any launch, so the dummy pointers are never
dereferenced and no GPU is needed (the pattern of test_streaming_args_cpu.py); each refusal is -22 with the words that name it."""
import pytest

P = 4096      # a non-null, 16-byte aligned "pointer"
N = None
SHAPES = [(0, 4, 6), (-1, 4, 6), (2, 0, 6), (2, -4, 6), (2, 4, 0), (2, 4, -6)]      # B, C, HW: each count at zero and negative


@pytest.fixture(scope="module")
def lib():
    from e4t import _C
    return _C.load()


def refused(lib, rc, words):
    assert rc == -22, rc
    assert words.encode() in lib.e4t_last_error(), (words, lib.e4t_last_error())


def test_masked_mse_fwd_refusals(lib):
    for pred, target, w, stats in [(N, P, P, P), (P, N, P, P), (P, P, N, P), (P, P, P, N)]:      # wd may be null
        refused(lib, lib.e4t_masked_mse_fwd(pred, target, w, N, stats, 2, 4, 6, 0, N), "masked_mse_fwd: bad arguments")
    for B, C, HW in SHAPES:
        refused(lib, lib.e4t_masked_mse_fwd(P, P, P, P, P, B, C, HW, 0, N), "masked_mse_fwd: bad arguments")


def test_weighted_mse_fwd_refusals(lib):
    words = "weighted_mse_fwd: bad arguments (pred, target, stats non-null; B, C, HW > 0)"
    for pred, target, stats in [(N, P, P), (P, N, P), (P, P, N)]:      # w, lam and wd may be null
        refused(lib, lib.e4t_weighted_mse_fwd(pred, target, N, N, N, stats, 2, 4, 6, 0, N), words)
    for B, C, HW in SHAPES:
        refused(lib, lib.e4t_weighted_mse_fwd(P, P, P, P, P, P, B, C, HW, 0, N), words)


def test_robust_loss_fwd_refusals(lib):
    def call(pred=P, target=P, ctab=P, stats=P, B=2, C=4, HW=6, T=1000, kind=1):
        return lib.e4t_robust_loss_fwd(pred, target, N, N, ctab, N, N, stats, B, C, HW, T, kind, 0, N)
    words = "robust_loss_fwd: bad arguments (pred, target, ctab, stats non-null; B, C, HW > 0)"
    for name in ("pred", "target", "ctab", "stats"):
        refused(lib, call(**{name: N}), words)
    for B, C, HW in SHAPES:
        refused(lib, call(B=B, C=C, HW=HW), words)
    for T in (0, -1):
        refused(lib, call(T=T), "robust_loss_fwd: T = %d, the table needs at least one entry" % T)
    for kind in (0, 3, -1):
        refused(lib, call(kind=kind), "robust_loss_fwd: kind = %d must be 1 (huber) or 2 (smooth_l1)" % kind)


def test_masked_mse_bwd_refusals(lib):
    for wd, stats, g, dpred in [(N, P, P, P), (P, N, P, P), (P, P, N, P), (P, P, P, N)]:
        refused(lib, lib.e4t_masked_mse_bwd(wd, stats, g, dpred, 48, N), "masked_mse_bwd: bad arguments")
    for n in (0, -48):
        refused(lib, lib.e4t_masked_mse_bwd(P, P, P, P, n, N), "masked_mse_bwd: bad arguments")


def test_diffuse_refusals(lib):
    def call(ptrs=(P,) * 7, z=P, B=2, C=4, HW=6, T=1000, s=0.0):      # ptrs = x0, noise, timesteps, coef, noisy, target, lam
        x0, noise, timesteps, coef, noisy, target, lam = ptrs
        return lib.e4t_diffuse(x0, noise, z, timesteps, coef, noisy, target, lam, B, C, HW, T, s, 0, N)
    for k in range(7):
        refused(lib, call(tuple(N if j == k else P for j in range(7))), "diffuse: null pointer (only z may be null)")
    for B, C, HW in SHAPES:
        refused(lib, call(B=B, C=C, HW=HW), "diffuse: B = %d, C = %d, HW = %d, T = 1000 must be positive" % (B, C, HW))
    for T in (0, -1):
        refused(lib, call(T=T), "diffuse: B = 2, C = 4, HW = 6, T = %d must be positive" % T)
    refused(lib, call(z=N, s=0.1), "diffuse: a noise offset s = 0.1 needs z")
    refused(lib, call(s=-0.1), "diffuse: the noise offset s = -0.1 must be >= 0")
    refused(lib, call(z=N, s=-0.1), "diffuse: a noise offset s = -0.1 needs z")
