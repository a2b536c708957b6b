"""CPU: the masked diffusion loss above the kernels — the fp32 composition of functional.masked_mse (the executable specification,
and what the op emulation runs) against a float64 restatement, mask pairing in E4TDataset, mask packing in pack_batch, the trainer
with a loss mask through the op emulation, and the two command-line flags.

Bound: rel-L2 <= 2e-5, the project's bound for an fp32 kernel against a float64 restatement."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from test_unet_host_logic import emu_fp32  # noqa: F401
from test_train_step_host_logic import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-5
SHAPES = [(1, 4, 1, 1), (3, 4, 5, 7), (2, 4, 64, 64)]


def restate64(pred, target, w):
    """the definition in float64, gradient by torch autograd: (loss, dloss/dpred)"""
    p = pred.detach().double().requires_grad_(True)
    d = p - target.detach().double()
    wd = w.detach().double()
    den = pred.shape[1] * torch.clamp(wd.sum(), min=1.0)
    loss = (wd.unsqueeze(1) * d * d).sum() / den
    loss.backward()
    return loss.detach(), p.grad


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def make_mask(kind, B, h, w, g):
    if kind == "soft":
        return torch.rand(B, h, w, generator=g)
    return torch.ones(B, h, w) if kind == "ones" else torch.zeros(B, h, w)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["soft", "ones", "zero"])
def test_fallback_matches_float64_restatement(emu_fp32, shape, kind):
    from e4t import functional as Fn
    B, C, h, w = shape
    g = torch.Generator().manual_seed(B * 1000 + h)
    pred = torch.randn(shape, generator=g).requires_grad_(True)
    target = torch.randn(shape, generator=g)
    m = make_mask(kind, B, h, w, g)
    loss = Fn.masked_mse(pred, target, m)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    want, dwant = restate64(pred, target, m)
    if kind == "zero":
        assert float(loss.detach()) == 0.0 and float(pred.grad.abs().max()) == 0.0
        assert float(want) == 0.0 and float(dwant.abs().max()) == 0.0
        return
    assert rel(loss.detach(), want) <= BOUND
    assert rel(pred.grad, dwant) <= BOUND
    if kind == "ones":
        assert rel(loss.detach(), F.mse_loss(pred.detach(), target)) <= BOUND


def test_entry_points_check_their_arguments():
    """argument validation happens on the host before any launch: safe to call without a GPU"""
    import ctypes
    from e4t import _C
    lib = _C.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.e4t_mask_prep(p, p, None, p, 1, 64, None) == -22 and b"null pointer" in lib.e4t_last_error()
    assert lib.e4t_mask_prep(p, p, p, p, 1, 60, None) == -22 and b"S % 8 == 0" in lib.e4t_last_error()
    assert lib.e4t_mask_prep(p, p, p, p, 65536, 64, None) == -22
    assert lib.e4t_masked_mse_fwd(p, p, None, p, p, 1, 4, 1, 0, None) == -22 and b"masked_mse_fwd" in lib.e4t_last_error()
    assert lib.e4t_masked_mse_fwd(p, p, p, p, p, 1, 0, 1, 0, None) == -22
    assert lib.e4t_masked_mse_bwd(p, p, None, p, 16, None) == -22 and b"masked_mse_bwd" in lib.e4t_last_error()
    assert _C.MASKED_MSE_STATS == 2050


# ---------------------------------------------------------------------------------------------- data
def _png(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _tree(tmp_path, rng):
    """two image roots (one with a sub-directory) and their mask roots; returns {image path: mask array}"""
    want = {}
    layout = [("imgA", "maskA", ["a.png", "sub/b.jpg", "sub/c.png"]), ("imgB", "maskB", ["d.png", "e.png"])]
    for iroot, mroot, files in layout:
        for k, f in enumerate(files):
            h, w = 20 + 3 * k, 30 + k
            _png(str(tmp_path / iroot / f), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            m = rng.integers(0, 256, (h, w), dtype=np.uint8)
            # masks are looked up by stem: the .jpg image has a .png mask
            _png(str(tmp_path / mroot / (os.path.splitext(f)[0] + ".png")), m)
            want[str(tmp_path / iroot / f)] = m
    return want


def test_dataset_pairs_masks_by_relative_path_and_stem(tmp_path):
    from e4t.data import E4TDataset
    rng = np.random.default_rng(0)
    want = _tree(tmp_path, rng)
    ds = E4TDataset(f"{tmp_path / 'imgA'}::{tmp_path / 'imgB'}", resolution=16, mask_dataset=f"{tmp_path / 'maskA'}::{tmp_path / 'maskB'}")
    assert len(ds) == 5 and len(ds.masks) == 5
    for i in range(len(ds)):
        s = ds[i]
        assert s["mask"].dtype == np.uint8 and s["mask"].shape == s["image"].shape[:2]
        np.testing.assert_array_equal(s["mask"], want[ds.dataset[i]])
    # without masks: samples as before
    plain = E4TDataset(f"{tmp_path / 'imgA'}::{tmp_path / 'imgB'}", resolution=16)
    assert plain.masks is None and set(plain[0]) == {"image", "plan"} and plain.dataset == ds.dataset
    # the same random stream draws the same plan with and without a mask
    import random
    assert ds.__getitem__(1, random.Random(5))["plan"] == plain.__getitem__(1, random.Random(5))["plan"]


def test_dataset_mask_errors(tmp_path):
    from e4t.data import E4TDataset
    rng = np.random.default_rng(1)
    _tree(tmp_path, rng)
    roots = f"{tmp_path / 'imgA'}::{tmp_path / 'imgB'}"
    os.remove(tmp_path / "maskA" / "sub" / "b.png")
    os.remove(tmp_path / "maskB" / "e.png")
    with pytest.raises(FileNotFoundError) as e:
        E4TDataset(roots, resolution=16, mask_dataset=f"{tmp_path / 'maskA'}::{tmp_path / 'maskB'}")
    assert "2 images" in str(e.value) and os.path.join("sub", "b") in str(e.value) and os.path.join("maskB", "e") in str(e.value)
    with pytest.raises(ValueError, match="directories"):
        E4TDataset(roots, resolution=16, mask_dataset=str(tmp_path / "maskA"))
    # wrong size: found at construction, refused when it is loaded
    _png(str(tmp_path / "maskA" / "sub" / "b.png"), np.zeros((5, 5), np.uint8))
    _png(str(tmp_path / "maskB" / "e.png"), np.zeros((23, 31), np.uint8))
    ds = E4TDataset(roots, resolution=16, mask_dataset=f"{tmp_path / 'maskA'}::{tmp_path / 'maskB'}")
    bad = ds.dataset.index(str(tmp_path / "imgA" / "sub" / "b.jpg"))
    with pytest.raises(ValueError, match="5x5"):
        ds[bad]
    ds[ds.dataset.index(str(tmp_path / "imgB" / "e.png"))]
    with pytest.raises(ValueError, match="image directories only"):
        E4TDataset("some/hub-dataset", resolution=16, mask_dataset="masks")


def test_missing_mask_error_names_at_most_five(tmp_path):
    from e4t.data import E4TDataset
    for k in range(8):
        _png(str(tmp_path / "img" / f"{k}.png"), np.zeros((16, 16, 3), np.uint8))
    os.makedirs(tmp_path / "mask")
    with pytest.raises(FileNotFoundError) as e:
        E4TDataset(str(tmp_path / "img"), resolution=16, mask_dataset=str(tmp_path / "mask"))
    assert "8 images" in str(e.value) and str(e.value).count(str(tmp_path / "mask")) == 5


def test_pack_batch_with_masks():
    from e4t.data import make_transforms, pack_batch, packed_nbytes
    rng = np.random.default_rng(2)
    samples, plain = [], []
    for (h, w) in [(16, 16), (17, 23), (33, 19)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        plan = make_transforms(16).plan(h, w)
        samples.append(dict(image=img, plan=plan, mask=rng.integers(0, 256, (h, w), dtype=np.uint8)))
        plain.append(dict(image=img, plan=plan))
    pool0, table0, total0 = pack_batch(plain, 16)
    pool, table, total, moff = pack_batch(samples, 16)
    assert moff.dtype == torch.int64 and moff.shape == (3,)
    assert torch.equal(table, table0)                               # the image part is what it is without masks (padding bytes are unspecified)
    for s, off in zip(samples, table[:, 0].tolist()):
        assert off % 16 == 0
        np.testing.assert_array_equal(pool.numpy()[off:off + s["image"].size], s["image"].reshape(-1))
        np.testing.assert_array_equal(pool0.numpy()[off:off + s["image"].size], s["image"].reshape(-1))
    assert total == packed_nbytes(samples) and total0 == packed_nbytes(plain) and total <= pool.numel()
    prev_end = total0
    for s, off in zip(samples, moff.tolist()):
        assert off % 16 == 0 and off >= prev_end
        np.testing.assert_array_equal(pool.numpy()[off:off + s["mask"].size].reshape(s["mask"].shape), s["mask"])
        prev_end = off + s["mask"].size
    assert prev_end <= total
    # a caller's buffers are filled in place
    h_pool, h_table, h_moff = torch.zeros(total + 64, dtype=torch.uint8), torch.zeros((3, 8), dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    out = pack_batch(samples, 16, h_pool, h_table, h_moff)
    assert out[0] is h_pool and out[3] is h_moff and torch.equal(h_moff, moff) and out[2] == total
    # all or none
    with pytest.raises(ValueError, match="mask"):
        pack_batch([samples[0], plain[1]], 16)
    # pack_samples, what the loader and tuning_e4t call: four values either way, None for the offsets of plain samples
    from e4t.data import pack_samples
    p4, t4, n4, m4 = pack_samples(plain, 16)
    assert m4 is None and n4 == total0 and torch.equal(t4, table0)
    p4, t4, n4, m4 = pack_samples(samples, 16)
    assert torch.equal(m4, moff) and n4 == total and torch.equal(t4, table)


# ---------------------------------------------------------------------------------------------- trainer
def _inputs(seed=7, B=2):
    g = torch.Generator().manual_seed(seed)
    return dict(pixels=torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, latents=torch.randn(B, 4, 16, 16, generator=g) * 0.18215,
                noise=torch.randn(B, 4, 16, 16, generator=g), t=torch.tensor([5, 700]), ids=torch.randint(1, 99, (B, 9), generator=g),
                pidx=torch.tensor([2, 4]), soft=torch.rand(B, 16, 16, generator=g))


def _trainer():
    from e4t.trainer import E4TTrainer
    _, _, n_unet, n_enc, text = build()
    return E4TTrainer(n_unet, n_enc, text, vae=None, lr=1e-3, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long),
                      device=torch.device("cpu"))


def test_all_ones_mask_is_the_unmasked_step(emu_fp32):
    x = _inputs()
    res = []
    for mask in (None, torch.ones(2, 16, 16)):
        tr = _trainer()
        out = tr.losses(x["pixels"], x["latents"], x["noise"], x["t"], x["ids"], x["pidx"], loss_mask=mask)
        out[0].backward()
        res.append([o.detach().clone() for o in out] + [tr.flat.grad.detach().clone()])
    for got, want in zip(res[1], res[0]):
        assert rel(got, want) <= BOUND
    assert float(res[0][3].abs().max()) > 0


def test_soft_mask_step_uses_the_given_mask(emu_fp32, monkeypatch):
    from e4t import functional as Fn
    x = _inputs()
    tr = _trainer()
    seen = []
    orig = Fn.masked_mse

    def recording(pred, target, w):
        seen.append((pred.detach().clone(), target.detach().clone(), w))
        return orig(pred, target, w)

    monkeypatch.setattr(Fn, "masked_mse", recording)
    before = tr.flat.data.detach().clone()
    loss, ld, lr_ = tr.train_step(x["pixels"], x["ids"], x["pidx"], noise=x["noise"], timesteps=x["t"], latents=x["latents"], loss_mask=x["soft"])
    assert len(seen) == 1
    pred, target, w = seen[0]
    assert w is x["soft"] and tuple(pred.shape) == (2, 4, 16, 16) and torch.equal(target, x["noise"])
    assert rel(ld, restate64(pred, target, w)[0]) <= BOUND
    assert rel(loss, ld.double() + lr_.double()) <= BOUND
    assert not torch.equal(tr.flat.data, before)                     # the optimiser stepped
    # and the mask matters: the unmasked loss of the same prediction is another number
    assert abs(float(F.mse_loss(pred, target)) - float(ld)) > 1e-4 * float(ld)


def test_masked_step_never_takes_the_graphed_path(emu_fp32, monkeypatch):
    x = _inputs()
    tr = _trainer()
    tr.enable_step_graph(True)                # (refused without a GPU; the flag is forced below)
    tr._step_graph_on = True
    taken = []
    monkeypatch.setattr(tr, "_graphed_step", lambda *a, **k: taken.append(1) or tr._train_step(*a[:3], noise=a[3], timesteps=a[4], latents=a[6]))
    out = tr.train_step(x["pixels"], x["ids"], x["pidx"], noise=x["noise"], timesteps=x["t"], latents=x["latents"], loss_mask=x["soft"])
    assert not taken and all(torch.isfinite(o) for o in out)
    tr.train_step(x["pixels"], x["ids"], x["pidx"], noise=x["noise"], timesteps=x["t"], latents=x["latents"])
    assert taken == [1]                       # the unmasked step is still routed to the graph


# ---------------------------------------------------------------------------------------------- command lines
def parse(module, argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", [f"{module}.py"] + argv)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(module).parse_args()


def test_mask_flags(monkeypatch):
    a = parse("pretrain_e4t", ["--train_image_dataset", "a::b", "--train_mask_dataset", "ma::mb"], monkeypatch)
    assert a.train_mask_dataset == "ma::mb"
    assert parse("pretrain_e4t", ["--train_image_dataset", "a"], monkeypatch).train_mask_dataset is None
    for other in ("--webdataset", "--iterable_dataset", "--synthetic_data"):
        with pytest.raises(SystemExit):
            parse("pretrain_e4t", ["--train_image_dataset", "a", "--train_mask_dataset", "m", other], monkeypatch)
    t = parse("tuning_e4t", ["--train_image_path", "x.png", "--train_mask_path", "m.png"], monkeypatch)
    assert t.train_mask_path == "m.png"
    assert parse("tuning_e4t", ["--train_image_path", "x.png"], monkeypatch).train_mask_path is None
    with pytest.raises(SystemExit):
        parse("tuning_e4t", ["--synthetic_data", "--train_mask_path", "m.png"], monkeypatch)
