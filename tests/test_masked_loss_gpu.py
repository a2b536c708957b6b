"""-m gpu: the masked diffusion loss on the real kernels — e4t_mask_prep byte-exact against the numpy oracle, DeviceLoader with masks
end to end, e4t_masked_mse_fwd / _bwd against a float64 restatement (rel-L2 <= 2e-5, the project's fp32-kernel bound), and one
masked training step at the tiny model sizes."""
import importlib
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

import image_prep_oracle as ipo
from test_masked_loss_host_logic import BOUND, ROOT, SHAPES, make_mask, rel, restate64

pytestmark = pytest.mark.gpu

DIMS_256 = [(300, 420), (512, 512), (1024, 768), (700, 933), (256, 300), (640, 512), (513, 1000), (1536, 1536), (999, 777), (520, 530)]
# one per resize branch: untouched, integer factor (2 x 2, and 3 x 3 with room to crop), general area, enlarging fixed point
DIMS_64 = [(64, 64), (128, 192), (192, 384), (100, 150), (40, 50)]


def block_weights(px_channel):
    """fp32 [S, S] in [-1, 1] as image_prep writes it -> the loss weights e4t_mask_prep defines: bytes recovered, summed as integers over
    8 x 8 blocks, float32(float64(s) / 16320)"""
    u = np.rint((px_channel.astype(np.float64) + 1.0) * 127.5).astype(np.int64)
    S = u.shape[0]
    s = u.reshape(S // 8, 8, S // 8, 8).sum(axis=(1, 3))
    return (s.astype(np.float64) / 16320.0).astype(np.float32)


@pytest.mark.parametrize("S,dims", [(256, DIMS_256), (64, DIMS_64)], ids=["S256", "S64_branches"])
def test_mask_prep_is_exact(hip_env, S, dims):
    from e4t.data import pack_batch
    hip, emu, dev, ops = hip_env
    rng = np.random.default_rng(S)
    samples = []
    for (H, W) in dims:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        mask = rng.integers(0, 256, (H, W), dtype=np.uint8)
        nh, nw = ipo.smallest_max_size_dims(H, W, S)
        for flip in (0, 1):
            y0, x0 = ipo.random_crop_origin(nh, nw, S, rng.random(), rng.random())
            samples.append(dict(image=img, mask=mask, plan=(nh, nw, y0, x0, flip)))
    assert sum(1 for s in samples if s["plan"][2] > 0 or s["plan"][3] > 0) >= len(dims)          # non-zero crop origins are in
    B = len(samples)
    pool, table, total, moff = pack_batch(samples, S)
    d_pool, d_table, d_moff = pool.to(dev), table.to(dev), moff.to(dev)
    d_table[:, 0] = -(1 << 40)                                   # column 0 (the image's offset) is not the mask kernel's business
    got = hip.mask_prep(d_pool, d_table, d_moff, B, S)
    assert got.shape == (B, S // 8, S // 8) and got.dtype == torch.float32
    got = got.cpu().numpy()
    for i, smp in enumerate(samples):
        nh, nw, y0, x0, flip = smp["plan"]
        want = block_weights(ipo.image_prep(np.repeat(smp["mask"][:, :, None], 3, axis=2), S, y0, x0, bool(flip))[0])
        np.testing.assert_array_equal(got[i], want, err_msg=f"{smp['mask'].shape} -> {nh}x{nw} crop ({y0},{x0}) flip {flip}")
    # the image kernel on the same pool and (intact) table is untouched by the masks packed behind the images
    px = hip.image_prep(d_pool, table.to(dev), B, S).cpu().numpy()
    for i in (0, B - 1):
        nh, nw, y0, x0, flip = samples[i]["plan"]
        np.testing.assert_array_equal(px[i], ipo.image_prep(samples[i]["image"], S, y0, x0, bool(flip)))


def test_device_loader_hands_out_aligned_masks(hip_env, tmp_path):
    """PNG images whose mask is their own red channel: the loss mask must be the 8 x 8 block mean of the red channel the image kernel
    wrote — same samples, same order, same resize branch, crop window and flip in both kernels."""
    from e4t.data import DeviceLoader, E4TDataset
    hip, emu, dev, ops = hip_env
    rng = np.random.default_rng(5)
    dims = [(64, 64), (128, 192), (100, 150), (40, 50), (97, 131), (192, 256), (70, 64), (200, 77), (65, 90)]
    iroot, mroot = tmp_path / "imgs", tmp_path / "masks"
    iroot.mkdir(), mroot.mkdir()
    for i, (h, w) in enumerate(dims):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(a).save(iroot / f"{i:02d}.png")
        Image.fromarray(a[:, :, 0]).save(mroot / f"{i:02d}.png")
    masked = DeviceLoader(E4TDataset(str(iroot), resolution=64, mask_dataset=str(mroot)), batch_size=3, shuffle=True, num_workers=3, device=dev, seed=1)
    plain = DeviceLoader(E4TDataset(str(iroot), resolution=64), batch_size=3, shuffle=True, num_workers=3, device=dev, seed=1)
    seen = 0
    for epoch in range(2):
        ref = [b["pixel_values"].clone() for b in plain]
        n = 0
        for k, batch in enumerate(masked):
            assert set(batch) == {"pixel_values", "loss_mask"}
            px, lm = batch["pixel_values"], batch["loss_mask"]
            assert lm.is_cuda and lm.dtype == torch.float32 and lm.shape == (3, 8, 8) and px.shape == (3, 3, 64, 64)
            assert torch.equal(px, ref[k])                        # the image path is the mask-free one, bit for bit
            pxn, lmn = px.cpu().numpy(), lm.cpu().numpy()
            for j in range(3):
                np.testing.assert_array_equal(lmn[j], block_weights(pxn[j, 0]))
                seen += 1
            n += 1
        assert n == len(ref) == 3
    assert seen == 18
    it = iter(plain)
    assert set(next(it)) == {"pixel_values"}
    it.close()


def _red_channel_tree(tmp_path, dims, seed):
    """PNG images under imgs/, and under masks/ each image's own red channel as its mask"""
    rng = np.random.default_rng(seed)
    iroot, mroot = tmp_path / "imgs", tmp_path / "masks"
    iroot.mkdir(), mroot.mkdir()
    for i, (h, w) in enumerate(dims):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(a).save(iroot / f"{i:02d}.png")
        Image.fromarray(a[:, :, 0]).save(mroot / f"{i:02d}.png")
    return iroot, mroot


def _script(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(name)


def test_pretraining_batches_keep_their_mask_across_the_look_ahead(hip_env, tmp_path):
    """pretrain_e4t.main draws batch k+1 before it runs step k, and the mask of batch k is read only at the end of step k: the mask
    that image_batches hands out must still be batch k's after later batches have been drawn, however far the loader has run ahead
    (it has four buffers, so batch k+4 is written where batch k was)."""
    from e4t.data import DeviceLoader, E4TDataset
    hip, emu, dev, ops = hip_env
    dims = [(64, 64), (128, 192), (100, 150), (40, 50), (97, 131), (192, 256), (70, 64), (200, 77), (65, 90)]
    iroot, mroot = _red_channel_tree(tmp_path, dims, seed=6)
    # what every batch is: a loader of the same seed, each batch looked at as soon as it is handed out
    ref = DeviceLoader(E4TDataset(str(iroot), resolution=64, mask_dataset=str(mroot)), batch_size=1, shuffle=True, num_workers=2, device=dev, seed=4)
    want = []
    for epoch in range(2):
        for batch in ref:
            w = batch["loss_mask"].cpu().numpy()
            np.testing.assert_array_equal(w[0], block_weights(batch["pixel_values"][0, 0].cpu().numpy()))
            want.append(w)
    assert len(want) == 18
    assert all(not np.array_equal(want[k], want[k + 4]) for k in range(5))        # other images: a shared buffer would show
    args = types.SimpleNamespace(webdataset=False, train_image_dataset=str(iroot), train_mask_dataset=str(mroot), resolution=64,
                                 train_batch_size=1, dataloader_num_workers=2, seed=4)
    data = _script("pretrain_e4t").image_batches(args, dev, 0, 1, lambda n: (None, None))
    held = []
    pending = next(data)
    for k in range(12):                                  # past one epoch (9 batches), and three times round the loader's buffers
        batch = pending
        pending = next(data)                             # the look-ahead of the training loop
        assert len(batch) == 4 and batch[3].shape == (1, 8, 8)
        np.testing.assert_array_equal(batch[3].cpu().numpy(), want[k], err_msg=f"batch {k} after batch {k + 1} was drawn")
        held.append(batch[3])
    data.close()
    torch.cuda.synchronize()
    for k, m in enumerate(held):                         # and still, with every later batch drawn: nothing shares a buffer
        np.testing.assert_array_equal(m.cpu().numpy(), want[k], err_msg=f"batch {k} at the end")


def test_tuning_image_and_mask_share_one_plan(hip_env, tmp_path):
    """tuning_e4t.training_image: the mask goes through the image's resize, crop and flip, is expanded to the batch, and is kept
    next to domain.png"""
    hip, emu, dev, ops = hip_env
    iroot, mroot = _red_channel_tree(tmp_path, [(150, 233)], seed=8)
    tuning = _script("tuning_e4t")
    for seed in (0, 1, 2, 3):                            # several crops, both flips most likely; every one must line up
        args = types.SimpleNamespace(train_batch_size=3, resolution=64, synthetic_data=False, seed=seed,
                                     train_image_path=str(iroot / "00.png"), train_mask_path=str(mroot / "00.png"))
        pixels, loss_mask, pil_image, pil_mask = tuning.training_image(args, dev, None)
        assert pixels.shape == (3, 3, 64, 64) and loss_mask.shape == (3, 8, 8) and loss_mask.dtype == torch.float32
        assert loss_mask.is_contiguous() and pixels.is_contiguous()
        px, lm = pixels.cpu().numpy(), loss_mask.cpu().numpy()
        for j in range(3):
            np.testing.assert_array_equal(lm[j], block_weights(px[j, 0]))
    tuning.save_domain_images(str(tmp_path), pil_image, pil_mask)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "domain_mask.png")), np.asarray(Image.open(mroot / "00.png")))
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "domain.png")), np.asarray(Image.open(iroot / "00.png")))
    args.train_mask_path = None
    assert tuning.training_image(args, dev, None)[1::2] == (None, None)
    (h, w) = (10, 12)
    Image.fromarray(np.zeros((h, w), np.uint8)).save(tmp_path / "small.png")
    args.train_mask_path = str(tmp_path / "small.png")
    with pytest.raises(SystemExit):
        tuning.training_image(args, dev, None)


def _operands(shape, nhwc, kind, dev, seed=0):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(seed + B * 1000 + h)
    base = torch.randn((B, h, w, C) if nhwc else shape, generator=g).to(dev).requires_grad_(True)
    pred = base.permute(0, 3, 1, 2) if nhwc else base
    target = torch.randn(shape, generator=g).to(dev)
    return base, pred, target, make_mask(kind, B, h, w, g).to(dev)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", SHAPES + [(16, 4, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_masked_mse_kernels(hip_env, shape, nhwc):
    from e4t import functional as Fn
    hip, emu, dev, ops = hip_env
    assert ops.backend().name == "hip"
    for kind in ("soft", "ones", "zero"):
        base, pred, target, m = _operands(shape, nhwc, kind, dev)
        loss = Fn.masked_mse(pred, target, m)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        (loss * 3.0).backward()                                   # an upstream gradient other than 1
        dpred = base.grad.permute(0, 3, 1, 2) if nhwc else base.grad
        want, dwant = restate64(pred.cpu(), target.cpu(), m.cpu())
        if kind == "zero":
            assert float(loss.detach()) == 0.0 and float(dpred.abs().max()) == 0.0
            continue
        r_loss, r_grad = rel(loss.detach().cpu(), want), rel(dpred.cpu(), 3.0 * dwant)
        print(f"masked_mse {shape} nhwc={nhwc} {kind}: rel loss {r_loss:.3e} dpred {r_grad:.3e}")
        assert r_loss <= BOUND and r_grad <= BOUND
        if kind == "ones":
            assert rel(loss.detach().cpu(), torch.nn.functional.mse_loss(pred.detach(), target).cpu()) <= BOUND
    # run to run: bitwise; the gradient comes back in pred's own layout
    base, pred, target, m = _operands(shape, nhwc, "soft", dev, seed=1)
    g = torch.full((), 0.5, device=dev)
    runs = []
    for _ in range(2):
        loss, wd, stats = hip.masked_mse(pred.detach(), target, m)
        dp = hip.masked_mse_bwd(wd, stats, g)
        assert dp.shape == pred.shape and (pred.is_contiguous() or (dp.stride() == pred.stride() and wd.stride() == pred.stride()))
        runs.append((loss.clone(), dp.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_masked_mse_forward_replays_from_a_graph(hip_env):
    hip, emu, dev, ops = hip_env
    base, pred, target, m = _operands((3, 4, 5, 7), True, "soft", dev, seed=2)
    pred = pred.detach()
    eager = hip.masked_mse(pred, target, m)[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard():
        with torch.cuda.graph(graph):
            loss, wd, stats = hip.masked_mse(pred, target, m)
    loss.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager)
    # new values in the captured buffers, same graph
    target.mul_(0.5)
    graph.replay()
    assert torch.equal(loss, hip.masked_mse(pred, target, m)[0])


# ---------------------------------------------------------------------------------------------- one masked training step
def _tiny_trainer(dev):
    from test_train_step_host_logic import TEXT_CFG, build
    from e4t.text import CLIPTextModel
    from e4t.trainer import E4TTrainer
    _, _, n_unet, n_enc, text_t = build(seed=0)
    text = CLIPTextModel(**TEXT_CFG).requires_grad_(False)
    text.load_state_dict(text_t.state_dict())
    n_unet.to(dev), n_enc.to(dev), text.to(dev)
    return E4TTrainer(n_unet, n_enc, text, vae=None, lr=1e-3, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long, device=dev), device=dev)


def _tiny_batches(dev, n, B=2):
    g = torch.Generator().manual_seed(3)
    out = []
    for _ in range(n):
        b = dict(px=torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, lat=torch.randn(B, 4, 16, 16, generator=g) * 0.18215,
                 noise=torch.randn(B, 4, 16, 16, generator=g), t=torch.randint(0, 1000, (B,), generator=g), ids=torch.randint(1, 99, (B, 9), generator=g),
                 mask=torch.rand(B, 16, 16, generator=g))
        out.append({k: v.to(dev) for k, v in b.items()})
    return out


def test_masked_training_step(hip_env, monkeypatch):
    from e4t import functional as Fn
    hip, emu, dev, ops = hip_env
    (b,) = _tiny_batches(dev, 1)
    pidx = torch.tensor([2, 4], device=dev)
    seen = []
    orig = Fn.masked_mse

    def recording(pred, target, w):
        seen.append((pred.detach().clone(), target.detach().clone(), w))
        return orig(pred, target, w)

    monkeypatch.setattr(Fn, "masked_mse", recording)
    runs = []
    for _ in range(2):
        tr0, tr = _tiny_trainer(dev), _tiny_trainer(dev)
        out = tr0.losses(b["px"], b["lat"], b["noise"], b["t"], b["ids"], pidx, loss_mask=b["mask"])
        out[0].backward()
        grad = tr0.flat.grad.detach().clone()
        step = tr.train_step(b["px"], b["ids"], pidx, noise=b["noise"], timesteps=b["t"], latents=b["lat"], loss_mask=b["mask"])
        torch.cuda.synchronize()
        runs.append((torch.stack([o.detach().float() for o in out]).cpu(), grad.cpu(), torch.stack([o.detach().float() for o in step]).cpu(),
                     tr.flat.data.detach().cpu().clone()))
    assert len(seen) == 4
    pred, target, w = seen[0]
    assert w is b["mask"] and float(runs[0][1].abs().max()) > 0
    want = restate64(pred.cpu(), target.cpu(), w.cpu())[0]
    r = rel(runs[0][0][1], want)
    print(f"masked step loss_diff {float(runs[0][0][1]):.6f} vs float64 restatement {float(want):.6f}: rel {r:.3e}")
    assert r <= BOUND
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)


def test_masked_step_with_step_graph_enabled_equals_eager(hip_env):
    """a step with a loss mask runs eagerly even when the step graph is on (no capture, no replay), with the eager result"""
    hip, emu, dev, ops = hip_env
    batches = _tiny_batches(dev, 3)
    pidx = torch.tensor([2, 4], device=dev)

    def run(graph):
        tr = _tiny_trainer(dev)
        assert tr.enable_step_graph(True)
        tr._step_graph_on = graph              # the eager leg keeps the device-side AdamW scalars, as in test_step_graph_replay_equals_eager
        losses = []
        for b in batches:
            out = tr.train_step(b["px"], b["ids"], pidx, noise=b["noise"], timesteps=b["t"], latents=b["lat"], loss_mask=b["mask"])
            losses.append(torch.stack([o.detach().float() for o in out]).cpu())
        torch.cuda.synchronize()
        return torch.stack(losses), tr.flat.data.detach().cpu().clone(), len(tr._step_graphs), len(tr._seen_sigs)

    l0, p0, _, _ = run(False)
    l1, p1, n1, s1 = run(True)
    assert n1 == 0 and s1 == 0
    assert torch.equal(l0, l1), (l0, l1)
    assert torch.equal(p0, p1), float((p0 - p1).abs().max())
