"""-m gpu: token merging (csrc/tome.hip, e4t/tome.py) on the real kernels against the torch restatement (tests/tome_reference.py):
the match as properties of the plan and exactly on a tie-free input, merge / unmerge with the kernel's own plan, one ToMe'd
BasicTransformerBlock forward and every gradient against the bf16 op emulation with the GPU's plan injected, and a tiny-model
training step / sampling loop (finite, bitwise reproducible, graph replay == eager)."""
import ctypes as C

import pytest
import torch

import tome_reference as ref

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16


def _r(T, ratio):
    return min(T - T // 4, int(T * ratio))


def _choice(h, w, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 4, ((h // 2) * (w // 2),), generator=g, dtype=torch.int32).to(dev)


def _x(B, T, d, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, d, generator=g) * (0.5 + torch.rand(B, T, 1, generator=g))).to(bf16).to(dev)


def _abi(plan):
    return plan.buf[: plan.B * (2 * plan.T + plan.nd + 1)].clone()


# (B, h, w, d, ratio or None, r or None, random choice)
MATCH_CASES = [
    (2, 8, 8, 64, 0.5, None, False),       # smallest
    (2, 24, 24, 320, 0.5, None, True),     # ragged src and dst tiles
    (3, 10, 6, 64, 0.25, None, True),      # non-square
    (2, 24, 24, 320, 0.75, None, True),    # r = ns: no unmerged rows
    (2, 8, 8, 64, None, 1, False),         # one merge
    (1, 64, 64, 320, 0.5, None, True),     # the real level
    (1, 96, 96, 64, 0.5, None, False),     # T = 9216
    (1, 8, 12, 640, 0.5, None, True),      # the score kernel's d <= 640 and d <= 1280 instantiations (levels a max_downsample > 1 reaches)
    (1, 8, 8, 1280, 0.5, None, True),
]


@pytest.mark.parametrize("case", MATCH_CASES, ids=lambda c: "B%d_%dx%d_d%d_%s" % (c[0], c[1], c[2], c[3], c[4] if c[4] else "r%d" % c[5]))
def test_match_plan_properties(hip_env, case):
    hip, _, dev, _ = hip_env
    B, h, w, d, ratio, r, rand = case
    T, nd = h * w, h * w // 4
    ns = T - nd
    r = r if r is not None else _r(T, ratio)
    choice = _choice(h, w, 11, dev) if rand else None
    x = _x(B, T, d, 5, dev)
    plan = hip.tome_match(x.reshape(B * T, d), B, h, w, r, choice)
    first = _abi(plan)
    for _ in range(2):       # launch determinism: three launches, one plan
        assert torch.equal(_abi(hip.tome_match(x.reshape(B * T, d), B, h, w, r, choice)), first)
    mp, row_tok, so, ss = (t.cpu().to(torch.int64) for t in (plan.map, plan.row_tok, plan.seg_off, plan.seg_src))
    dst, src = ref.split_tokens(h, w, choice)
    assert plan.Tm == T - r and mp.min() >= 0 and mp.max() < plan.Tm and row_tok.min() >= 0 and row_tok.max() < T
    is_src = torch.zeros(T, dtype=torch.bool)
    is_src[src] = True
    src_pos = torch.full((T,), -1, dtype=torch.int64)
    src_pos[src] = torch.arange(ns)
    s64 = ref.scores(x, h, w, choice, torch.float64).cpu()           # fp64 scores of the same bf16 x^
    eps = d * 2.0 ** -23
    for b in range(B):
        # the dst tokens are the ones `choice` names; map and row_tok are mutually inverse
        assert torch.equal(row_tok[b, :nd], dst) and torch.equal(mp[b, dst], torch.arange(nd))
        assert torch.equal(mp[b, row_tok[b]], torch.arange(plan.Tm))
        cnt = torch.ones(plan.Tm, dtype=torch.int64)
        cnt[:nd] += so[b, 1:] - so[b, :-1]
        assert so[b, 0] == 0 and so[b, -1] == r and bool((so[b, 1:] >= so[b, :-1]).all())
        assert int(cnt.sum()) == T
        assert torch.equal(cnt, torch.bincount(mp[b], minlength=plan.Tm))
        single = cnt[mp[b]] == 1
        assert torch.equal(row_tok[b, mp[b][single]], torch.arange(T)[single])
        # exactly r src tokens are merged, each into the row of its segment, ascending within the segment
        seg_of = torch.repeat_interleave(torch.arange(nd), so[b, 1:] - so[b, :-1])
        assert bool(is_src[ss[b]].all()) and ss[b].unique().numel() == r
        assert torch.equal(mp[b, ss[b]], seg_of)
        same = seg_of[1:] == seg_of[:-1]
        assert bool((ss[b, 1:] > ss[b, :-1])[same].all())
        merged = torch.zeros(T, dtype=torch.bool)
        merged[ss[b]] = True
        un = src[~merged[src]]
        assert torch.equal(row_tok[b, nd:], un)                      # the unmerged src in ascending token order
        # against the fp64 scores: the chosen dst is a row maximum, the merged src are the top r — both to eps = d 2^-23 (twice the
        # worst-case fp32 error of a d-term dot product of unit vectors)
        rowmax = s64[b].max(-1).values
        chosen = s64[b][src_pos[ss[b]], seg_of]
        worst = float((rowmax[src_pos[ss[b]]] - chosen).max())
        print(f"image {b}: chosen dst below the row max by at most {worst:.3e} (eps {eps:.3e})")
        assert worst <= eps
        if un.numel():
            gap = float(rowmax[src_pos[ss[b]]].min() - rowmax[src_pos[un]].max())
            print(f"image {b}: weakest merged node_max - strongest unmerged = {gap:.3e}")
            assert gap >= -eps


def _tie_free_input(B, h, w, d, r, choice, seed):
    """dst tokens = random directions; every src = its assigned dst + noise (sigma 0.1 for exactly r of them, 1.0 for the rest),
    rows rescaled by random positive factors"""
    g = torch.Generator().manual_seed(seed)
    T, nd = h * w, h * w // 4
    ns = T - nd
    dst, src = ref.split_tokens(h, w, choice)
    x = torch.empty(B, T, d)
    for b in range(B):
        dv = torch.nn.functional.normalize(torch.randn(nd, d, generator=g), dim=-1)
        assign = torch.randint(0, nd, (ns,), generator=g)
        sigma = torch.full((ns,), 1.0)
        sigma[torch.randperm(ns, generator=g)[:r]] = 0.1
        x[b, dst] = dv
        x[b, src] = dv[assign] + torch.randn(ns, d, generator=g) * (sigma / d ** 0.5)[:, None]
    return (x * (0.25 + 4 * torch.rand(B, T, 1, generator=g))).to(bf16)


def test_match_equals_restatement_on_tie_free_input(hip_env):
    hip, _, dev, _ = hip_env
    B, h, w, d = 2, 24, 24, 320
    T = h * w
    r = T // 2
    choice = _choice(h, w, 3, dev)
    x = _tie_free_input(B, h, w, d, r, choice, 17).to(dev)
    s = ref.scores(x, h, w, choice, torch.float64)
    top2 = s.topk(2, dim=-1).values
    nm = top2[..., 0].sort(dim=-1, descending=True).values
    assert float((top2[..., 0] - top2[..., 1]).min()) > 0.1 and float((nm[:, r - 1] - nm[:, r]).min()) > 0.05     # no tie anywhere
    want = ref.match_plan(x, h, w, r, choice)
    got = hip.tome_match(x.reshape(B * T, d), B, h, w, r, choice)
    for k, v in got.fields().items():
        assert torch.equal(v.cpu(), want[k]), k


def _raw_merge(hip, x, ldx, plan, y, ldy, d, mean):
    from e4t import _C, ops
    _C.check(hip.lib.e4t_tome_merge(x.data_ptr(), ldx, plan.buf.data_ptr(), y.data_ptr(), ldy, plan.B, plan.T, plan.r, d, int(mean), ops._stream()), "merge")


def _raw_unmerge(hip, y, ldy, plan, res, xo, ldx, d, scale):
    from e4t import _C, ops
    _C.check(hip.lib.e4t_tome_unmerge(y.data_ptr(), ldy, plan.buf.data_ptr(), None if res is None else res.data_ptr(), xo.data_ptr(), ldx,
                                      plan.B, plan.T, plan.r, d, int(scale), ops._stream()), "unmerge")


@pytest.mark.parametrize("case", [(2, 24, 24, 320, 0.5), (3, 10, 6, 64, 0.25), (2, 8, 8, 64, 0.75)], ids=str)
def test_merge_unmerge_match_restatement(hip_env, case):
    hip, _, dev, _ = hip_env
    B, h, w, d, ratio = case
    T = h * w
    r = _r(T, ratio)
    # clustered rows, so that segments of several src tokens exist
    g = torch.Generator().manual_seed(2)
    centres = torch.randn(B, 12, d, generator=g)
    x = (centres[:, torch.randint(0, 12, (T,), generator=g)] + 0.3 * torch.randn(B, T, d, generator=g)).to(bf16).to(dev)
    plan = hip.tome_match(x.reshape(B * T, d), B, h, w, r, _choice(h, w, 4, dev))
    cnt = ref.counts(plan)
    assert int(cnt.max()) >= 3
    Tm = plan.Tm
    # merge: count-1 rows are copies, merged rows within the single-rounding bf16 bound of the fp32 restatement
    for mean in (True, False):
        y = hip.tome_merge(x.reshape(B * T, d), plan, mean=mean).view(B, Tm, d)
        want = ref.merge(x, plan, mean=mean)
        one = cnt == 1
        assert torch.equal(y[one], x[torch.arange(B, device=dev)[:, None].expand_as(one)[one], plan.row_tok.to(torch.int64)[one]])
        rel = float((y.float() - want).norm() / want.norm())
        per = [float((y[b].float() - want[b]).norm() / want[b].norm()) for b in range(B)]
        print(f"merge mean={mean}: rel-L2 {rel:.3e}, per image {per}")
        assert rel <= 6e-3 and max(per) <= 6e-3
        assert torch.equal(y, want.to(bf16))          # (same accumulation order: in fact bitwise)
    # unmerge: bitwise, with / without residual and 1/count scale
    g2 = torch.Generator().manual_seed(8)
    ym = torch.randn(B, Tm, d, generator=g2).to(bf16).to(dev)
    res = torch.randn(B, T, d, generator=g2).to(bf16).to(dev)
    for use_res in (False, True):
        for scale in (False, True):
            got = hip.tome_unmerge(ym.reshape(B * Tm, d), plan, residual=res.reshape(B * T, d) if use_res else None, scale=scale)
            want = ref.unmerge(ym, plan, res if use_res else None, scale).to(bf16)
            assert torch.equal(got.view(B, T, d), want), (use_res, scale)
    # row strides beyond dense: NaN in the gaps of the inputs, sentinels around and between the output rows
    ld = d + 8
    nan, sent = float("nan"), -7.0
    xs = torch.full((B * T, ld), nan, dtype=bf16, device=dev)
    xs[:, :d] = x.reshape(B * T, d)
    ybuf = torch.full((B * Tm + 2, ld), sent, dtype=bf16, device=dev)
    _raw_merge(hip, xs, ld, plan, ybuf[1:], ld, d, True)
    assert torch.equal(ybuf[1:-1, :d], hip.tome_merge(x.reshape(B * T, d), plan))
    assert bool((ybuf[0] == sent).all()) and bool((ybuf[-1] == sent).all()) and bool((ybuf[:, d:] == sent).all())
    ys = torch.full((B * Tm, ld), nan, dtype=bf16, device=dev)
    ys[:, :d] = ym.reshape(B * Tm, d)
    rs = torch.full((B * T, ld), nan, dtype=bf16, device=dev)
    rs[:, :d] = res.reshape(B * T, d)
    xbuf = torch.full((B * T + 2, ld), sent, dtype=bf16, device=dev)
    _raw_unmerge(hip, ys, ld, plan, rs, xbuf[1:], ld, d, True)
    assert torch.equal(xbuf[1:-1, :d], hip.tome_unmerge(ym.reshape(B * Tm, d), plan, residual=res.reshape(B * T, d), scale=True))
    assert bool((xbuf[0] == sent).all()) and bool((xbuf[-1] == sent).all()) and bool((xbuf[:, d:] == sent).all())


def test_match_rejects_bad_arguments_before_any_launch(hip_env):
    hip, _, dev, _ = hip_env
    x = torch.zeros(64, 64, dtype=bf16, device=dev)
    buf = torch.zeros(4096, dtype=torch.int32, device=dev)
    call = lambda ld, h, w, d, r: hip.lib.e4t_tome_match(x.data_ptr(), ld, 1, h, w, d, r, None, buf.data_ptr(), None)
    assert call(64, 8, 8, 64, 16) == 0
    for bad in ((64, 8, 8, 24, 16), (64, 7, 8, 64, 16), (64, 8, 9, 64, 16), (64, 8, 8, 64, 0), (64, 8, 8, 64, 49), (64, 130, 128, 64, 16)):
        assert call(*bad) == -22, bad
    torch.cuda.synchronize()


def _block_leg(backend, ops, dev, d, heads, hw, B, sd, x0, ctx0, wout, plans, record):
    """one ToMe'd BasicTransformerBlock forward + backward on `backend` -> (output, gradients, recorded plans)"""
    from e4t import tome
    from e4t.models.attention import BasicTransformerBlock
    from e4t.weightoffsets import WOBank
    old = ops.set_backend(backend)
    try:
        blk = BasicTransformerBlock(d, heads, d // heads, cross_attention_dim=ctx0.shape[-1])
        blk.load_state_dict(sd)
        blk.to(dev)
        for n, p in blk.named_parameters():      # the pre-training split, plus what attn1's neighbours need to be checked
            p.requires_grad_("wo" in n or n.startswith("norm1") or n.startswith("attn1.to_out"))
        bank = WOBank("t")
        blk.attn1.register_bank(bank)
        blk.attn2.register_bank(bank)
        st = tome.TomeState(0.5, use_rand=False)
        st.latent_tokens, st.plans, st.record = hw[0] * hw[1], plans, record
        blk._tome = st
        x = x0.to(dev).to(ops.ACT).requires_grad_(True)
        bank.begin(dev)
        y = blk(x, encoder_hidden_states=ctx0.to(dev).to(ops.ACT), hw=hw)
        (y.float() * wout.to(dev)).sum().backward()
        grads = {"x": x.grad.float().cpu()}
        for n, p in blk.named_parameters():
            if p.requires_grad and (n.startswith("norm1") or n.startswith("attn1")):
                assert p.grad is not None, n
                grads[n] = p.grad.float().cpu()
        return y.detach().float().cpu(), grads, st.recorded
    finally:
        ops.set_backend(old)


@pytest.mark.parametrize("d,heads,hw", [(64, 2, (16, 16)), (320, 8, (24, 24))], ids=["d64_16x16", "d320_24x24"])
def test_tomed_block_forward_and_gradients(hip_env, d, heads, hw):
    """the GPU leg records its plan, the bf16-rounding emulation gets that plan injected: both merge the same tokens, whatever either
    would make of a near-tie.  rel-L2 <= 1.5e-2: the project's bound for chains with an in-kernel bf16 intermediate."""
    hip, _, dev, ops = hip_env
    from e4t.models.attention import BasicTransformerBlock
    B, T = 2, hw[0] * hw[1]
    torch.manual_seed(0)
    sd = BasicTransformerBlock(d, heads, d // heads, cross_attention_dim=64).state_dict()
    g = torch.Generator().manual_seed(1)
    for k in sd:                                  # weight offsets start at zero: give them (and the LN affine) something to differentiate
        if "wo_" in k or k.startswith("norm1"):
            sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=g)
    x0 = torch.randn(B, T, d, generator=g).to(bf16).float()
    ctx0 = torch.randn(B, 7, 64, generator=g).to(bf16).float()
    wout = torch.randn(B, T, d, generator=g)
    y_g, g_g, plans = _block_leg(hip, ops, dev, d, heads, hw, B, sd, x0, ctx0, wout, None, True)
    assert len(plans) == 1 and plans[0].Tm == T - T // 2
    y_e, g_e, _ = _block_leg(ref.TomeEmuBackend(), ops, dev, d, heads, hw, B, sd, x0, ctx0, wout, plans, False)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    print(f"forward rel-L2 {rel(y_g, y_e):.3e}")
    assert rel(y_g, y_e) <= 1.5e-2
    assert set(g_g) == set(g_e) and any("wo_q" in n for n in g_g) and any("to_out.0.weight" in n for n in g_g)
    for n in g_g:
        assert torch.isfinite(g_g[n]).all(), n
        e = rel(g_g[n], g_e[n]) if float(g_e[n].norm()) > 0 else float(g_g[n].norm())
        print(f"grad {n}: rel-L2 {e:.3e}")
        assert e <= 1.5e-2, (n, e)


def _tiny_trainer(dev, use_rand, graph):
    from test_train_step_host_logic import TEXT_CFG, build
    from e4t import tome
    from e4t.text import CLIPTextModel
    from e4t.trainer import E4TTrainer
    _, _, n_unet, n_enc, text_t = build(seed=0)
    text = CLIPTextModel(**TEXT_CFG).requires_grad_(False)
    text.load_state_dict(text_t.state_dict())
    n_unet.to(dev), n_enc.to(dev), text.to(dev)
    st = tome.apply_tome(n_unet, 0.5, use_rand=use_rand, generator=torch.Generator().manual_seed(9), record=True)
    tr = E4TTrainer(n_unet, n_enc, text, vae=None, lr=1e-3, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long, device=dev), device=dev)
    assert tr.enable_step_graph(True)
    tr._step_graph_on = graph                  # the eager leg keeps the device-side AdamW scalars (as test_step_graph_replay_equals_eager does)
    return tr, st


@pytest.mark.parametrize("use_rand", [True, False], ids=["rand", "no_rand"])
def test_tiny_training_step_with_tome(hip_env, use_rand):
    """ratio 0.5 on the tiny model (its 16x16 level, d = 64): losses and gradients finite, two runs bitwise equal, and the step graph
    (1 eager warm-up, 1 capture + replay, 1 replay; the choice buffer refreshed in place before every replay) equals the eager run bitwise"""
    hip, _, dev, _ = hip_env
    g = torch.Generator().manual_seed(3)
    B = 2
    batches = [(torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, torch.randn(B, 4, 16, 16, generator=g) * 0.18215,
                torch.randn(B, 4, 16, 16, generator=g), torch.randint(0, 1000, (B,), generator=g), torch.randint(1, 99, (B, 9), generator=g))
               for _ in range(3)]
    pidx = torch.tensor([2, 4], device=dev)

    def run(graph):
        tr, st = _tiny_trainer(dev, use_rand, graph)
        losses, choices = [], []
        for px, lat, noise, t, ids in batches:
            out = tr.train_step(px.to(dev), ids.to(dev), pidx, noise=noise.to(dev), timesteps=t.to(dev), latents=lat.to(dev))
            losses.append(torch.stack([o.detach().float() for o in out]).cpu())
            if use_rand:
                choices.append(st.choice(16, 16, dev).cpu().clone())
        torch.cuda.synchronize()
        return torch.stack(losses), tr.flat.data.detach().cpu().clone(), choices, st, len(tr._step_graphs)

    l0, p0, c0, st0, n0 = run(False)
    assert torch.isfinite(l0).all() and torch.isfinite(p0).all()
    assert n0 == 0 and len(st0.recorded) == 3 * 6 and all(p.Tm == 128 for p in st0.recorded)     # ToMe really ran: 6 block calls a step
    if use_rand:
        assert not torch.equal(c0[0], c0[1]) and not torch.equal(c0[1], c0[2])                  # one draw per step
    l1, p1, c1, _, _ = run(False)
    assert torch.equal(l0, l1) and torch.equal(p0, p1)
    l2, p2, c2, _, n2 = run(True)
    assert n2 == 1
    assert all(torch.equal(a, b) for a, b in zip(c0, c2))
    assert torch.equal(l0, l2), (l0, l2)
    assert torch.equal(p0, p2), float((p0 - p2).abs().max())
    # gradients of one step (no optimiser): finite and not all zero
    tr, _ = _tiny_trainer(dev, use_rand, False)
    px, lat, noise, t, ids = batches[0]
    loss, _, _ = tr.losses(px.to(dev), lat.to(dev), noise.to(dev), t.to(dev), ids.to(dev), pidx)
    loss.backward()
    assert torch.isfinite(tr.flat.grad).all() and float(tr.flat.grad.abs().max()) > 0


def test_tiny_pipeline_with_tome_graph_equals_eager(hip_env):
    """4 denoising steps, one image: the hipGraph loop (choice refreshed in its fixed buffer before every replay) against the eager loop"""
    from word_tokenizer import WordTokenizer
    from test_train_step_host_logic import build
    from e4t import tome
    from e4t.pipeline_stable_diffusion_e4t import StableDiffusionE4TPipeline
    from e4t.schedulers import DDIMScheduler
    from e4t.text import CLIPTextModel
    from e4t.vae import VAEDecoder
    dev = torch.device("cuda:0")
    _, _, n_unet, n_enc, text_t = build()
    text = CLIPTextModel(**text_t.config).requires_grad_(False)
    text.load_state_dict(text_t.state_dict())
    pipe = StableDiffusionE4TPipeline(vae=VAEDecoder(block_out_channels=(64, 64)).requires_grad_(False), text_encoder=text, tokenizer=WordTokenizer(),
                                      unet=n_unet, e4t_encoder=n_enc, scheduler=DDIMScheduler.stable_diffusion(), safety_checker=None,
                                      e4t_config=dict(placeholder_token="*s", domain_class_token="art", domain_embed_scale=0.1)).to(dev)
    g = torch.Generator().manual_seed(5)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    lat0 = torch.randn(1, 4, 16, 16, generator=g)
    kw = dict(height=32, width=32, num_inference_steps=4, guidance_scale=5.0, num_images_per_prompt=1, image=image, output_type="latent")
    plain = pipe("a painting of *s", latents=lat0.clone(), use_graph=False, **kw).images
    outs = []
    for use_graph in (False, True):
        st = tome.apply_tome(n_unet, 0.5, generator=torch.Generator().manual_seed(2), record=True)
        outs.append(pipe("a painting of *s", latents=lat0.clone(), use_graph=use_graph, **kw).images)
        assert len(st.recorded) >= 7 and all(p.T == 256 and p.Tm == 128 for p in st.recorded)       # 2 + 5 block calls per model step (the graph leg runs Python twice)
    tome.remove_tome(n_unet)
    assert torch.isfinite(outs[0]).all() and not torch.equal(outs[0], plain)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(pipe("a painting of *s", latents=lat0.clone(), use_graph=False, **kw).images, plain)      # off means off
