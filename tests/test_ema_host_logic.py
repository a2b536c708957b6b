"""CPU: the EMA of the trained weights through the trainer's host logic (E4TTrainer(ema_decay=...)) on the op emulation
of tests/ema_reference.py: the average only observes, follows the float64 recurrence, survives the deferred-region split, micro-batch
accumulation, the state dict and a two-rank (gloo) run; the decay schedule; the command lines' flags and *_ema files."""
import argparse
import os
import socket
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ema_reference import EmaEmuBackend, ema_trajectory, rel_l2
from test_train_step_host_logic import _data, _step, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CPU = torch.device("cpu")
DECAY = 0.9999
TOLF = 2e-5          # the project's fp32-kernel bound (rel-L2)


@pytest.fixture()
def ema_emu():
    from e4t import ops
    old_b, old_act = ops.set_backend(EmaEmuBackend(round_bf16=False)), ops.ACT
    ops.ACT = torch.float32
    yield ops
    ops.set_backend(old_b)
    ops.ACT = old_act


def _trainer(ema_decay=DECAY, lr=1e-3, seed=0):
    from e4t.trainer import E4TTrainer
    _, _, n_unet, n_enc, text = build(seed)
    return E4TTrainer(n_unet, n_enc, text, vae=None, lr=lr, class_token_id=11, empty_prompt_ids=torch.zeros(1, 9, dtype=torch.long), device=CPU,
                      ema_decay=ema_decay)


# ---- the decay schedule ---------------------------------------------------------------------------------------------------------
def test_ema_weight_schedule():
    from e4t.optimization import ema_weight
    f32 = lambda x: float(np.float32(x))
    assert ema_weight(DECAY, 1) == f32(1.0 - 2.0 / 11.0) and ema_weight(DECAY, 2) == f32(1.0 - 3.0 / 12.0) == 0.75
    assert ema_weight(DECAY, 10 ** 6) == f32(1.0 - DECAY)
    ws = [ema_weight(DECAY, t) for t in range(1, 200000, 7)]
    assert all(a >= b for a, b in zip(ws, ws[1:])) and ws[0] > ws[-1]                 # monotone: the average stiffens
    # (1 + t) / (10 + t) >= decay  <=>  t >= (10 d - 1) / (1 - d): from there on the cap binds
    t_cap = int(np.ceil((10 * DECAY - 1) / (1 - DECAY)))
    assert ema_weight(DECAY, t_cap - 2) > f32(1.0 - DECAY) and all(ema_weight(DECAY, t) == f32(1.0 - DECAY) for t in (t_cap, t_cap + 1, 10 * t_cap))
    assert len({ema_weight(DECAY, t) for t in range(1, 6)}) == 5                       # five steps, five weights
    assert float(np.float32(ema_weight(0.3, 5))) == ema_weight(0.3, 5) == f32(0.7)     # an fp32 value, rounded once from the double
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ema_weight(bad, 1)
    with pytest.raises(ValueError):
        ema_weight(DECAY, 0)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------
def test_the_average_only_observes_and_follows_the_recurrence(ema_emu):
    batches = [_data(2, 51 + i) for i in range(5)]
    off, on = _trainer(None), _trainer(DECAY)
    assert off.ema is None and "ema" not in off.state_dict() and set(off.state_dict()) == {"params", "exp_avg", "exp_avg_sq", "step_count", "lr"}
    assert torch.equal(on.ema, on.flat.data) and on.ema.data_ptr() != on.flat.data.data_ptr()
    snaps = [on.flat.data.clone()]
    for d in batches:
        lo, ln = _step(off, d), _step(on, d)
        assert all(torch.equal(a, b) for a, b in zip(lo, ln))
        snaps.append(on.flat.data.clone())
    for a, b in ((off.flat.data, on.flat.data), (off.exp_avg, on.exp_avg), (off.exp_avg_sq, on.exp_avg_sq)):
        assert torch.equal(a, b)
    want = ema_trajectory(snaps, DECAY)
    err = rel_l2(on.ema, want)
    print(f"ema vs float64 trajectory after 5 steps: rel-L2 {err:.3e}")
    assert err <= TOLF
    assert not torch.equal(on.ema, on.flat.data) and not torch.equal(on.ema, snaps[0])
    # a stale weight would show: the trajectory with step 1's weight at every step is elsewhere
    from e4t.optimization import ema_weight
    e = snaps[0].double()
    for p in snaps[1:]:
        e = e - ema_weight(DECAY, 1) * (e - p.double())
    assert rel_l2(on.ema, e) > 100 * TOLF


def test_adamw_in_two_parts_around_a_deferred_region_changes_no_bit_of_the_average(ema_emu):
    class Handle:
        def wait(self):
            pass
    res = []
    for split in (False, True):
        tr = _trainer()
        tr.ema.mul_(0.5)            # (an average away from the parameters: every element's update is visible)
        loss, _, _ = tr.losses(*[_data(2, 31)[k] for k in ("px", "lat", "noise", "t", "ids", "pidx")])
        loss.backward()
        n = tr.flat.numel
        lo, hi = (n // 3) // 64 * 64, (2 * n // 3) // 64 * 64
        before = tr.ema.clone()
        tr.optimizer_step(((lo, hi), [Handle()]) if split else None)
        assert float((tr.ema != before).float().mean()) > 0.9
        res.append((tr.ema.clone(), tr.flat.data.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_micro_batches_move_the_average_once(ema_emu):
    from e4t.optimization import ema_weight
    tr = _trainer()
    start = tr.ema.clone()
    _step(tr, _data(1, 21), sync=False, loss_scale=1 / 3)
    _step(tr, _data(1, 22), sync=False, loss_scale=1 / 3)
    assert torch.equal(tr.ema, start) and tr.step_count == 0
    with pytest.raises(RuntimeError, match="micro-batch"):           # the averaged view does not open over pending gradients
        with tr.ema_weights():
            pass
    _step(tr, _data(1, 23), sync=True, loss_scale=1 / 3)
    assert tr.step_count == 1
    w = ema_weight(DECAY, 1)
    assert torch.equal(tr.ema, start - (start - tr.flat.data) * w)       # ONE application, with step 1's weight (the emulation's fp32 form)


def test_ema_weights_context_swaps_and_restores(ema_emu):
    tr, twin = _trainer(), _trainer()
    for t in (tr, twin):
        _step(t, _data(2, 61))
    raw, avg = tr.flat.data.clone(), tr.ema.clone()
    epoch0 = ema_emu._WEIGHTS_EPOCH
    d = _data(2, 62)
    args = [d[k] for k in ("px", "lat", "noise", "t", "ids", "pidx")]
    with torch.no_grad():
        l_raw = tr.losses(*args)
        with tr.ema_weights():
            assert ema_emu._WEIGHTS_EPOCH == epoch0 + 1
            assert torch.equal(tr.flat.data, avg) and torch.equal(tr.ema, avg)
            l_avg = tr.losses(*args)
            with pytest.raises(RuntimeError, match="ema_weights"):
                _step(tr, d)
            with pytest.raises(RuntimeError, match="already open"):
                with tr.ema_weights():
                    pass
        assert ema_emu._WEIGHTS_EPOCH == epoch0 + 2
    assert torch.equal(tr.flat.data, raw) and torch.equal(tr.ema, avg)
    assert not torch.equal(l_raw[0], l_avg[0])
    # a trainer BUILT from the averaged values computes the same losses
    other = _trainer(None)
    other.flat.data.copy_(avg)
    ema_emu.bump_weights_epoch()
    with torch.no_grad():
        l_other = other.losses(*args)
    assert all(torch.equal(a, b) for a, b in zip(l_avg, l_other))
    # the next step is the untouched twin's, bit for bit
    out, out_twin = _step(tr, d), _step(twin, d)
    assert all(torch.equal(a, b) for a, b in zip(out, out_twin))
    assert torch.equal(tr.flat.data, twin.flat.data) and torch.equal(tr.ema, twin.ema)
    with pytest.raises(RuntimeError, match="no EMA"):
        with _trainer(None).ema_weights():
            pass
    with pytest.raises(ValueError):
        _trainer(1.0)


def test_state_dict_round_trip_and_parent_format(ema_emu, tmp_path):
    batches = [_data(2, 31 + i) for i in range(3)]
    full = _trainer()
    for d in batches:
        _step(full, d)
    tr2 = _trainer()
    for d in batches[:2]:
        _step(tr2, d)
    sd = tr2.state_dict()
    assert set(sd) == {"params", "exp_avg", "exp_avg_sq", "step_count", "lr", "ema", "ema_decay"} and sd["ema_decay"] == DECAY
    torch.save(sd, tmp_path / "state.pt")
    tr3 = _trainer()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr3.load_state_dict(torch.load(tmp_path / "state.pt"))
    assert torch.equal(tr3.ema, tr2.ema)
    _step(tr3, batches[2])
    assert torch.equal(tr3.flat.data, full.flat.data) and torch.equal(tr3.ema, full.ema)
    # a state file of the parent's format (no 'ema'): EMA on starts the average from the loaded parameters, with ONE warning ...
    parent = {k: v for k, v in sd.items() if k not in ("ema", "ema_decay")}
    tr4 = _trainer()
    with pytest.warns(UserWarning, match="no 'ema'") as rec:
        tr4.load_state_dict(parent)
    assert len([r for r in rec if "no 'ema'" in str(r.message)]) == 1
    assert torch.equal(tr4.ema, sd["params"]) and torch.equal(tr4.flat.data, sd["params"]) and tr4.step_count == 2
    # ... and EMA off loads it as before, and ignores an 'ema' key
    for state in (parent, sd):
        tr5 = _trainer(None)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            tr5.load_state_dict(state)
        assert tr5.ema is None and torch.equal(tr5.flat.data, sd["params"]) and "ema" not in tr5.state_dict()
        _step(tr5, batches[2])
        assert torch.equal(tr5.flat.data, full.flat.data)


# ---- two ranks over gloo ----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, out_dir, mode):
    for p in (os.path.join(ROOT, "e4t-diffusion_amd"), ROOT, HERE, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), E4T_REPLICA_CHECK_EVERY="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from e4t import ops
    from test_ddp_gloo import _batch
    ops.set_backend(EmaEmuBackend(round_bf16=False))
    ops.ACT = torch.float32
    tr = _trainer(seed=rank if mode == "seeds" else 0)          # "seeds": rank 1 is constructed from other weights
    step = lambda r: (lambda b: tr.train_step(b["pixels"], b["ids"], b["pidx"], noise=b["noise"], timesteps=b["t"], latents=b["latents"]))(_batch(r))
    msg = "no error"
    if mode == "seeds":
        for i in range(3):
            step(rank + 2 * i)
    elif mode == "resume":
        # every rank reads ITS OWN state file: different parameters, moments and averages
        g = torch.Generator().manual_seed(70 + rank)
        sd = tr.state_dict()
        for k in ("params", "exp_avg", "ema"):
            sd[k] = sd[k] + torch.randn(sd[k].shape, generator=g) * 1e-2
        sd["exp_avg_sq"] = sd["exp_avg_sq"] + torch.rand(sd["exp_avg_sq"].shape, generator=g) * 1e-4
        sd["step_count"] = 7
        torch.save(sd["ema"], os.path.join(out_dir, f"file_ema{rank}.pt"))
        tr.load_state_dict(sd)
        torch.save(tr.ema.clone(), os.path.join(out_dir, f"loaded_ema{rank}.pt"))
        step(rank)
    else:                                                       # "diverge": the averages alone differ
        if rank == 1:
            tr.ema[5] += 1e-3
        try:
            step(rank)
        except RuntimeError as e:
            msg = str(e)
    torch.save(dict(ema=tr.ema.clone(), params=tr.flat.data.clone(), msg=msg), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["seeds", "resume", "diverge"])
def test_two_ranks_keep_one_average(tmp_path, mode):
    """seeds: the average is copied AFTER the start-up broadcast, so ranks built from different seeds hold identical averages after three
    steps (the per-step replica check, which now covers the average, passes).  resume: each rank loads a different state file and ends with
    rank 0's average.  diverge: a difference in the average ALONE makes check_replicas raise on every rank."""
    world = 2
    mp.spawn(_gloo_worker, args=(world, _free_port(), str(tmp_path), mode), nprocs=world, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(world))
    if mode == "diverge":
        assert all("replicas diverged" in r["msg"] for r in (r0, r1))
        assert torch.equal(r0["params"], r1["params"])           # (only the average differed)
        return
    assert r0["msg"] == r1["msg"] == "no error"
    assert torch.equal(r0["ema"], r1["ema"]) and torch.equal(r0["params"], r1["params"])
    assert not torch.equal(r0["ema"], r0["params"])
    if mode == "resume":
        f0, f1 = torch.load(tmp_path / "file_ema0.pt"), torch.load(tmp_path / "file_ema1.pt")
        assert not torch.equal(f0, f1)
        assert all(torch.equal(torch.load(tmp_path / f"loaded_ema{r}.pt"), f0) for r in range(world))


# ---- command lines ------------------------------------------------------------------------------------------------------------
def _parse(module, argv, monkeypatch):
    import importlib
    monkeypatch.setattr(sys, "argv", [f"{module}.py"] + argv)
    return importlib.import_module(module).parse_args()


def test_flags(monkeypatch, capsys):
    a = _parse("pretrain_e4t", ["--synthetic_data"], monkeypatch)
    assert a.use_ema is False and a.ema_decay is None
    a = _parse("pretrain_e4t", ["--synthetic_data", "--use_ema"], monkeypatch)
    assert a.use_ema and a.ema_decay == 0.9999
    assert _parse("pretrain_e4t", ["--use_ema", "--ema_decay", "0.999"], monkeypatch).ema_decay == 0.999
    for bad, msg in ((["--use_ema", "--ema_decay", "1.0"], "(0, 1)"), (["--use_ema", "--ema_decay", "0"], "(0, 1)"),
                     (["--use_ema", "--ema_decay", "-0.5"], "(0, 1)"), (["--ema_decay", "0.999"], "needs --use_ema")):
        with pytest.raises(SystemExit) as ex:
            _parse("pretrain_e4t", bad, monkeypatch)
        assert ex.value.code == 2 and msg in capsys.readouterr().err           # argparse errors
    for module in ("tuning_e4t", "inference"):
        assert _parse(module, ["--use_ema"], monkeypatch).use_ema and not _parse(module, [], monkeypatch).use_ema
        with pytest.raises(SystemExit):
            _parse(module, ["--use_ema", "--ema_decay", "0.999"], monkeypatch)       # tuning and sampling do not average


def test_ema_files_are_written_loaded_and_missed_loudly(ema_emu, tmp_path):
    import json
    import inference
    import tuning_e4t
    from e4t import cli_common as cc
    from e4t.utils import save_config, save_e4t_encoder, save_e4t_unet
    import pretrain_e4t
    from test_cli_setup import pretrain_args, tuning_args
    off = pretrain_e4t.setup(pretrain_args(), CPU)["trainer"]
    assert off.ema is None and off.ema_decay is None                     # no flag, no average
    st = pretrain_e4t.setup(pretrain_args(use_ema=True, ema_decay=0.99, scale_lr=False, learning_rate=1e-3), CPU)
    tr = st["trainer"]
    assert tr.ema_decay == 0.99 and tr.ema is not None
    px, ids, pidx = next(pretrain_e4t.synthetic_batches(pretrain_args(resolution=64), CPU, 0, 1, st["prompts"]))
    tr.train_step(px, ids, pidx, latents=torch.randn(4, 4, 16, 16) * 0.18215)
    d = str(tmp_path / "run")
    save_config(dict(placeholder_token="*s", use_ema=True, ema_decay=0.99, tome_ratio=0.5), d)
    assert json.load(open(os.path.join(d, "config.json"))) == {"placeholder_token": "*s"}          # config.json does not record the EMA
    save_e4t_unet(tr.unet, d)
    save_e4t_encoder(tr.encoder, d)
    for module, args in ((tuning_e4t, tuning_args(pretrained_model_name_or_path=d, use_ema=True)),
                         (inference, argparse.Namespace(pretrained_model_name_or_path=d, use_ema=True, random_init=False, scheduler_type="ddim",
                                                        unet_variant="sd14"))):
        with pytest.raises(SystemExit, match="holds no weight_offsets_ema.pt / encoder_ema.pt"):
            module.setup(args, CPU)
    raw_sd = torch.load(os.path.join(d, "weight_offsets.pt"))
    with tr.ema_weights():
        save_e4t_unet(tr.unet, d, "weight_offsets_ema.pt")
        save_e4t_encoder(tr.encoder, d, "encoder_ema.pt")
    assert sorted(os.listdir(d)) == ["config.json", "encoder.pt", "encoder_ema.pt", "weight_offsets.pt", "weight_offsets_ema.pt"]
    ema_sd = torch.load(os.path.join(d, "weight_offsets_ema.pt"))
    assert ema_sd.keys() == raw_sd.keys() and any(not torch.equal(ema_sd[k], raw_sd[k]) for k in raw_sd)
    assert all(torch.equal(raw_sd[k], v) for k, v in torch.load(os.path.join(d, "weight_offsets.pt")).items())       # the raw file is untouched
    # the averaged files hold the average: they are the flat EMA buffer seen through the parameters' views
    flat_of = {id(p): i for i, p in enumerate(tr.flat.params)}
    checked = 0
    for name, p in list(tr.unet.named_parameters()) + [("enc." + n, q) for n, q in tr.encoder.named_parameters()]:
        if id(p) in flat_of:
            got = (torch.load(os.path.join(d, "encoder_ema.pt"))[name[4:]] if name.startswith("enc.") else ema_sd[name])
            assert torch.equal(got, tr.flat.view(flat_of[id(p)], tr.ema)), name
            checked += 1
    assert checked == len(tr.flat.params)
    # ... and build_models(use_ema=True) loads them, not the raw ones
    unet, enc, _, _ = cc.build_models(CPU, None, "tiny-test", seed=9, e4t_dir=d, use_ema=True)
    name = next(k for k in raw_sd if not torch.equal(ema_sd[k], raw_sd[k]))
    assert torch.equal(dict(unet.named_parameters())[name].detach(), ema_sd[name])
    assert cc.ema_file_names(d, True) == {"weight_offsets.pt": "weight_offsets_ema.pt", "encoder.pt": "encoder_ema.pt"}
    assert cc.ema_file_names(d, False) == {"weight_offsets.pt": "weight_offsets.pt", "encoder.pt": "encoder.pt"}
