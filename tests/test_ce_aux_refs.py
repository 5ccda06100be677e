"""z-loss and final-logit soft-capping on the CPU: the fp64 reference of ``_ce_aux_refs`` against fp64 autograd, the
calibration of its budgets, the ops' torch path against autograd of the formula, and the configuration, model,
generation, parallel and Trainer plumbing."""
import copy
import math
import os
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import _ce_aux_refs as A
import _streaming_refs as R

F64 = torch.float64


def _formula(x, t, z, c, reduction="mean"):
    """F.cross_entropy(c tanh(x / c)) + z logsumexp^2 over the valid rows, in x's dtype."""
    y = c * torch.tanh(x / c) if c else x
    valid = (t != R.IGNORE).to(x.dtype)
    rows = F.cross_entropy(y, t, ignore_index=R.IGNORE, reduction="none") + z * torch.logsumexp(y, -1) ** 2 * valid
    return rows if reduction == "none" else rows.sum() / valid.sum().clamp_min(1)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", A.cases(), ids=A.case_id)
def test_reference_matches_fp64_autograd(case):
    z, c, V = case
    inp = R.ce_inputs(V)
    x = inp["logits"].to(F64).requires_grad_()
    rows = _formula(x, inp["targets"], z, c, "none")
    n_valid = int((inp["targets"] != R.IGNORE).sum())
    (rows.sum() / n_valid).backward()
    ref = A.ce_aux_ref(inp["logits"], inp["targets"], z, c)
    y = c * torch.tanh(x.detach() / c) if c else x.detach()
    lse = torch.logsumexp(y, -1) * (inp["targets"] != R.IGNORE)
    # two fp64 evaluations: 2^-40 relative to the row's scale is far below every fp32 unit
    assert torch.allclose(ref["loss"][0], rows.detach(), rtol=1e-12, atol=1e-11)
    assert torch.allclose(ref["lse"][0], lse, rtol=1e-12, atol=1e-11)
    assert torch.allclose(ref["dlogits"][0], x.grad, rtol=1e-11, atol=1e-14)
    assert ref["loss"][0][-1] == 0 and ref["lse"][0][-1] == 0 and not ref["dlogits"][0][-1].any()  # the ignored row
    for k in ref:
        assert (ref[k][1] >= 0).all() and torch.isfinite(ref[k][1]).all() and torch.isfinite(ref[k][0]).all()
    # the project's torch path (CPU, fp16 / fp32, PLLM_TORCH_OPS=ce) is the same function in fp32
    from pretraining_llm_amd.ops import reference as ops_ref
    got = ops_ref.cross_entropy(inp["logits"], inp["targets"], R.IGNORE, z, c or None)
    want = float(rows.detach().sum() / n_valid)
    assert got.dtype == torch.float32 and abs(float(got) - want) < 1e-5 * abs(want), (float(got), want)


def test_minus_inf_under_a_cap_is_minus_cap():
    """Row 4 of the inputs holds -inf entries: under a cap they are y = -c, take part in the softmax and get a
    zero gradient (1 - tanh^2 = 0); without a cap their probability and gradient are 0 as before."""
    inp = R.ce_inputs(4104)
    masked = torch.isinf(inp["logits"][4])
    assert masked.any()
    capped = A.ce_aux_ref(inp["logits"], inp["targets"], 0.0, 2.0)
    x = inp["logits"][4].to(F64)
    y = 2.0 * torch.tanh(x / 2.0)
    assert (y[masked] == -2.0).all()
    assert abs(float(capped["lse"][0][4]) - float(torch.logsumexp(y, -1))) < 1e-12
    assert not capped["dlogits"][0][4][masked].any()
    from pretraining_llm_amd import ops
    assert (ops.softcap(inp["logits"][4].float(), 2.0)[masked] == -2.0).all()  # the tensors handed out agree
    plain = A.ce_aux_ref(inp["logits"], inp["targets"], 0.0, 0.0)
    old = R.ce_ref(inp["logits"], inp["targets"])
    assert torch.equal(plain["loss"][0], old["loss"][0]) and torch.equal(plain["dlogits"][0], old["dlogits"][0])


def test_budgets_are_calibrated():
    """The fp32 model passes every case at ``measured`` and fails one at ``measured - 1``; budget = 2 measured."""
    need = {}
    for z, c, V in A.cases():
        inp = R.ce_inputs(V)
        items = A.checks(inp, A.ce_aux_model_f32(inp["logits"], inp["targets"], z, c), z, c)
        for op, n in A.needed(items).items():
            need[op] = max(need.get(op, 0), n)
        A.check_all(items, budget={op: A.BUDGET[op][0] for op in A.BUDGET})
    print("calibration (op: needed by the fp32 model):", need)
    for op, (measured, budget) in A.BUDGET.items():
        assert need[op] == measured, f"{op}: the table says {measured}, the fp32 model needs {need[op]}"
        assert budget == 2 * measured


# ------------------------------------------------------------------------------------------------ ops, torch path
@pytest.mark.parametrize("z,c", [(0.5, None), (0.0, 2.0), (0.5, 2.0), (1e-4, 30.0)])
def test_ops_match_autograd_of_the_formula(z, c):
    from pretraining_llm_amd import ops
    torch.manual_seed(0)
    N, C, V = 12, 16, 40
    h = torch.randn(N, C).requires_grad_()
    w = torch.randn(V, C).requires_grad_()
    b = torch.randn(V).requires_grad_()
    t = torch.randint(0, V, (N,))
    t[3] = R.IGNORE
    zt = torch.full((1,), math.nan)
    la = ops.lm_head_cross_entropy(h, w, b, t, z_loss=z, softcap=c, z_out=zt)
    ga = torch.autograd.grad(la, (h, w, b))
    h64, w64, b64 = (v.detach().to(F64).requires_grad_() for v in (h, w, b))
    logits = F.linear(h64, w64, b64)
    lb = _formula(logits, t, z, c or 0.0)
    gb = torch.autograd.grad(lb, (h64, w64, b64))
    assert la.dtype == torch.float32 and abs(float(la.detach()) - float(lb.detach())) < 1e-5 * abs(float(lb.detach()))
    for a, bb in zip(ga, gb):
        assert torch.allclose(a.to(F64), bb, rtol=1e-4, atol=1e-5 * float(bb.abs().max()))
    lc = ops.cross_entropy(logits.detach().float(), t, z_loss=z, softcap=c)  # fp32 whole-logits path
    lb = lb.detach()
    assert abs(float(lc) - float(lb)) < 1e-5 * max(1.0, abs(float(lb)))
    if z:  # the z term alone: total minus the plain CE of the capped logits
        plain = _formula(logits.detach(), t, 0.0, c or 0.0)
        assert abs(float(zt) - (float(lb) - float(plain))) < 1e-5 * float(lb)
    else:
        assert math.isnan(float(zt))  # untouched
    y = ops.softcap(logits.detach().float(), c)
    if c is None:
        assert y.data_ptr() == logits.detach().float().data_ptr() or torch.equal(y, logits.detach().float())
    else:
        assert torch.allclose(y, (c * torch.tanh(logits.detach() / c)).float(), atol=1e-6)
        assert torch.equal(y.argmax(-1), logits.argmax(-1))  # monotone: greedy decoding unchanged


def test_ops_reject_bad_options():
    from pretraining_llm_amd import ops
    x, t = torch.randn(4, 8), torch.zeros(4, dtype=torch.long)
    with pytest.raises(ValueError, match="z_loss"):
        ops.cross_entropy(x, t, z_loss=-1.0)
    with pytest.raises(ValueError, match="softcap"):
        ops.cross_entropy(x, t, softcap=0.0)
    with pytest.raises(ValueError, match="softcap"):
        ops.lm_head_cross_entropy(torch.randn(4, 8), torch.randn(8, 8), None, t, softcap=-2.0)


# ------------------------------------------------------------------------------------------------ configuration
def test_config_validation_presets_and_round_trip():
    from config.config import default_config
    from pretraining_llm_amd.models import ModelConfig, get_preset
    from pretraining_llm_amd.train.trainer import model_config_from
    assert ModelConfig().z_loss == 0.0 and ModelConfig().final_logit_softcap is None
    with pytest.raises(ValueError, match="z_loss"):
        ModelConfig(z_loss=-1e-4)
    for bad in (0.0, -30.0):
        with pytest.raises(ValueError, match="final_logit_softcap"):
            ModelConfig(final_logit_softcap=bad)
    tiny, big = get_preset("llama-tiny-zloss"), get_preset("llama-1.3b-zloss")
    assert (tiny.z_loss, tiny.final_logit_softcap, tiny.qk_norm) == (1e-4, 30.0, True)
    assert (big.z_loss, big.final_logit_softcap, big.qk_norm) == (1e-4, None, True)
    # no parameters, no FLOPs
    assert tiny.num_params() == get_preset("llama-tiny-qknorm").num_params()
    assert tiny.flops_per_token() == get_preset("llama-tiny-qknorm").flops_per_token()
    assert ModelConfig.from_dict(tiny.to_dict()) == tiny
    # a config dict written before the options existed
    old = {k: v for k, v in tiny.to_dict().items() if k not in ("z_loss", "final_logit_softcap")}
    loaded = ModelConfig.from_dict(old)
    assert loaded.z_loss == 0.0 and loaded.final_logit_softcap is None
    # the training config: None -> the preset's, a value overrides
    assert "z_loss" in default_config and "final_logit_softcap" in default_config
    assert default_config["z_loss"] is None and default_config["final_logit_softcap"] is None
    cfg = dict(default_config)
    cfg.update(model_preset="llama-tiny-zloss")
    mc = model_config_from(cfg)
    assert (mc.z_loss, mc.final_logit_softcap) == (1e-4, 30.0)
    cfg.update(z_loss=1e-3, final_logit_softcap=50.0)
    mc = model_config_from(cfg)
    assert (mc.z_loss, mc.final_logit_softcap) == (1e-3, 50.0)
    cfg = dict(default_config)
    cfg.update(model_preset="llama-tiny")
    assert model_config_from(cfg).z_loss == 0.0 and model_config_from(cfg).final_logit_softcap is None


def test_checkpoint_round_trip_and_old_checkpoint(tmp_path):
    from pretraining_llm_amd.models import GPT, ModelConfig, get_preset
    cfg = get_preset("llama-tiny-zloss").replace(vocab_size=64, context_length=16)
    m = GPT(cfg)
    assert not any("z_term" in k for k in m.state_dict())
    assert set(m.state_dict()) == set(GPT(cfg.replace(z_loss=0.0, final_logit_softcap=None)).state_dict())
    path = tmp_path / "m.pt"
    torch.save({"model": m.state_dict(), "config": cfg.to_dict()}, path)
    ck = torch.load(path, weights_only=True)
    cfg2 = ModelConfig.from_dict(ck["config"])
    assert cfg2 == cfg
    GPT(cfg2).load_state_dict(ck["model"])
    old = {k: v for k, v in ck["config"].items() if k not in ("z_loss", "final_logit_softcap")}
    cfg3 = ModelConfig.from_dict(old)
    assert cfg3.z_loss == 0.0 and cfg3.final_logit_softcap is None
    GPT(cfg3).load_state_dict(ck["model"])


# ------------------------------------------------------------------------------------------------ model
def _tiny(**kw):
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(0)
    cfg = get_preset("llama-tiny-zloss").replace(vocab_size=64, context_length=32, **kw)
    m = GPT(cfg)
    with torch.no_grad():  # logits large enough for the cap and the z term to matter
        m.lm_head.weight.mul_(40.0)
    return cfg, m


def test_forward_eval_is_plain_ce_and_train_adds_the_z_term():
    cfg, m = _tiny(z_loss=0.05, final_logit_softcap=5.0)
    x, y = torch.randint(0, 64, (2, 32)), torch.randint(0, 64, (2, 32))
    m.eval()
    with torch.no_grad():
        raw = m(x)[0]  # handed out capped
        assert raw.abs().max() <= 5.0
        h = m._trunk(x)
        uncapped = F.linear(h, m.lm_head.weight)
        assert uncapped.abs().max() > 5.0
        assert torch.allclose(raw, 5.0 * torch.tanh(uncapped / 5.0), atol=1e-6)
        ce = F.cross_entropy(raw.reshape(-1, 64), y.reshape(-1))
        lg_e, le = m(x, y)
        le2 = m(x, y, return_logits=False)[1]
        assert torch.allclose(lg_e, raw, atol=1e-6)
    assert abs(float(le) - float(ce)) < 1e-5 and abs(float(le2) - float(ce)) < 1e-5
    assert m.z_term is None  # eval never wrote it
    m.train()
    zterm = 0.05 * torch.logsumexp(raw.reshape(-1, 64), -1).square().mean()
    lg_t, lt = m(x, y)
    assert abs(float(lt) - float(ce + zterm)) < 1e-5
    assert abs(float(m.z_term) - float(zterm)) < 1e-5 and m.z_term.dtype == torch.float32
    buf = m.z_term
    m.z_term.zero_()
    lt2 = m(x, y, return_logits=False)[1]
    assert m.z_term is buf and abs(float(m.z_term) - float(zterm)) < 1e-5  # written in place
    assert abs(float(lt2) - float(lt)) < 1e-5
    assert torch.allclose(lg_t, raw, atol=1e-6)
    # gradients flow through both terms
    lt2.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_kv_cache_generation_matches_recompute_with_cap():
    cfg, m = _tiny(final_logit_softcap=5.0)
    m.eval()
    idx = torch.randint(0, 64, (2, 6))
    a = m.generate(idx, 10, temperature=0.0, use_cache=True)
    b = m.generate(idx, 10, temperature=0.0, use_cache=False)
    assert torch.equal(a, b)
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached
    cache = KVCache(cfg.n_blocks, 2, 32, cfg.n_kv_head, cfg.head_dim, torch.float32, "cpu")
    with torch.no_grad():
        lg = forward_cached(m, idx, cache, 0)
        full = m(idx)[0][:, -1]
    assert lg.abs().max() <= 5.0 and torch.allclose(lg, full, atol=1e-5)
    # greedy decoding is what it is without the cap (tanh is monotone)
    m2 = copy.deepcopy(m)
    m2.config = cfg.replace(final_logit_softcap=None)
    assert torch.equal(m2.generate(idx, 10, temperature=0.0), a)


# ------------------------------------------------------------------------------------------------ TP + SP
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_cfg():
    # llama-tiny-zloss with a z term large enough to show in the gradients; QK-norm off: the tensor-parallel
    # layout refuses it (parallel/model_parallel.py), which is not this feature's business
    from pretraining_llm_amd.models import get_preset
    return get_preset("llama-tiny-zloss").replace(vocab_size=256, context_length=32, n_embed=64, n_head=4, n_kv_head=2,
                                                  ffn_hidden=96, qk_norm=False, z_loss=1e-2, final_logit_softcap=3.0)


def _tp_batch():
    g = torch.Generator().manual_seed(7)
    data = torch.randint(0, 256, (2, 33), generator=g)
    return data[:, :-1], data[:, 1:]


def _tp_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pretraining_llm_amd.models import GPT
    from pretraining_llm_amd.parallel.dp import DataParallelEngine
    from pretraining_llm_amd.parallel.model_parallel import (gather_dense_state, init_parallel_groups,
                                                             parallelize_gpt, sync_replicated_grads)
    from pretraining_llm_amd.train.optim import FlatAdamW
    cfg = _tp_cfg()
    torch.manual_seed(0)
    model = GPT(cfg)
    pg = init_parallel_groups(2, 1, True, "ring")
    parallelize_gpt(model, pg)
    opt = FlatAdamW(model, lr=1e-2)
    eng = DataParallelEngine(opt, process_group=pg.grad_group, bucket_mb=0.05, first_bucket_mb=0.01)
    opt.set_tensor_parallel(pg.tp_group, 2)
    x, y = _tp_batch()
    _, loss = model(x, y, return_logits=False)
    loss.backward()
    scale = eng.finish_grad_sync()
    sync_replicated_grads(opt, pg)
    scale /= 2
    grads = {id(p): opt.grad_view(i).view(p.shape) * scale for i, p in enumerate(opt.params)}
    gd = gather_dense_state(model, GPT(cfg), pg, grads)
    out = {"grads": {n: p.detach().clone() for n, p in gd.named_parameters()}}
    lt = torch.stack([loss.detach(), model.z_term[0]]).clone()
    dist.all_reduce(lt)
    out["loss"], out["z"] = float(lt[0]) / world, float(lt[1]) / world
    if rank == 0:
        torch.save(out, os.path.join(outdir, "out.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_tp_sp_step_matches_dense():
    """As tests/test_model_parallel.py::test_model_parallel_step_matches_dense (case tp2_sp_llama, its tolerances):
    the LM head is replicated and the loss a per-token mean, so the sharded step needs nothing new."""
    from pretraining_llm_amd.models import GPT
    from pretraining_llm_amd.train.optim import FlatAdamW
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_tp_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        got = torch.load(os.path.join(d, "out.pt"), weights_only=True)
    cfg = _tp_cfg()
    torch.manual_seed(0)
    model = GPT(cfg)
    opt = FlatAdamW(model, lr=1e-2)
    x, y = _tp_batch()
    _, loss = model(x, y, return_logits=False)
    loss.backward()
    assert abs(got["loss"] - float(loss)) < 1e-5, (got["loss"], float(loss))
    assert float(model.z_term) > 1e-3 and abs(got["z"] - float(model.z_term)) < 1e-5
    for i, (n, p) in enumerate(zip(opt.names, opt.params)):
        g = opt.grad_view(i).view(p.shape)
        assert torch.allclose(got["grads"][n], g, atol=1e-6, rtol=1e-4), (n, (got["grads"][n] - g).abs().max())


# ------------------------------------------------------------------------------------------------ Trainer
def test_trainer_logs_the_z_term(tmp_path):
    from config.config import default_config
    from pretraining_llm_amd.train.trainer import Trainer
    cfg = dict(default_config)
    cfg.update(model_preset="llama-tiny-zloss", t_batch_size=2, seq_len=32, t_train_steps=3, t_lr=1e-3, warmup_steps=1,
               log_interval=1, t_eval_steps=2, t_eval_iters=1, t_out_path=str(tmp_path / "m.pt"), synthetic_data=True,
               synthetic_tokens=20_000, synthetic_dir=str(tmp_path / "syn"), device="cpu", z_loss=1e-2)
    recs = []
    tr = Trainer(cfg, log=lambda *_: None)
    assert tr.mcfg.z_loss == 1e-2 and tr.mcfg.final_logit_softcap == 30.0
    tr.metrics.log = recs.append
    tr.train()
    assert len(recs) == 3
    for r in recs:
        assert math.isfinite(r["z_loss"]) and 0 < r["z_loss"] < r["train_loss"], r
    # validation is plain CE: below ln(V) + a margin, where the z term alone (1e-2 ln(512)^2 = 0.39) would show
    val = [r["val_loss"] for r in recs if math.isfinite(r["val_loss"])]
    assert val
    tr.model.eval()
    x, y = tr.val_loader.next()
    with torch.no_grad():
        plain = float(tr.model(x, y, return_logits=False)[1])
        logits = tr.model(x)[0]
    assert abs(plain - float(F.cross_entropy(logits.reshape(-1, logits.shape[-1]).float(), y.reshape(-1)))) < 1e-4
    # the saved checkpoint carries the options
    from pretraining_llm_amd.models import ModelConfig
    ck = torch.load(tmp_path / "m.pt", weights_only=False)
    saved = ModelConfig.from_dict(ck["model_config"])
    assert saved.z_loss == 1e-2 and saved.final_logit_softcap == 30.0
