"""Attention sinks on the CPU (reference backend): the config key and its validation, the parameter and the state
dict, checkpoints written before the option, the decay exemption, a training step, the sink in local and global
layers, and generation through the cached and the uncached path."""
import math

import pytest
import torch

from pretraining_llm_amd import ops
from pretraining_llm_amd.models import GPT, ModelConfig, get_preset
from pretraining_llm_amd.ops import reference as ref


def _tiny(**kw):
    return get_preset("llama-tiny-sinks").replace(vocab_size=64, context_length=48, **kw)


def _set_sinks(m, seed=0):
    """Sinks away from their zero initialisation, distinct per head and block."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for blk in m.attn_blocks:
            blk.attn.sinks.copy_(1.0 + torch.randn(blk.attn.sinks.shape, generator=g))


def test_config_and_presets():
    cfg = get_preset("llama-tiny-sinks")
    assert cfg.attn_sinks and cfg.to_dict()["attn_sinks"] is True
    assert ModelConfig.from_dict(cfg.to_dict()) == cfg
    assert cfg == get_preset("llama-tiny-swa").replace(attn_sinks=True)
    assert get_preset("llama-1.3b-sinks") == get_preset("llama-1.3b-swa").replace(attn_sinks=True)
    for name in ("llama-tiny", "llama-tiny-swa", "llama-1.3b", "gpt2-small"):
        assert not get_preset(name).attn_sinks
    old = {k: v for k, v in get_preset("llama-tiny").to_dict().items() if k != "attn_sinks"}
    assert not ModelConfig.from_dict(old).attn_sinks  # a config written before the option
    # n_head parameters per block, nothing else; FLOP accounting unchanged
    for c in (cfg, get_preset("llama-1.3b-sinks"), get_preset("gpt2-tiny").replace(attn_sinks=True)):
        plain = c.replace(attn_sinks=False)
        assert c.num_params() - plain.num_params() == c.n_head * c.n_blocks
        assert c.flops_per_token() == plain.flops_per_token() and c.matmul_params() == plain.matmul_params()
    m = GPT(_tiny())
    assert m.num_params() == m.config.num_params()


def test_ref_arch_and_tp_cp_rejected():
    from config.config import default_config
    from pretraining_llm_amd.parallel.model_parallel import parallelize_gpt
    from pretraining_llm_amd.train.trainer import Trainer
    with pytest.raises(ValueError, match="attn_sinks"):
        get_preset("ref-small").replace(attn_sinks=True)
    with pytest.raises(ValueError, match="attn_sinks"):
        ModelConfig(arch="ref", attn_sinks=True)

    class PG:  # what parallelize_gpt reads
        tp, cp, sequence_parallel, cp_mode = 2, 1, False, "ring"
    m = GPT(_tiny(sliding_window=None, sliding_window_pattern=0))  # (the window is rejected there on its own)
    with pytest.raises(ValueError, match="attn_sinks"):
        parallelize_gpt(m, PG)
    PG.tp, PG.cp = 1, 2
    with pytest.raises(ValueError, match="attn_sinks"):
        parallelize_gpt(m, PG)
    assert m.parallel is None and type(m.attn_blocks[0].attn).__name__ == "Attention"
    for kw in (dict(tp_size=2), dict(cp_size=2)):
        cfg = dict(default_config)
        cfg.update(model_preset="llama-tiny", attn_sinks=True, device="cpu", **kw)
        with pytest.raises(ValueError, match="attn_sinks"):  # no process group exists yet: raised before init
            Trainer(cfg, log=lambda *_: None)
        assert not torch.distributed.is_initialized()


def test_config_hand_over_and_cli():
    import importlib.util
    import os
    from config.config import default_config
    from pretraining_llm_amd.train import model_config_from
    cfg = dict(default_config)
    assert "attn_sinks" in cfg and cfg["attn_sinks"] is None
    cfg.update(model_preset="llama-tiny-swa")
    assert not model_config_from(cfg).attn_sinks
    cfg.update(attn_sinks=True)
    assert model_config_from(cfg) == get_preset("llama-tiny-sinks")
    cfg.update(model_preset="llama-tiny-sinks", attn_sinks=None)
    assert model_config_from(cfg).attn_sinks  # None leaves the preset's value
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_transformer.py")
    spec = importlib.util.spec_from_file_location("_train_transformer_sinks", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    c1 = mod.build_config(["--preset=llama-1.3b", "--sliding_window=512", "--sliding_window_pattern=4",
                           "--attn_sinks=True"])
    assert c1["attn_sinks"] is True and model_config_from(c1) == get_preset("llama-1.3b-sinks")
    for name in ("llama-tiny-sinks", "llama-1.3b-sinks"):
        assert model_config_from(mod.build_config([f"--model_preset={name}"])) == get_preset(name)


def test_state_dict_keys_and_old_checkpoints():
    base = get_preset("llama-tiny-swa").replace(vocab_size=64, context_length=48)
    off, on = GPT(base), GPT(base.replace(attn_sinks=True))
    extra = set(on.state_dict()) - set(off.state_dict())
    assert extra == {f"attn_blocks.{i}.attn.sinks" for i in range(base.n_blocks)}
    assert set(off.state_dict()) <= set(on.state_dict()) and not any("sinks" in k for k in off.state_dict())
    blk = {k for k in off.state_dict() if k.startswith("attn_blocks.0.")}  # today's keys, spelled out for one block
    assert blk == {"attn_blocks.0." + s for s in (
        "ln1.weight", "attn.qkv.weight", "attn.proj.weight", "ln2.weight", "mlp.hidden.weight", "mlp.proj.weight")}
    for b in on.attn_blocks:
        s = b.attn.sinks
        assert isinstance(s, torch.nn.Parameter) and s.shape == (base.n_head,) and not s.any() and s.requires_grad
    assert not hasattr(off.attn_blocks[0].attn, "sinks")
    old = {k: v.clone() for k, v in off.state_dict().items()}  # a checkpoint written before the option
    GPT(base).load_state_dict(old)  # loads unchanged with the option off
    with pytest.raises(RuntimeError, match=r"Missing key.*attn_blocks\.0\.attn\.sinks"):
        GPT(base.replace(attn_sinks=True)).load_state_dict(old)
    on.load_state_dict(old, strict=False)  # ... and into the trunk when asked to
    # sinks = 0 is not "no sinks": softmax-off-by-one
    idx = torch.randint(0, 64, (2, 20), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert (on(idx)[0] - off(idx)[0]).abs().max() > 1e-4
    # reset_parameters keeps the zeros (other 1-D parameters are gains and start at 1)
    _set_sinks(on)
    on.reset_parameters()
    assert all(not b.attn.sinks.any() for b in on.attn_blocks) and bool((on.attn_blocks[0].ln1.weight == 1).all())


def test_sinks_take_no_weight_decay():
    from pretraining_llm_amd.train.optim import FlatAdamW, no_decay_1d
    m = GPT(_tiny())
    sinks = [(n, p) for n, p in m.named_parameters() if n.endswith("attn.sinks")]
    assert len(sinks) == 2 and all(p.dim() == 1 for _, p in sinks)
    assert not any(no_decay_1d(n, p) for n, p in sinks)  # the filter returns True for DECAYED parameters
    # in the optimizer: with zero gradients and a large decay the sinks stay, a matrix shrinks
    _set_sinks(m)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = FlatAdamW(m, lr=1e-2, weight_decay=0.5, decay_filter=no_decay_1d)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    after = dict(m.named_parameters())
    for n, _ in sinks:
        assert torch.equal(after[n].detach(), before[n]), n
    w = "attn_blocks.0.attn.qkv.weight"
    assert float(after[w].detach().norm()) < float(before[w].norm())


def test_training_step_changes_the_sinks():
    from pretraining_llm_amd.train.optim import FlatAdamW, no_decay_1d
    torch.manual_seed(0)
    m = GPT(_tiny())
    opt = FlatAdamW(m, lr=1e-2, weight_decay=0.1, decay_filter=no_decay_1d)
    idx = torch.randint(0, 64, (2, 48))
    losses = []
    for _ in range(3):
        _, loss = m(idx, torch.roll(idx, -1, 1))
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    for b in m.attn_blocks:
        assert b.attn.sinks.detach().abs().min() > 0  # AdamW moves every element by about lr per step
    # under activation checkpointing the recompute carries the sink: the same loss and sink gradients
    m.zero_grad()
    _, l1 = m(idx, torch.roll(idx, -1, 1))
    l1.backward()
    g1 = [b.attn.sinks.grad.clone() for b in m.attn_blocks]
    m.zero_grad()
    m.config.activation_checkpointing = True
    m.train()
    _, l2 = m(idx, torch.roll(idx, -1, 1))
    l2.backward()
    assert l1.item() == l2.item()
    for a, b in zip(g1, m.attn_blocks):
        assert torch.allclose(a, b.attn.sinks.grad, rtol=1e-5, atol=1e-8)


def test_sink_is_present_in_local_and_global_layers():
    """llama-tiny-sinks alternates a local (W = 32) and a global layer.  Moving one layer's sinks moves the logits,
    in either layer; a very negative sink is no sink (the model without the option); and in the local layer a row far
    past the window still has the sink in its denominator: its attention output is that of the windowed softmax
    scaled by 1 - p_sink."""
    torch.manual_seed(2)
    cfg = _tiny()
    assert cfg.layer_window(0) == 32 and cfg.layer_window(1) is None
    m = GPT(cfg).eval()
    idx = torch.randint(0, 64, (2, 48))
    with torch.no_grad():
        base = m(idx)[0]
        for layer in (0, 1):
            m.attn_blocks[layer].attn.sinks.fill_(3.0)
            assert (m(idx)[0] - base).abs().max() > 1e-3, layer
            m.attn_blocks[layer].attn.sinks.zero_()
        off = GPT(cfg.replace(attn_sinks=False)).eval()
        off.load_state_dict({k: v for k, v in m.state_dict().items() if not k.endswith("attn.sinks")})
        for b in m.attn_blocks:
            b.attn.sinks.fill_(-1e4)
        assert torch.allclose(m(idx)[0], off(idx)[0], atol=1e-6)
    # the op: a window of 8 over 40 positions, sinks per head
    g = torch.Generator().manual_seed(3)
    B, T, H, Hkv, D = 2, 40, 4, 2, 16
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, generator=g)
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0])
    bounds = ops.window_bounds(B, T, 8, "cpu")
    o_s = ops.attention_packed(qkv, H, Hkv, bounds=bounds, sinks=sinks).view(B, T, H, D)
    o_p = ops.attention_packed(qkv, H, Hkv, bounds=bounds).view(B, T, H, D)
    q, k, v = ops._split_qkv(qkv, H, Hkv, D)
    lse_p = ref.attention(q, k, v, causal=True, bounds=bounds)[1]                       # [B, H, T]
    p_sink = torch.sigmoid(sinks.view(1, H, 1) - lse_p)                                # e^s / (e^s + Z)
    assert torch.allclose(o_s, o_p * (1 - p_sink).transpose(1, 2).unsqueeze(-1), atol=1e-5)
    assert float(p_sink[..., -1].min()) > 0.01  # the last row, 32 positions past its window's start
    # under doc_mask a row that sees only itself attends to itself and the sink
    one = (torch.arange(T, dtype=torch.int32).expand(B, T).contiguous(),) * 2  # every token its own document
    o_1 = ops.attention_packed(qkv, H, Hkv, bounds=one, sinks=sinks).view(B, T, H, D)
    s_self = (q * k.repeat_interleave(H // Hkv, 2)).sum(-1) / math.sqrt(D)            # [B, T, H]
    w_self = torch.sigmoid(s_self - sinks.view(1, 1, H))
    assert torch.allclose(o_1, w_self.unsqueeze(-1) * v.repeat_interleave(H // Hkv, 2), atol=1e-5)


def test_ops_paths_carry_the_sink_on_the_cpu():
    """ops.attention (prefill, one-token and kv_start forms) and ops.attention_decode (host, scalar and per-row
    counts, window) against the packed op's rows."""
    g = torch.Generator().manual_seed(4)
    B, T, H, Hkv, D = 2, 24, 4, 2, 16
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, generator=g)
    sinks = torch.tensor([1.0, -0.5, 0.0, 2.0])
    q, k, v = ops._split_qkv(qkv, H, Hkv, D)
    full = ops.attention_packed(qkv, H, Hkv, sinks=sinks).view(B, T, H, D)
    assert torch.allclose(ops.attention(q, k, v, sinks=sinks), full, atol=1e-6)
    last = ops.attention(q[:, -1:], k, v, sinks=sinks)
    assert torch.allclose(last, full[:, -1:], atol=1e-6)
    assert torch.allclose(ops.attention_decode(q[:, -1:], k, v, sinks=sinks), full[:, -1:], atol=1e-6)
    n = torch.tensor([T], dtype=torch.int32)
    assert torch.allclose(ops.attention_decode(q[:, -1:], k, v, seqlen=n, sinks=sinks), full[:, -1:], atol=1e-6)
    rows = ops.attention_decode(torch.stack([q[0, 9], q[1, 23]])[:, None], k, v,
                                seqlen=torch.tensor([10, 24], dtype=torch.int32), sinks=sinks)
    assert torch.allclose(rows[:, 0], torch.stack([full[0, 9], full[1, 23]]), atol=1e-6)
    W = 8
    win = ops.attention_packed(qkv, H, Hkv, bounds=ops.window_bounds(B, T, W, "cpu"), sinks=sinks).view(B, T, H, D)
    assert torch.allclose(ops.attention_decode(q[:, -1:], k, v, seqlen=n, window=W, sinks=sinks), win[:, -1:],
                          atol=1e-6)
    assert torch.allclose(ops.attention(q, k, v, kv_start=ops.window_bounds(B, T, W, "cpu")[0], sinks=sinks), win,
                          atol=1e-6)
    empty = ops.attention_decode(q[:, -1:], k, v, seqlen=torch.tensor([0, 3], dtype=torch.int32), sinks=sinks)
    assert not empty[0].any() and empty[1].any()  # a count of 0: the sink takes the row, o = 0
    # sinks of -inf: the plain op
    off = torch.full((H,), -math.inf)
    assert torch.equal(ops.attention_packed(qkv, H, Hkv, sinks=off), ops.attention_packed(qkv, H, Hkv))


@pytest.mark.parametrize("T0", [5, 40])
def test_generation_cached_matches_uncached(T0):
    """Greedy tokens through the KV cache (prefill + one-token steps; the prompt of 40 is past the local layer's
    window of 32, so the prefill takes kv_start and the steps the cache's last 32 rows) and by full recompute."""
    torch.manual_seed(3)
    cfg = get_preset("llama-tiny-sinks").replace(vocab_size=256, context_length=64)
    m = GPT(cfg).eval()
    _set_sinks(m, 1)
    idx = torch.randint(0, 256, (2, T0))
    a = m.generate(idx, 20, temperature=0.0, use_cache=True)
    b = m.generate(idx, 20, temperature=0.0, use_cache=False)
    assert a.shape == (2, T0 + 20) and torch.equal(a, b)
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached
    cache = KVCache(cfg.n_blocks, 2, 64, cfg.n_kv_head, cfg.head_dim, torch.float32, "cpu")
    with torch.no_grad():
        forward_cached(m, idx, cache, 0)
        step = forward_cached(m, a[:, T0:T0 + 1], cache, T0)
        full = m(a[:, :T0 + 1])[0][:, -1]
    assert torch.allclose(step.reshape(full.shape), full, atol=1e-4)
