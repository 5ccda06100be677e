"""QK-norm on the CPU: configuration, parameters and state dict, the parallelism guard, the stand-alone op's
gradients, KV-cache generation and activation checkpointing (the reference path the GPU tests compare against)."""
import pytest
import torch

from pretraining_llm_amd import ops
from pretraining_llm_amd.models import GPT, ModelConfig, get_preset
from pretraining_llm_amd.ops import reference as ref

QKN_PRESETS = ["llama-tiny-qknorm", "gpt2-tiny+qk_norm"]


def _cfg(name, **kw):
    if name.endswith("+qk_norm"):
        return get_preset(name[: -len("+qk_norm")]).replace(qk_norm=True, **kw)
    return get_preset(name).replace(**kw) if kw else get_preset(name)


def test_config_round_trip_and_presets():
    cfg = get_preset("llama-tiny-qknorm").replace(qk_norm_eps=3e-6)
    assert cfg.qk_norm and cfg.qk_norm_eps == 3e-6
    d = cfg.to_dict()
    assert d["qk_norm"] is True and d["qk_norm_eps"] == 3e-6
    assert ModelConfig.from_dict(d) == cfg
    old = {k: v for k, v in get_preset("llama-tiny").to_dict().items() if not k.startswith("qk_norm")}
    assert ModelConfig.from_dict(old) == get_preset("llama-tiny")  # a checkpoint from before the keys existed
    assert not get_preset("llama-tiny").qk_norm and not get_preset("llama-1.3b").qk_norm
    assert get_preset("llama-tiny-qknorm") == get_preset("llama-tiny").replace(qk_norm=True)
    assert get_preset("llama-1.3b-qknorm") == get_preset("llama-1.3b").replace(qk_norm=True)


def test_checkpoint_config_round_trip(tmp_path):
    """What generate_text.py / serve.py do: rebuild the model from the checkpoint's model_config."""
    from pretraining_llm_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    torch.manual_seed(0)
    m = GPT(_cfg("llama-tiny-qknorm", vocab_size=64, context_length=16))
    with torch.no_grad():
        m.attn_blocks[1].attn.k_norm.weight.mul_(1.5)
    path = str(tmp_path / "m.pt")
    save_checkpoint(path, m)
    ckpt = load_checkpoint(path)
    cfg = ModelConfig.from_dict(ckpt["model_config"])
    assert cfg.qk_norm and cfg == m.config
    m2 = GPT(cfg)
    m2.load_state_dict(ckpt["model_state_dict"])
    assert torch.equal(m2.attn_blocks[1].attn.k_norm.weight, m.attn_blocks[1].attn.k_norm.weight)


@pytest.mark.parametrize("name", QKN_PRESETS + ["llama-tiny", "gpt2-tiny"])
def test_num_params_formula(name):
    cfg = _cfg(name, vocab_size=512, context_length=64)
    m = GPT(cfg)
    assert sum(p.numel() for p in m.parameters()) == cfg.num_params()
    plain = cfg.replace(qk_norm=False)
    assert cfg.num_params() - plain.num_params() == (2 * cfg.head_dim * cfg.n_blocks if cfg.qk_norm else 0)


def test_state_dict_keys_only_with_qk_norm():
    base = get_preset("llama-tiny").replace(vocab_size=64, context_length=16)
    off, on = GPT(base), GPT(base.replace(qk_norm=True))
    extra = set(on.state_dict()) - set(off.state_dict())
    assert extra == {f"attn_blocks.{i}.attn.{w}_norm.weight" for i in range(base.n_blocks) for w in "qk"}
    assert set(off.state_dict()) <= set(on.state_dict())
    assert not any("q_norm" in k or "k_norm" in k for k in off.state_dict())
    # today's keys, spelled out for one block
    blk = {k for k in off.state_dict() if k.startswith("attn_blocks.0.")}
    assert blk == {"attn_blocks.0." + s for s in (
        "ln1.weight", "attn.qkv.weight", "attn.proj.weight", "ln2.weight", "mlp.hidden.weight", "mlp.proj.weight")}
    for i in range(base.n_blocks):
        a = on.attn_blocks[i].attn
        assert torch.equal(a.q_norm.weight, torch.ones(base.head_dim)) and a.k_norm.weight.shape == (base.head_dim,)
    on.load_state_dict(off.state_dict(), strict=False)  # an older checkpoint loads into the trunk
    off.load_state_dict({k: v for k, v in on.state_dict().items() if k not in extra})


def test_ref_arch_rejected():
    with pytest.raises(ValueError, match="qk_norm"):
        get_preset("ref-small").replace(qk_norm=True)
    with pytest.raises(ValueError, match="qk_norm"):
        ModelConfig(arch="ref", qk_norm=True)


def test_gains_take_no_weight_decay():
    from pretraining_llm_amd.train.optim import no_decay_1d
    m = GPT(_cfg("llama-tiny-qknorm", vocab_size=64, context_length=16))
    gains = [(n, p) for n, p in m.named_parameters() if "q_norm" in n or "k_norm" in n]
    assert len(gains) == 4
    assert not any(no_decay_1d(n, p) for n, p in gains)  # the filter returns True for DECAYED parameters


def test_tp_cp_rejected_before_any_collective():
    from config.config import default_config
    from pretraining_llm_amd.parallel.model_parallel import parallelize_gpt
    from pretraining_llm_amd.train.trainer import Trainer

    class PG:  # what parallelize_gpt reads
        tp, cp, sequence_parallel, cp_mode = 2, 1, False, "ring"
    m = GPT(_cfg("llama-tiny-qknorm", vocab_size=64, context_length=16))
    with pytest.raises(ValueError, match="qk_norm"):
        parallelize_gpt(m, PG)
    PG.tp, PG.cp = 1, 2
    with pytest.raises(ValueError, match="qk_norm"):
        parallelize_gpt(m, PG)
    assert m.parallel is None and type(m.attn_blocks[0].attn).__name__ == "Attention"  # nothing was sharded
    for kw in (dict(tp_size=2), dict(cp_size=2)):
        cfg = dict(default_config)
        cfg.update(model_preset="llama-tiny-qknorm", device="cpu", **kw)
        with pytest.raises(ValueError, match="qk_norm"):  # no process group exists yet: raised before init
            Trainer(cfg, log=lambda *_: None)
        assert not torch.distributed.is_initialized()


def test_model_config_from_forwards_keys():
    from config.config import default_config
    from pretraining_llm_amd.train import model_config_from
    cfg = dict(default_config)
    cfg.update(model_preset="llama-tiny")
    assert not model_config_from(cfg).qk_norm
    cfg.update(qk_norm=True, qk_norm_eps=1e-6)
    mc = model_config_from(cfg)
    assert mc.qk_norm and mc.qk_norm_eps == 1e-6 and mc == get_preset("llama-tiny").replace(qk_norm=True,
                                                                                           qk_norm_eps=1e-6)
    cfg.update(model_preset="llama-tiny-qknorm", qk_norm=None, qk_norm_eps=None)
    assert model_config_from(cfg).qk_norm  # None leaves the preset's value


def test_train_script_accepts_qk_norm_flag():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_transformer.py")
    spec = importlib.util.spec_from_file_location("_train_transformer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pretraining_llm_amd.train import model_config_from
    cfg = mod.build_config(["--preset=llama-1.3b", "--qk_norm=True"])
    assert cfg["qk_norm"] is True and model_config_from(cfg) == get_preset("llama-1.3b-qknorm")


@pytest.mark.parametrize("rope", [False, True])
def test_qk_norm_packed_gradients_match_autograd(rope):
    torch.manual_seed(1)
    B, T, H, Hkv, D, pos = 2, 7, 4, 2, 16, 3
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, dtype=torch.float64, requires_grad=True)
    wq = (1 + 0.3 * torch.randn(D, dtype=torch.float64)).requires_grad_()
    wk = (1 + 0.3 * torch.randn(D, dtype=torch.float64)).requires_grad_()
    cos, sin = ref.rope_cos_sin(T + pos, D) if rope else (None, None)
    q, k = ops.qk_norm_packed(qkv.float(), wq.float(), wk.float(), 1e-5, H, Hkv, cos, sin, pos)
    assert q.shape == (B, T, H, D) and k.shape == (B, T, Hkv, D)
    dq, dk = torch.randn_like(q), torch.randn_like(k)
    # the op against plain autograd through ref.qk_norm (and ref.rope) on the split heads
    x32 = qkv.detach().float().requires_grad_()
    wq32, wk32 = wq.detach().float().requires_grad_(), wk.detach().float().requires_grad_()
    q1, k1 = ops.qk_norm_packed(x32, wq32, wk32, 1e-5, H, Hkv, cos, sin, pos)
    torch.autograd.backward([q1, k1], [dq, dk])
    y32 = qkv.detach().float().requires_grad_()
    vq32, vk32 = wq.detach().float().requires_grad_(), wk.detach().float().requires_grad_()
    q0, k0, _ = ops._split_qkv(y32, H, Hkv, D)
    q2, k2 = ref.qk_norm(q0, vq32, 1e-5), ref.qk_norm(k0, vk32, 1e-5)
    if rope:
        q2, k2 = ref.rope(q2, cos[pos:pos + T], sin[pos:pos + T]), ref.rope(k2, cos[pos:pos + T], sin[pos:pos + T])
    torch.autograd.backward([q2, k2], [dq, dk])
    assert torch.allclose(q1, q2, atol=1e-6) and torch.allclose(k1, k2, atol=1e-6)
    for a, b in ((x32.grad, y32.grad), (wq32.grad, vq32.grad), (wk32.grad, vk32.grad)):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)
    assert not x32.grad[..., (H + Hkv) * D:].any()
    # and against the closed form: x_hat = x r, dx = r (g - x_hat mean(g x_hat)) for one un-rotated head
    if not rope:
        x = qkv.detach()[0, 0, :D]
        r = (x.pow(2).mean() + 1e-5).rsqrt()
        g = dq[0, 0, 0].double() * wq.detach()
        dx = r * (g - x * r * (g * x * r).mean())
        assert torch.allclose(x32.grad[0, 0, :D].double(), dx, atol=1e-5)


@pytest.mark.parametrize("name", QKN_PRESETS)
def test_kv_cache_generation_matches_recompute(name):
    """tests/test_models.py::test_kv_cache_generation_matches_recompute with QK-norm."""
    torch.manual_seed(3)
    cfg = _cfg(name, vocab_size=256, context_length=32)
    m = GPT(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                p.add_(0.3 * torch.randn_like(p))
    idx = torch.randint(0, 256, (2, 5))
    a = m.generate(idx, 20, temperature=0.0, use_cache=True)
    b = m.generate(idx, 20, temperature=0.0, use_cache=False)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", QKN_PRESETS)
def test_device_position_decode_step_matches_cached(name):
    """tests/test_models.py::test_device_position_decode_step_matches_cached with QK-norm, and with one position
    per sequence (the continuous server's form)."""
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached, forward_decode
    torch.manual_seed(6)
    cfg = _cfg(name, vocab_size=256, context_length=32)
    m = GPT(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                p.add_(0.3 * torch.randn_like(p))
    idx = torch.randint(0, 256, (2, 7))
    mk = lambda: KVCache(cfg.n_blocks, 2, 32, cfg.n_kv_head, cfg.head_dim, torch.float32, "cpu")  # noqa: E731
    c1, c2, c3 = mk(), mk(), mk()
    for c in (c1, c2, c3):
        forward_cached(m, idx[:, :6], c, 0)
    a = forward_cached(m, idx[:, 6:], c1, 6)
    b = forward_decode(m, idx[:, 6:], c2, torch.tensor([6]), torch.tensor([7], dtype=torch.int32))
    assert torch.allclose(a, b, atol=1e-5, rtol=1e-4)
    assert torch.equal(c1.k[1][:, :7], c2.k[1][:, :7])
    d = forward_decode(m, idx[:, 6:], c3, torch.tensor([6, 6]), torch.tensor([7, 7], dtype=torch.int32))
    assert torch.allclose(a, d, atol=1e-5, rtol=1e-4)
    assert torch.allclose(c1.k[1][:, :7], c3.k[1][:, :7], atol=1e-6)
    # K is cached normalised: unit RMS up to the gains, not the raw projection's ~0.2
    assert abs(c1.k[0][:, :7].pow(2).mean().sqrt().item() - 1.0) < 0.3


@pytest.mark.parametrize("name", QKN_PRESETS)
def test_activation_checkpointing_same_grads(name):
    """tests/test_models.py::test_activation_checkpointing_same_grads with QK-norm."""
    torch.manual_seed(5)
    cfg = _cfg(name, vocab_size=512, context_length=64)
    m1 = GPT(cfg)
    m2 = GPT(cfg.replace(activation_checkpointing=True))
    m2.load_state_dict(m1.state_dict())
    x = torch.randint(0, 512, (2, 64))
    l1 = m1(x, x)[1]
    l1.backward()
    l2 = m2(x, x)[1]
    l2.backward()
    assert torch.allclose(l1, l2)
    names = [n for n, _ in m1.named_parameters()]
    assert any("q_norm" in n for n in names)
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert p1.grad is not None and torch.allclose(p1.grad, p2.grad, atol=1e-6), n
        if "q_norm" in n or "k_norm" in n:
            assert p1.grad.abs().sum() > 0, n
