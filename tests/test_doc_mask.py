"""Document masking at model level on the CPU (``ModelConfig.doc_mask``): the config plumbing, that no parameter or
state-dict key changes, and that a token's logits depend on its own document only."""
import pytest
import torch

from pretraining_llm_amd.models import GPT, ModelConfig, get_preset

SEP = 7  # a separator inside the tiny vocabularies
V, T = 64, 24


def _cfg(name, **kw):
    return get_preset(name).replace(vocab_size=V, context_length=32, doc_mask=True, doc_sep_token=SEP, **kw)


def _model(name, **kw):
    torch.manual_seed(0)
    return GPT(_cfg(name, **kw)).float().eval()


def _tokens(seed=0, B=2):
    """Two documents per row: [0, 10) ending with the separator at 9, and [10, T)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(SEP + 1, V, (B, T), generator=g)
    idx[:, 9] = SEP
    return idx


# ---------------------------------------------------------------------------------------------- plumbing
def test_config_round_trip_and_defaults():
    base = get_preset("llama-tiny")
    assert not base.doc_mask and base.doc_sep_token == 50256 and not ModelConfig().doc_mask
    cfg = base.replace(doc_mask=True, doc_sep_token=5)
    d = cfg.to_dict()
    assert d["doc_mask"] is True and d["doc_sep_token"] == 5
    assert ModelConfig.from_dict(d) == cfg
    old = {k: v for k, v in base.to_dict().items() if not k.startswith("doc_")}
    assert ModelConfig.from_dict(old) == base  # a checkpoint from before the keys existed
    for bad in (-1, base.vocab_size, 50256):   # llama-tiny's vocabulary is 512
        with pytest.raises(ValueError, match="doc_sep_token"):
            base.replace(doc_mask=True, doc_sep_token=bad)
    base.replace(doc_mask=False, doc_sep_token=50256)  # only checked when the mask is on
    assert get_preset("gpt2-tiny").replace(doc_mask=True).doc_sep_token == 50256  # GPT-2's vocabulary holds it


def test_checkpoint_config_round_trip(tmp_path):
    from pretraining_llm_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    m = _model("llama-tiny")
    path = str(tmp_path / "m.pt")
    save_checkpoint(path, m)
    ckpt = load_checkpoint(path)
    cfg = ModelConfig.from_dict(ckpt["model_config"])
    assert cfg.doc_mask and cfg.doc_sep_token == SEP and cfg == m.config
    GPT(cfg).load_state_dict(ckpt["model_state_dict"])


@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_no_new_parameters_or_keys(name):
    on = _cfg(name)
    off = on.replace(doc_mask=False)
    a, b = GPT(on), GPT(off)
    assert list(a.state_dict()) == list(b.state_dict())
    assert on.num_params() == off.num_params() == sum(p.numel() for p in a.parameters())


def test_tp_cp_rejected_before_any_collective():
    from config.config import default_config
    from pretraining_llm_amd.parallel.model_parallel import parallelize_gpt
    from pretraining_llm_amd.train.trainer import Trainer

    class PG:  # what parallelize_gpt reads
        tp, cp, sequence_parallel, cp_mode = 2, 1, False, "ring"
    m = GPT(_cfg("llama-tiny"))
    with pytest.raises(ValueError, match="doc_mask"):
        parallelize_gpt(m, PG)
    PG.tp, PG.cp = 1, 2
    with pytest.raises(ValueError, match="doc_mask"):
        parallelize_gpt(m, PG)
    assert m.parallel is None and type(m.attn_blocks[0].attn).__name__ == "Attention"  # nothing was sharded
    for kw in (dict(tp_size=2), dict(cp_size=2)):
        cfg = dict(default_config)
        cfg.update(model_preset="llama-tiny", doc_mask=True, doc_sep_token=SEP, device="cpu", **kw)
        with pytest.raises(ValueError, match="doc_mask"):  # no process group exists yet: raised before init
            Trainer(cfg, log=lambda *_: None)
        assert not torch.distributed.is_initialized()


def test_model_config_from_forwards_keys():
    from config.config import default_config
    from pretraining_llm_amd.train import model_config_from
    assert default_config["doc_mask"] is None and default_config["doc_sep_token"] is None
    cfg = dict(default_config)
    cfg.update(model_preset="llama-tiny")
    assert not model_config_from(cfg).doc_mask
    cfg.update(doc_mask=True, doc_sep_token=SEP)
    mc = model_config_from(cfg)
    assert mc == get_preset("llama-tiny").replace(doc_mask=True, doc_sep_token=SEP)
    cfg.update(doc_mask=None, doc_sep_token=None)
    assert model_config_from(cfg) == get_preset("llama-tiny")  # None leaves the preset's value


def test_train_script_accepts_doc_mask_flag():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_transformer.py")
    spec = importlib.util.spec_from_file_location("_train_transformer_doc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pretraining_llm_amd.train import model_config_from
    cfg = mod.build_config(["--preset=gpt2-small", "--doc_mask=True"])
    assert cfg["doc_mask"] is True
    mc = model_config_from(cfg)
    assert mc.doc_mask and mc.doc_sep_token == 50256 and mc == get_preset(cfg["model_preset"]).replace(doc_mask=True)
    cfg = mod.build_config(["--preset=gpt2-small", "--doc_mask=True", "--doc_sep_token=11"])
    assert model_config_from(cfg).doc_sep_token == 11


# ---------------------------------------------------------------------------------------------- isolation
@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_document_two_does_not_see_document_one(name):
    m = _model(name)
    a = _tokens()
    b = a.clone()
    b[:, :9] = torch.randint(SEP + 1, V, (2, 9), generator=torch.Generator().manual_seed(1))  # another document 1
    assert not torch.equal(a[:, :9], b[:, :9])
    with torch.no_grad():
        la, lb = m(a)[0], m(b)[0]
        assert (la[:, 10:] - lb[:, 10:]).abs().max() <= 1e-5
        assert (la[:, :9] - lb[:, :9]).abs().max() > 1e-3  # document 1 itself did change
        # without the flag the same change reaches document 2
        ua, ub = m(a, doc_mask=False)[0], m(b, doc_mask=False)[0]
        assert (ua[:, 10:] - ub[:, 10:]).abs().max() > 1e-3
        off = GPT(m.config.replace(doc_mask=False)).float().eval()
        off.load_state_dict(m.state_dict())
        assert torch.equal(off(a)[0], ua)


def test_rope_document_two_equals_document_two_alone():
    """RoPE is relative, so within a document the window position does not matter: document 2 inside the window has
    the logits of document 2 fed alone."""
    m = _model("llama-tiny")
    a = _tokens()
    with torch.no_grad():
        full, alone = m(a)[0], m(a[:, 10:].contiguous())[0]
    assert (full[:, 10:] - alone).abs().max() <= 1e-4


def test_learned_positions_keep_the_window_position():
    m = _model("gpt2-tiny")
    a = _tokens()
    with torch.no_grad():
        full, alone = m(a)[0], m(a[:, 10:].contiguous())[0]
    assert (full[:, 10:] - alone).abs().max() > 1e-3


@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_activation_checkpointing_gives_the_same_gradients(name):
    a = _tokens()
    y = torch.roll(a, -1, 1)
    grads = []
    for ckpt in (False, True):
        torch.manual_seed(0)
        m = GPT(_cfg(name, activation_checkpointing=ckpt)).float().train()
        _, loss = m(a, y)
        loss.backward()
        grads.append((loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    assert torch.allclose(grads[0][0], grads[1][0], atol=1e-6)
    for n, g in grads[0][1].items():
        torch.testing.assert_close(grads[1][1][n], g, rtol=1e-5, atol=1e-6, msg=n)


@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_cached_generation_matches_recompute(name):
    m = _model(name)
    prompt = _tokens(B=1)[:, :14]  # holds a separator: generation treats the context as one document
    out_c = m.generate(prompt, 8, temperature=0.0, use_cache=True)
    out_r = m.generate(prompt, 8, temperature=0.0, use_cache=False)
    assert torch.equal(out_c, out_r)
    # the cached path sees the whole context, separator or not: its first new token is the unmasked model's
    with torch.no_grad():
        assert torch.equal(out_c[:, 14], m(prompt, doc_mask=False)[0][:, -1].argmax(-1))
