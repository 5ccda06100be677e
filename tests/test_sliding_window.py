"""Sliding-window attention at model level on the CPU (``ModelConfig.sliding_window`` / ``sliding_window_pattern``):
the config plumbing, the closed-form bounds, the receptive field of local and global layers, and that every inference
path (recompute, KV cache, device-position decode step, right-padded batched prefill) applies the same window."""
import pytest
import torch

from pretraining_llm_amd import ops
from pretraining_llm_amd.models import GPT, ModelConfig, get_preset

V = 64


def _cfg(name="llama-tiny", **kw):
    kw.setdefault("sliding_window", 8)
    return get_preset(name).replace(vocab_size=V, context_length=96, **kw)


def _model(name="llama-tiny", **kw):
    torch.manual_seed(0)
    return GPT(_cfg(name, **kw)).float().eval()


def _tokens(B=2, T=64, seed=0, lo=0):
    return torch.randint(lo, V, (B, T), generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------- config
def test_config_round_trip_and_layer_window():
    base = get_preset("llama-tiny")
    assert base.sliding_window is None and base.sliding_window_pattern == 0 and ModelConfig().sliding_window is None
    assert all(base.layer_window(l) is None for l in range(4))
    cfg = base.replace(sliding_window=16, sliding_window_pattern=2)
    d = cfg.to_dict()
    assert d["sliding_window"] == 16 and d["sliding_window_pattern"] == 2
    assert ModelConfig.from_dict(d) == cfg
    old = {k: v for k, v in base.to_dict().items() if not k.startswith("sliding_")}
    assert ModelConfig.from_dict(old) == base  # a checkpoint from before the keys existed
    # pattern 0: every layer local; n >= 2: layer l global iff (l + 1) % n == 0
    assert [base.replace(sliding_window=16).layer_window(l) for l in range(4)] == [16] * 4
    assert [cfg.layer_window(l) for l in range(6)] == [16, None, 16, None, 16, None]
    g3 = base.replace(sliding_window=5, sliding_window_pattern=6)
    assert [g3.layer_window(l) for l in range(13)] == [5] * 5 + [None] + [5] * 5 + [None] + [5]


def test_presets():
    tiny, big = get_preset("llama-tiny-swa"), get_preset("llama-1.3b-swa")
    assert tiny == get_preset("llama-tiny").replace(sliding_window=32, sliding_window_pattern=2)
    assert big == get_preset("llama-1.3b").replace(sliding_window=512, sliding_window_pattern=4)
    assert [tiny.layer_window(l) for l in range(2)] == [32, None]
    assert [big.layer_window(l) for l in range(24)].count(None) == 6


@pytest.mark.parametrize("kw", [dict(sliding_window=0), dict(sliding_window=-3),
                                dict(sliding_window=8, sliding_window_pattern=1),
                                dict(sliding_window=8, sliding_window_pattern=-2),
                                dict(sliding_window_pattern=2), dict(sliding_window_pattern=6)])
def test_invalid_config_raises(kw):
    with pytest.raises(ValueError, match="sliding_window"):
        get_preset("llama-tiny").replace(**kw)
    with pytest.raises(ValueError, match="sliding_window"):
        ModelConfig(**kw)


def test_checkpoint_config_round_trip(tmp_path):
    from pretraining_llm_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    m = _model(sliding_window=8, sliding_window_pattern=2)
    path = str(tmp_path / "m.pt")
    save_checkpoint(path, m)
    ckpt = load_checkpoint(path)
    cfg = ModelConfig.from_dict(ckpt["model_config"])
    assert cfg.sliding_window == 8 and cfg.sliding_window_pattern == 2 and cfg == m.config
    GPT(cfg).load_state_dict(ckpt["model_state_dict"])


@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_no_new_parameters_or_keys(name):
    on = _cfg(name, sliding_window_pattern=2)
    off = on.replace(sliding_window=None, sliding_window_pattern=0)
    a, b = GPT(on), GPT(off)
    assert list(a.state_dict()) == list(b.state_dict())
    assert on.num_params() == off.num_params() == sum(p.numel() for p in a.parameters())
    assert on.flops_per_token(64) == off.flops_per_token(64)  # the dense convention, as for doc_mask


def test_tp_cp_rejected_before_any_collective():
    from config.config import default_config
    from pretraining_llm_amd.parallel.model_parallel import parallelize_gpt
    from pretraining_llm_amd.train.trainer import Trainer

    class PG:  # what parallelize_gpt reads
        tp, cp, sequence_parallel, cp_mode = 2, 1, False, "ring"
    m = GPT(_cfg())
    with pytest.raises(ValueError, match="sliding_window"):
        parallelize_gpt(m, PG)
    PG.tp, PG.cp = 1, 2
    with pytest.raises(ValueError, match="sliding_window"):
        parallelize_gpt(m, PG)
    assert m.parallel is None and type(m.attn_blocks[0].attn).__name__ == "Attention"  # nothing was sharded

    class Sharded:  # a model some other way sharded: the trunk itself refuses
        tp, cp, sequence_parallel, cp_mode, model_parallel = 2, 1, False, "ring", True
    m.parallel = Sharded
    with pytest.raises(ValueError, match="sliding_window"):
        m._trunk(_tokens())
    for kw in (dict(tp_size=2), dict(cp_size=2)):
        cfg = dict(default_config)
        cfg.update(model_preset="llama-tiny-swa", device="cpu", **kw)
        with pytest.raises(ValueError, match="sliding_window"):  # no process group exists yet: raised before init
            Trainer(cfg, log=lambda *_: None)
        assert not torch.distributed.is_initialized()


def test_model_config_from_forwards_keys():
    from config.config import default_config
    from pretraining_llm_amd.train import model_config_from
    assert default_config["sliding_window"] is None and default_config["sliding_window_pattern"] is None
    cfg = dict(default_config)
    cfg.update(model_preset="llama-tiny")
    assert model_config_from(cfg).sliding_window is None
    cfg.update(sliding_window=16, sliding_window_pattern=2)
    assert model_config_from(cfg) == get_preset("llama-tiny").replace(sliding_window=16, sliding_window_pattern=2)
    cfg.update(model_preset="llama-tiny-swa", sliding_window=None, sliding_window_pattern=None)
    assert model_config_from(cfg) == get_preset("llama-tiny-swa")  # None leaves the preset's value
    cfg.update(sliding_window_pattern=0)  # 0 is a value, not "unset": every layer local
    assert model_config_from(cfg).sliding_window_pattern == 0


def test_train_script_accepts_the_keys():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_transformer.py")
    spec = importlib.util.spec_from_file_location("_train_transformer_swa", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pretraining_llm_amd.train import model_config_from
    cfg = mod.build_config(["--preset=llama-1.3b", "--sliding_window=512", "--sliding_window_pattern=4"])
    assert cfg["sliding_window"] == 512 and cfg["sliding_window_pattern"] == 4
    mc = model_config_from(cfg)
    assert mc == get_preset(cfg["model_preset"]).replace(sliding_window=512, sliding_window_pattern=4)
    assert mc == get_preset("llama-1.3b-swa")


# ---------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("W", [1, 2, 7, 24, 25, 10 ** 6])
def test_window_bounds_closed_form(W):
    B, T = 2, 24
    kv, ql = ops.window_bounds(B, T, W, "cpu")
    assert kv.dtype == ql.dtype == torch.int32 and kv.shape == ql.shape == (B, T)
    i = torch.arange(T)
    assert torch.equal(kv[0].long(), (i - W + 1).clamp_min(0)) and torch.equal(kv[0], kv[1])
    assert torch.equal(ql, ops.bounds_from_start(kv))
    if W >= T:  # does not bite: plain causal
        assert not kv.any() and (ql == T - 1).all()


@pytest.mark.parametrize("W", [1, 3, 8, 24, 40])
def test_window_bounds_with_documents(W):
    B, T, SEP = 3, 24, 7
    idx = _tokens(B, T, seed=2, lo=SEP + 1)
    idx[0, 9] = SEP
    idx[1, [0, 1, 15]] = SEP
    idx[2, T - 1] = SEP
    doc = ops.doc_bounds(idx, SEP)
    kv, ql = ops.window_bounds(B, T, W, "cpu", doc=doc)
    i = torch.arange(T).expand(B, T)
    assert torch.equal(kv.long(), torch.maximum(doc[0].long(), i - W + 1))
    assert torch.equal(ql.long(), torch.minimum(doc[1].long(), i + W - 1))
    assert torch.equal(ql, ops.bounds_from_start(kv)) and kv.dtype == ql.dtype == torch.int32


# ---------------------------------------------------------------------------------------------- receptive field
def _changed(m, t, T=64):
    """Per position: did the logits change when token ``t`` did?"""
    a = _tokens(1, T)
    b = a.clone()
    b[0, t] = (a[0, t] + 1) % V
    with torch.no_grad():
        la, lb = m(a)[0], m(b)[0]
    return [not torch.equal(la[0, p], lb[0, p]) for p in range(T)]


@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_receptive_field_of_one_local_block(name):
    W, t = 8, 20
    ch = _changed(_model(name, n_blocks=1, sliding_window=W), t)
    assert not any(ch[:t]) and all(ch[t:t + W]) and not any(ch[t + W:])  # exactly unchanged from t + W on
    assert all(_changed(_model(name, n_blocks=1, sliding_window=None), t)[t:])


def test_receptive_field_of_two_blocks():
    W, t = 8, 20
    ch = _changed(_model(n_blocks=2, sliding_window=W), t)  # two local blocks: W - 1 further each
    assert not any(ch[:t]) and all(ch[t:t + 2 * W - 1]) and not any(ch[t + 2 * W - 1:])
    ch = _changed(_model(n_blocks=2, sliding_window=W, sliding_window_pattern=2), t)  # the global block sees all
    assert not any(ch[:t]) and all(ch[t:])


# ---------------------------------------------------------------------------------------------- equivalence
@pytest.mark.parametrize("W", [64, 65, 10 ** 6])
def test_window_that_does_not_bite_is_the_dense_model(W, monkeypatch):
    m = _model(sliding_window=W)
    dense = GPT(m.config.replace(sliding_window=None)).float().eval()
    dense.load_state_dict(m.state_dict())
    calls = []
    real = ops.window_bounds
    monkeypatch.setattr(ops, "window_bounds", lambda *a, **k: calls.append(a) or real(*a, **k))
    idx = _tokens()
    with torch.no_grad():
        assert torch.equal(m(idx)[0], dense(idx)[0])
    assert not calls  # W >= T on the host: the local layers take the global layers' bounds (none)
    out_w = m.generate(idx[:, :10], 12, temperature=0.0)
    assert torch.equal(out_w, dense.generate(idx[:, :10], 12, temperature=0.0))


@pytest.mark.parametrize("name,kw", [("llama-tiny", dict(sliding_window_pattern=2)), ("llama-tiny", {}),
                                     ("gpt2-tiny", {}), ("llama-tiny", dict(qk_norm=True))])
def test_cached_generation_matches_recompute(name, kw):
    """A prompt longer than the window, generation crossing several windows."""
    m = _model(name, **kw)
    prompt = _tokens(2, 13, seed=4)
    out_c = m.generate(prompt, 30, temperature=0.0, use_cache=True)
    out_r = m.generate(prompt, 30, temperature=0.0, use_cache=False)
    assert torch.equal(out_c, out_r)
    dense = GPT(m.config.replace(sliding_window=None, sliding_window_pattern=0)).float().eval()
    dense.load_state_dict(m.state_dict())
    with torch.no_grad():  # the window is in force on both paths
        full = torch.cat([prompt, out_c[:, 13:]], 1)
        assert (m(full)[0][:, -1] - dense(full)[0][:, -1]).abs().max() > 1e-3


@pytest.mark.parametrize("name", ["gpt2-tiny", "llama-tiny"])
@pytest.mark.parametrize("per_row", [False, True])
def test_device_position_decode_step_matches_cached(name, per_row):
    """forward_decode (device position; one per row under continuous batching) against the host-position step and
    against recompute, at the tolerances of tests/test_models.py (atol 1e-5, rtol 1e-4)."""
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached, forward_decode
    m = _model(name, sliding_window_pattern=2)
    cfg = m.config
    idx = _tokens(2, 31, seed=6)
    mk = lambda B: KVCache(cfg.n_blocks, B, 48, cfg.n_kv_head, cfg.head_dim, torch.float32, "cpu")  # noqa: E731
    if not per_row:
        c1, c2 = mk(2), mk(2)
        forward_cached(m, idx[:, :30], c1, 0)
        forward_cached(m, idx[:, :30], c2, 0)
        a = forward_cached(m, idx[:, 30:], c1, 30)
        b = forward_decode(m, idx[:, 30:], c2, torch.tensor([30]), torch.tensor([31], dtype=torch.int32))
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-4)
        with torch.no_grad():
            assert torch.allclose(m(idx)[0][:, -1], b, atol=1e-5, rtol=1e-4)
        return
    # one window, one count per slot: rows at positions 30 (past the window) and 5 (inside it)
    lens = (30, 5)
    c = mk(2)
    want = []
    for r, n in enumerate(lens):
        one = mk(1)
        forward_cached(m, idx[r:r + 1, :n], one, 0)
        for l in range(cfg.n_blocks):
            c.k[l][r, :n], c.v[l][r, :n] = one.k[l][0, :n], one.v[l][0, :n]
        want.append(forward_cached(m, idx[r:r + 1, n:n + 1], one, n))
    tok = torch.stack([idx[0, 30:31], idx[1, 5:6]])
    pos = torch.tensor(lens)
    got = forward_decode(m, tok, c, pos, (pos + 1).to(torch.int32))
    assert torch.allclose(got, torch.cat(want), atol=1e-5, rtol=1e-4)


def test_chunked_prefill_on_a_local_layer_is_refused():
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached
    m = _model()
    cfg = m.config
    c = KVCache(cfg.n_blocks, 1, 48, cfg.n_kv_head, cfg.head_dim, torch.float32, "cpu")
    idx = _tokens(1, 20)
    forward_cached(m, idx[:, :10], c, 0)
    with pytest.raises(NotImplementedError, match="sliding_window"):
        forward_cached(m, idx[:, 10:], c, 10)


def test_right_padded_batched_prefill_matches_per_prompt_prefill():
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached
    m = _model(sliding_window_pattern=2)
    cfg = m.config
    lens = [30, 9, 17]
    idx = _tokens(3, 30, seed=8)
    mk = lambda B: KVCache(cfg.n_blocks, B, 32, cfg.n_kv_head, cfg.head_dim, torch.float32, "cpu")  # noqa: E731
    got = forward_cached(m, idx, mk(3), 0, last=torch.tensor(lens) - 1)
    for r, n in enumerate(lens):
        want = forward_cached(m, idx[r:r + 1, :n], mk(1), 0)
        assert torch.allclose(got[r:r + 1], want, atol=1e-5, rtol=1e-4), r


@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_activation_checkpointing_gives_the_same_gradients(name):
    a = _tokens()
    y = torch.roll(a, -1, 1)
    grads = []
    for ckpt in (False, True):
        torch.manual_seed(0)
        m = GPT(_cfg(name, sliding_window_pattern=2, activation_checkpointing=ckpt)).float().train()
        _, loss = m(a, y)
        loss.backward()
        grads.append((loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    assert torch.allclose(grads[0][0], grads[1][0], atol=1e-6)
    for n, g in grads[0][1].items():
        torch.testing.assert_close(grads[1][1][n], g, rtol=1e-5, atol=1e-6, msg=n)


def test_doc_mask_and_window_equal_the_explicit_mask(monkeypatch):
    """One local block with doc_mask: the attention output equals softmax under the explicit boolean mask
    (same document, j <= i, i - j < W); ``doc_mask=False`` turns off only the document part."""
    from pretraining_llm_amd.ops import reference as ref
    SEP, W, T = 7, 8, 40
    m = _model(n_blocks=1, sliding_window=W, doc_mask=True, doc_sep_token=SEP)
    idx = _tokens(2, T, seed=9, lo=SEP + 1)
    idx[0, 11], idx[1, 3], idx[1, 25] = SEP, SEP, SEP
    doc_id = torch.cumsum(torch.nn.functional.pad((idx == SEP)[:, :-1], (1, 0)).long(), 1)  # a separator ends its doc
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    win = (j <= i) & (i - j < W)
    both = win[None] & (doc_id[:, :, None] == doc_id[:, None, :])

    def masked(mask):
        def attention(q, k, v, causal=True, scale=None, bounds=None):
            B, T_, H, D = q.shape
            rep = H // k.shape[2]
            kf, vf = (t.float().repeat_interleave(rep, dim=2).transpose(1, 2) for t in (k, v))
            s = (q.float().transpose(1, 2) @ kf.transpose(-1, -2)) * (scale if scale is not None else D ** -0.5)
            s = s.masked_fill(~mask.expand(B, T_, T_)[:, None], float("-inf"))
            return (torch.softmax(s, -1) @ vf).transpose(1, 2).to(q.dtype), torch.logsumexp(s, -1)
        return attention

    with torch.no_grad():
        got, got_win = m(idx)[0], m(idx, doc_mask=False)[0]
        monkeypatch.setattr(ref, "attention", masked(both))
        want = m(idx)[0]
        monkeypatch.setattr(ref, "attention", masked(win[None]))
        want_win = m(idx)[0]
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-4)
    assert torch.allclose(got_win, want_win, atol=1e-5, rtol=1e-4)
    assert (got - got_win).abs().max() > 1e-3


def test_forward_embedding_applies_the_window():
    m = _model(n_blocks=2, sliding_window=8)
    a = _tokens(1, 40)
    b = a.clone()
    b[0, 3] = (a[0, 3] + 1) % V
    with torch.no_grad():
        (ha, ra), (hb, rb) = m.forward_embedding(a), m.forward_embedding(b)
    assert torch.equal(ha[:, 3 + 15:], hb[:, 3 + 15:]) and not torch.equal(ha[:, 3 + 14], hb[:, 3 + 14])


@pytest.mark.parametrize("name,kw", [("llama-tiny-swa", {}), ("gpt2-tiny", dict(sliding_window=16)),
                                     ("llama-tiny", dict(sliding_window=16, doc_mask=True, doc_sep_token=7))],
                         ids=["llama-tiny-swa", "gpt2-tiny-w16", "llama-tiny-w16-doc"])
def test_window_moves_the_first_block_gradient(name, kw):
    """The margin the GPU test asserts (tests/test_sliding_window_gpu.py::test_model_hip_matches_reference_backend):
    at T = 128 the first block's qkv gradient with the window off differs by more than 0.2 relative (measured here in
    fp32 over three seeds: 0.39 .. 0.45, 0.75 .. 0.79, 0.29 .. 0.33)."""
    torch.manual_seed(10)
    cfg = get_preset(name).replace(context_length=128, **kw)
    m = GPT(cfg).float()
    x = torch.randint(8, cfg.vocab_size, (2, 128), generator=torch.Generator().manual_seed(0))
    if cfg.doc_mask:
        for b in range(2):
            for s in (5, 31, 64, 100):
                x[b, s + 3 * b] = 7
    y = torch.randint(0, cfg.vocab_size, (2, 128))
    off = GPT(cfg.replace(sliding_window=None, sliding_window_pattern=0)).float()
    off.load_state_dict(m.state_dict())
    grads = []
    for mdl in (m, off):
        mdl(x, y)[1].backward()
        grads.append(dict(mdl.named_parameters())["attn_blocks.0.attn.qkv.weight"].grad)
    assert ((grads[1] - grads[0]).norm() / grads[0].norm()).item() > 0.25
