"""Weight-only FP8 decode weights through the model on the CPU: what ``GPT.quantize_decode_weights`` quantises, when
the quantised copies are dropped, and which calls read them (``ops.linear`` / ``ops.norm_linear`` routing with the
``ops.reference`` math in the kernels' place)."""
import pytest
import torch

import _fp8_refs as R
from pretraining_llm_amd import ops
from pretraining_llm_amd.inference.generate import KVCache, forward_cached, forward_decode
from pretraining_llm_amd.models import GPT, get_preset
from pretraining_llm_amd.models.gpt import decode_weight

PRESETS = ("gpt2-tiny", "llama-tiny", "ref-small")


def _model(preset, **kw):
    torch.manual_seed(3)
    cfg = get_preset(preset).replace(vocab_size=512, context_length=64, **kw)
    if preset == "ref-small":  # the reference architecture (ReLU, no W_o, biased untied head) at tiny dims
        cfg = cfg.replace(n_embed=128, n_head=4, n_kv_head=4, n_blocks=2, ffn_hidden=512)
    return GPT(cfg).eval()


def _quantised(model):
    return [n for n, p in model._decode_weight_params() if isinstance(decode_weight(p), ops.Fp8Weight)]


@pytest.mark.parametrize("preset", PRESETS)
def test_quantize_decode_weights_covers_the_decode_projections(preset):
    m = _model(preset)
    keys = list(m.state_dict().keys())
    assert m.decode_weights is None and _quantised(m) == []
    names = m.quantize_decode_weights("fp8")
    per_block = 4 if m.attn_blocks[0].attn.proj is not None else 3
    assert len(names) == per_block * len(m.attn_blocks) + 1 and names == _quantised(m)
    assert names[-1] == ("token_embed.weight" if m.lm_head is None else "lm_head.weight")
    assert m.decode_weights == "fp8" and list(m.state_dict().keys()) == keys
    for _, p in m._decode_weight_params():
        fw = decode_weight(p)
        assert fw.ref is p and fw.q.dtype == torch.uint8 and fw.q.shape == p.shape and fw.scale.shape == p.shape[:1]
        q, s = R.quant_ref(p)
        assert torch.equal(fw.q, q) and torch.equal(fw.scale, s)
    with pytest.raises(ValueError):
        m.quantize_decode_weights("int4")


def test_train_load_state_dict_and_to_drop_the_quantised_weights():
    m = _model("gpt2-tiny")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for drop in (lambda: m.train(), lambda: m.load_state_dict(sd), lambda: m.to(torch.bfloat16)):
        m.eval()
        m.quantize_decode_weights()
        assert m.decode_weights == "fp8"
        drop()
        assert m.decode_weights is None and _quantised(m) == []
    m.train()
    with pytest.raises(RuntimeError):
        m.quantize_decode_weights()  # eval mode only
    m.eval()
    m.quantize_decode_weights()
    m.eval()  # eval() itself keeps them
    assert m.decode_weights == "fp8"


def test_model_parallel_models_are_refused():
    from pretraining_llm_amd.parallel.model_parallel import ParallelGroups
    for kw in (dict(tp=2), dict(cp=2)):
        m = _model("gpt2-tiny")
        m.parallel = ParallelGroups(world=2, **kw)
        with pytest.raises(ValueError):
            m.quantize_decode_weights()
        assert m.decode_weights is None


def test_unsupported_k_stays_bf16_and_nonfinite_weights_raise():
    m = _model("gpt2-tiny", ffn_hidden=132)  # mlp.proj: K = 132, not a multiple of 8
    names = m.quantize_decode_weights()
    kept = [n for n, _ in m._decode_weight_params() if n not in names]
    assert kept == [f"attn_blocks.{i}.mlp.proj.weight" for i in range(len(m.attn_blocks))]
    assert ops.quantize_weight_fp8(torch.zeros(8, 12)) is None
    assert ops.quantize_weight_fp8(torch.zeros(16, 8).t()) is None  # not contiguous
    with torch.no_grad():
        m.attn_blocks[0].attn.qkv.weight[3, 5] = float("nan")
    with pytest.raises(ValueError):
        m.quantize_decode_weights()


def _dequantised_twin(m, preset, **kw):
    """A model whose decode weights ARE the dequantised values, without quantised copies."""
    tied = m.lm_head is None  # the embedding lookup keeps the bf16 table: the twin's head is a matrix of its own
    twin = _model(preset, **(dict(kw, tie_embeddings=False, head_bias=False) if tied else kw))
    sd = dict(m.state_dict())
    if tied:
        sd["lm_head.weight"] = m.token_embed.weight.detach().clone()
    twin.load_state_dict(sd)
    with torch.no_grad():
        for (_, p), (_, src) in zip(twin._decode_weight_params(), m._decode_weight_params()):
            fw = decode_weight(src)
            p.copy_(ops.dequantize_fp8(fw.q, fw.scale))
    return twin


def _steps(m, B, T):
    cfg = m.config
    torch.manual_seed(9)
    idx = torch.randint(0, 512, (B, T + 1))
    cache = KVCache(cfg.n_blocks, B, 64, cfg.n_kv_head, cfg.head_dim, torch.float32, idx.device)
    pre = forward_cached(m, idx[:, :T], cache, 0)
    pos_t = torch.tensor([T])
    dec = forward_decode(m, idx[:, T:], cache, pos_t, (pos_t + 1).int())
    return pre, dec, cache


@pytest.mark.parametrize("preset", PRESETS)
def test_more_than_8_rows_read_the_bf16_weights_bit_identically(preset):
    m = _model(preset)
    pre0, dec0, _ = _steps(m, 9, 2)  # 18 rows in the blocks, 9 at the head
    m.quantize_decode_weights()
    pre1, dec1, _ = _steps(m, 9, 2)
    assert torch.equal(pre0, pre1) and torch.equal(dec0, dec1)


@pytest.mark.parametrize("preset", PRESETS)
def test_at_most_8_rows_compute_the_dequantised_reference_math(preset):
    m = _model(preset)
    pre0, dec0, _ = _steps(m, 2, 3)
    m.quantize_decode_weights()
    twin = _dequantised_twin(m, preset)
    pre1, dec1, c1 = _steps(m, 2, 3)    # 6 rows, then 2
    pre2, dec2, c2 = _steps(twin, 2, 3)
    assert not torch.equal(pre0, pre1) and not torch.equal(dec0, dec1)  # the quantised values are in use
    for a, b in ((pre1, pre2), (dec1, dec2), (c1.k[-1][:, :4], c2.k[-1][:, :4]), (c1.v[-1][:, :4], c2.v[-1][:, :4])):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), (a - b).abs().max()  # fp32 both: summation order only
    with torch.enable_grad():  # grad mode: the bf16 parameters, whatever the row count
        x = torch.randn(2, 1, m.config.n_embed)
        w = m.attn_blocks[0].attn.qkv.weight
        assert torch.equal(ops.linear(x, decode_weight(w)), torch.nn.functional.linear(x, w))


def test_linear_and_norm_linear_reference_math():
    torch.manual_seed(1)
    w, b = torch.randn(24, 16), torch.randn(24)
    fw = ops.quantize_weight_fp8(w)
    x = torch.randn(2, 3, 16)
    dq = ops.dequantize_fp8(fw.q, fw.scale)
    assert torch.equal(dq, R.dq64(fw.q, fw.scale).float())
    with torch.no_grad():
        assert torch.equal(ops.linear(x, fw, b), (x @ dq.t() + b))
        g = torch.ones(16)
        y, s = ops.norm_linear(x, None, g, None, 1e-5, True, fw, b, act="relu")
        h = ops.rms_norm(x, g, 1e-5, None)[0]
        assert torch.equal(y, torch.relu(h @ dq.t() + b)) and s is x
        x9 = torch.randn(9, 16)
        assert torch.equal(ops.linear(x9, fw, b), torch.nn.functional.linear(x9, w, b))
        with ops.backend("torch"):
            assert torch.equal(ops.linear(x, fw, b), (x @ dq.t() + b))
