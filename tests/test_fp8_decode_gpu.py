"""Weight-only FP8 decode through the model on the GPU: a model whose weights lie on the e4m3fn grid computes the
same function from its codes as from its bf16 parameters (logits and KV caches), hipGraph replay equals eager
decoding, and the quantised layers run ``gemv_fp8`` -- never ``gemv`` -- exactly when a call has at most 8 rows."""
import collections

import pytest
import torch

import _fp8_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRESETS = ("gpt2-tiny", "llama-tiny", "ref-small")


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _model(preset, seed=5, ctx=64):
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(seed)
    cfg = get_preset(preset).replace(vocab_size=512, context_length=ctx)
    if preset == "ref-small":  # reference architecture (ReLU, no W_o, biased untied head), tiny dims
        cfg = cfg.replace(n_embed=128, n_head=4, n_kv_head=4, n_blocks=2, ffn_hidden=512)
    return GPT(cfg).to(DEV, torch.bfloat16).eval()


def _decode(m, idx, pos):
    """Prefill idx[:, :-1], then one decode step at ``pos`` ([1] or [B]) -> (prefill logits, step logits, cache)."""
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached, forward_decode
    cfg = m.config
    with torch.no_grad():
        cache = KVCache(cfg.n_blocks, idx.shape[0], 64, cfg.n_kv_head, cfg.head_dim, torch.bfloat16, idx.device)
        pre = forward_cached(m, idx[:, :-1], cache, 0)
        pos_t = torch.tensor(pos, device=DEV)
        dec = forward_decode(m, idx[:, -1:], cache, pos_t, (pos_t + 1).int())
    return pre, dec, cache


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("per_row", [False, True])
def test_lossless_grid_model_is_the_same_function(preset, per_row):
    m = _model(preset)
    R.snap_to_fp8_grid(m)
    idx = torch.randint(0, 512, (2, 20), device=DEV)
    pos = [19, 18] if per_row else [19]
    pre0, dec0, c0 = _decode(m, idx, pos)
    assert len(m.quantize_decode_weights()) == len(m._decode_weight_params()) and m.decode_weights == "fp8"
    for _, p in m._decode_weight_params():  # quantisation is exact on this model
        fw = p._pllm_decode_weight
        assert torch.equal(R.dq64(fw.q, fw.scale).to(torch.bfloat16), p.detach().cpu())
    pre1, dec1, c1 = _decode(m, idx, pos)
    print("prefill rel", _rel(pre1, pre0), "step rel", _rel(dec1, dec0), "bitwise", torch.equal(dec1, dec0))
    assert torch.isfinite(dec1).all()
    assert _rel(pre1, pre0) < 3e-2 and _rel(dec1, dec0) < 3e-2
    if m.config.pos != "rope":  # the QKV projection's epilogue appends: the caches of the two runs agree bitwise
        for l in range(m.config.n_blocks):
            for b, p in enumerate(pos if per_row else pos * 2):  # the slots written so far: row b's 0 .. p
                assert torch.equal(c1.k[l][b, :p + 1], c0.k[l][b, :p + 1])
                assert torch.equal(c1.v[l][b, :p + 1], c0.v[l][b, :p + 1])


@pytest.mark.parametrize("preset", ["gpt2-tiny", "llama-tiny"])
def test_graphed_fp8_decode_matches_eager(preset):
    m = _model(preset, seed=11, ctx=96)
    m.quantize_decode_weights()
    idx = torch.randint(0, 512, (3, 9), device=DEV)
    a = m.generate(idx, 24, temperature=0.0, cuda_graph=False)
    b = m.generate(idx, 24, temperature=0.0, cuda_graph=True)
    assert torch.equal(a, b)


class _Counting:
    """torch.ops.pllm with a Python-side call counter per op."""

    def __init__(self):
        self.calls = collections.Counter()

    def __getattr__(self, name):
        op = getattr(torch.ops.pllm, name)

        def call(*a, **kw):
            self.calls[name] += 1
            return op(*a, **kw)
        return call


@pytest.mark.parametrize("preset", ["gpt2-tiny", "llama-tiny"])
def test_routing_by_row_count(preset, monkeypatch):
    from pretraining_llm_amd import ops
    m = _model(preset, seed=2)
    counter = _Counting()
    monkeypatch.setattr(ops, "_ops", lambda: counter)
    idx = torch.randint(0, 512, (2, 9), device=DEV)
    m.generate(idx, 3, temperature=0.0)
    assert counter.calls["gemv"] > 0 and counter.calls["gemv_fp8"] == 0  # bf16 weights
    m.quantize_decode_weights()
    counter.calls.clear()
    m.generate(idx, 3, temperature=0.0)
    per_step = 4 * m.config.n_blocks + 1
    assert counter.calls["gemv_fp8"] >= 2 * per_step and counter.calls["gemv"] == 0, dict(counter.calls)
    counter.calls.clear()
    m.generate(torch.randint(0, 512, (9, 9), device=DEV), 3, temperature=0.0)  # 9 rows: neither
    assert counter.calls["gemv_fp8"] == 0 and counter.calls["gemv"] == 0, dict(counter.calls)
