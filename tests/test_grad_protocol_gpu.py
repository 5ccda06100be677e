"""The flat-gradient write protocol of the autograd functions in ops, end to end on five small models: every
backward takes its parameters' slots of the optimizer's flat gradient (``ops._take``), writes them, and notifies
the parameters (``ops._wrote``) exactly when it wrote.  parallel/dp.py and parallel/zero.py count those
notifications per parameter to launch their buckets and train/optim.py expects ``_pllm_grad_fresh`` consumed
once per slot per step, so the SEQUENCE of notified parameters is part of the contract: it is pinned here as
literal lists (recorded before the helpers of ops were factored out, they do not come from the code under
test), together with the freshness flags and the bits of the flat gradient over two micro-steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, T = 2, 128


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _cfg(name):
    from pretraining_llm_amd.models import get_preset
    if name in ("gpt2", "gpt2-unfused"):  # head dim 64: _AttnProjFn, the fused GELU MLP, residual-in-GEMM
        return get_preset("gpt2-tiny").replace(vocab_size=512, context_length=T, n_embed=128, n_head=2, n_blocks=2)
    if name == "ref":  # ReLU through gemm_lt, no W_o, biased untied head (the CE bias arm)
        return get_preset("ref-small").replace(vocab_size=512, context_length=T, n_embed=128, n_head=2, n_blocks=2)
    if name == "llama-sinks":  # attention sinks (their gradient: one reduction, _sink_bwd), local and global layers
        return get_preset("llama-tiny-sinks")
    return get_preset("llama-tiny-qknorm")  # fused SwiGLU, _FlashAttnPacked with RoPE and QK-norm, GQA


# The notified parameters of one backward, in order, as the commit before the helpers printed them.  gpt2, fused and
# unfused alike: a projection's bias comes from the backward of the norm that follows it (external bias
# gradients), so it is notified before its weight; the tied embedding is notified twice, by the LM head first and
# by the embedding scatter last.
EXPECTED = {
    "gpt2": [
        "token_embed.weight", "layer_norm.weight", "layer_norm.bias", "attn_blocks.1.mlp.proj.bias",
        "attn_blocks.1.mlp.proj.weight", "attn_blocks.1.mlp.hidden.bias", "attn_blocks.1.mlp.hidden.weight",
        "attn_blocks.1.ln2.weight", "attn_blocks.1.ln2.bias", "attn_blocks.1.attn.proj.bias",
        "attn_blocks.1.attn.proj.weight", "attn_blocks.1.attn.qkv.weight", "attn_blocks.1.attn.qkv.bias",
        "attn_blocks.1.ln1.weight", "attn_blocks.1.ln1.bias", "attn_blocks.0.mlp.proj.bias",
        "attn_blocks.0.mlp.proj.weight", "attn_blocks.0.mlp.hidden.bias", "attn_blocks.0.mlp.hidden.weight",
        "attn_blocks.0.ln2.weight", "attn_blocks.0.ln2.bias", "attn_blocks.0.attn.proj.bias",
        "attn_blocks.0.attn.proj.weight", "attn_blocks.0.attn.qkv.weight", "attn_blocks.0.attn.qkv.bias",
        "attn_blocks.0.ln1.weight", "attn_blocks.0.ln1.bias", "token_embed.weight", "position_embed.weight",
    ],
    "ref": [
        "lm_head.weight", "lm_head.bias", "layer_norm.weight", "layer_norm.bias", "attn_blocks.1.mlp.proj.weight",
        "attn_blocks.1.mlp.proj.bias", "attn_blocks.1.mlp.hidden.bias", "attn_blocks.1.mlp.hidden.weight",
        "attn_blocks.1.ln2.weight", "attn_blocks.1.ln2.bias", "attn_blocks.1.attn.qkv.weight",
        "attn_blocks.1.ln1.weight", "attn_blocks.1.ln1.bias", "attn_blocks.0.mlp.proj.weight",
        "attn_blocks.0.mlp.proj.bias", "attn_blocks.0.mlp.hidden.bias", "attn_blocks.0.mlp.hidden.weight",
        "attn_blocks.0.ln2.weight", "attn_blocks.0.ln2.bias", "attn_blocks.0.attn.qkv.weight",
        "attn_blocks.0.ln1.weight", "attn_blocks.0.ln1.bias", "token_embed.weight", "position_embed.weight",
    ],
    "llama-qknorm": [
        "lm_head.weight", "layer_norm.weight", "attn_blocks.1.mlp.proj.weight", "attn_blocks.1.mlp.hidden.weight",
        "attn_blocks.1.ln2.weight", "attn_blocks.1.attn.proj.weight", "attn_blocks.1.attn.q_norm.weight",
        "attn_blocks.1.attn.k_norm.weight", "attn_blocks.1.attn.qkv.weight", "attn_blocks.1.ln1.weight",
        "attn_blocks.0.mlp.proj.weight", "attn_blocks.0.mlp.hidden.weight", "attn_blocks.0.ln2.weight",
        "attn_blocks.0.attn.proj.weight", "attn_blocks.0.attn.q_norm.weight", "attn_blocks.0.attn.k_norm.weight",
        "attn_blocks.0.attn.qkv.weight", "attn_blocks.0.ln1.weight", "token_embed.weight",
    ],
    "gpt2-unfused": [
        "token_embed.weight", "layer_norm.weight", "layer_norm.bias", "attn_blocks.1.mlp.proj.bias",
        "attn_blocks.1.mlp.proj.weight", "attn_blocks.1.mlp.hidden.bias", "attn_blocks.1.mlp.hidden.weight",
        "attn_blocks.1.ln2.weight", "attn_blocks.1.ln2.bias", "attn_blocks.1.attn.proj.bias",
        "attn_blocks.1.attn.proj.weight", "attn_blocks.1.attn.qkv.weight", "attn_blocks.1.attn.qkv.bias",
        "attn_blocks.1.ln1.weight", "attn_blocks.1.ln1.bias", "attn_blocks.0.mlp.proj.bias",
        "attn_blocks.0.mlp.proj.weight", "attn_blocks.0.mlp.hidden.bias", "attn_blocks.0.mlp.hidden.weight",
        "attn_blocks.0.ln2.weight", "attn_blocks.0.ln2.bias", "attn_blocks.0.attn.proj.bias",
        "attn_blocks.0.attn.proj.weight", "attn_blocks.0.attn.qkv.weight", "attn_blocks.0.attn.qkv.bias",
        "attn_blocks.0.ln1.weight", "attn_blocks.0.ln1.bias", "token_embed.weight", "position_embed.weight",
    ],
    # (recorded at the commit before ``_take``, from the NOTIFIED line below)
    "llama-sinks": [
        "lm_head.weight", "layer_norm.weight", "attn_blocks.1.mlp.proj.weight", "attn_blocks.1.mlp.hidden.weight",
        "attn_blocks.1.ln2.weight", "attn_blocks.1.attn.proj.weight", "attn_blocks.1.attn.sinks",
        "attn_blocks.1.attn.qkv.weight", "attn_blocks.1.ln1.weight", "attn_blocks.0.mlp.proj.weight",
        "attn_blocks.0.mlp.hidden.weight", "attn_blocks.0.ln2.weight", "attn_blocks.0.attn.proj.weight",
        "attn_blocks.0.attn.sinks", "attn_blocks.0.attn.qkv.weight", "attn_blocks.0.ln1.weight",
        "token_embed.weight",
    ],
}


def _run(name, monkeypatch):
    """Two micro-steps (zero_grad before the first only) of a freshly built model -> (notified names of each
    micro-step, parameters left fresh after each, the flat gradient at the end)."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT
    from pretraining_llm_amd.train.optim import FlatAdamW
    if name == "gpt2-unfused":  # _LinearFn with bias; bias gradients from the norm and the activation backward
        monkeypatch.setattr(ops, "FUSED_MLP", False)
        monkeypatch.setattr(ops, "FUSED_ATTN_PROJ", False)
    cfg = _cfg(name)
    torch.manual_seed(0)
    model = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    opt = FlatAdamW(model, lr=1e-3, lazy_zero=True)
    assert opt.lazy_zero
    rec = []
    for n, p in zip(opt.names, opt.params):
        p._pllm_grad_ready = lambda n=n: rec.append(n)
    g = torch.Generator().manual_seed(1)
    notified, fresh = [], []
    opt.zero_grad()
    for _ in range(2):
        x = torch.randint(0, cfg.vocab_size, (B, T), generator=g).to(DEV)
        y = torch.randint(0, cfg.vocab_size, (B, T), generator=g).to(DEV)
        del rec[:]
        model(x, y, return_logits=False)[1].backward()
        notified.append(list(rec))
        fresh.append([n for n, p in zip(opt.names, opt.params) if getattr(p, "_pllm_grad_fresh", False)])
    torch.cuda.synchronize()
    return notified, fresh, opt.flat_grad.clone()


@pytest.mark.parametrize("name", ["gpt2", "ref", "llama-qknorm", "gpt2-unfused", "llama-sinks"])
def test_notifications_freshness_and_bits(name, monkeypatch):
    notified, fresh, flat = _run(name, monkeypatch)
    print(f"NOTIFIED {name} {notified!r}")  # (shown on failure, or with -s: how EXPECTED was recorded)
    assert notified[0] == EXPECTED[name], notified[0]
    assert notified[1] == EXPECTED[name], notified[1]  # a slot that is no longer fresh changes no notification
    assert fresh == [[], []], fresh
    # a second, freshly built identical model run the same way gives the same bits: a double write, a missed
    # zero or a read of a slot's stale contents would not
    notified2, _, flat2 = _run(name, monkeypatch)
    assert notified2 == notified
    assert torch.isfinite(flat).all() and flat.abs().sum() > 0
    assert torch.equal(flat, flat2)
