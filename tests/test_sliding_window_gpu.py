"""Sliding-window attention on the GPU: the windowed ``attn_decode`` kernel element by element against the fp64
references of ``_window_refs``, then the model -- the HIP path against the stock-torch backend, the captured (hipGraph)
training step, both servers, and a captured decode chain against recompute.  (The flash kernels with a window's
per-row bounds: tests/test_attention_seg_gpu.py, pattern ``window40``.)"""
import math

import pytest
import torch

import _attention_refs as A
import _window_refs as Wn

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEP = 7
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------------------------------------ kernel
def _seqlen(counts):
    if counts is None:
        return None
    return torch.tensor([counts] if isinstance(counts, int) else counts, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("case", Wn.window_cases(), ids=str)
def test_attn_decode_window_edges(case):
    """Every element within the ``decode_o`` budget; the rows below ``first`` and at or past the count are NaN."""
    D, Hq, Hkv, Bb, S, counts, W = case
    inp, ref = Wn.window_case(case)
    q, k, v = (inp[n].to(DEV) for n in ("q", "k", "v"))
    o = torch.ops.pllm.attn_decode(q, k, v, inp["scale"], _seqlen(counts), W)
    torch.cuda.synchronize()
    assert o.shape == (Bb, 1, Hq, D) and o.dtype == BF16
    print(f"decode window {case}: splits {Wn.window_splits(case)}, worst element "
          f"{A.worst_ratio('decode_o', o, ref):.2f} of its bound")
    A.check("decode_o", o, ref, f"o {case}")
    for b, n in enumerate(inp["counts"]):
        if n == 0:  # no key: exact zeros, no NaN
            assert not o[b].view(torch.int16).any()


@pytest.mark.parametrize("W", Wn.NO_BITE)
@pytest.mark.parametrize("counts", [None, 300, (300, 41)], ids=str)
def test_attn_decode_window_that_does_not_bite_is_bit_identical(W, counts):
    inp, _ = A.decode_case((64, 8, 4, 2, 300, counts))
    q, k, v = (inp[n].to(DEV) for n in ("q", "k", "v"))
    want = torch.ops.pllm.attn_decode(q, k, v, inp["scale"], _seqlen(counts))
    assert torch.equal(torch.ops.pllm.attn_decode(q, k, v, inp["scale"], _seqlen(counts), 0), want)
    got = torch.ops.pllm.attn_decode(q, k, v, inp["scale"], _seqlen(counts), W)
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all() and torch.equal(got, want)


def test_attn_decode_rejects_a_negative_window():
    inp, _ = A.decode_case((64, 8, 4, 2, 300, None))
    q, k, v = (inp[n].to(DEV) for n in ("q", "k", "v"))
    with pytest.raises(RuntimeError, match="window"):
        torch.ops.pllm.attn_decode(q, k, v, inp["scale"], None, -1)


def test_ops_attention_with_kv_start_on_a_cache_view():
    """ops.attention(kv_start=) -- the windowed prefill -- over k / v views of a longer cache, against fp32 math."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(5)
    B, T, H, Hkv, D, W = 2, 150, 4, 2, 32, 40
    q = (torch.randn(B, T, H, D, device=DEV) * 0.8).bfloat16()
    kc = (torch.randn(B, 200, Hkv, D, device=DEV) * 0.8).bfloat16()
    vc = torch.randn(B, 200, Hkv, D, device=DEV).bfloat16()
    kv = ops.window_bounds(B, T, W, DEV)[0]
    o = ops.attention(q, kc[:, :T], vc[:, :T], causal=True, kv_start=kv)
    want, _ = ref.attention(q.float(), kc[:, :T].float(), vc[:, :T].float(), causal=True, bounds=(kv, None))
    dense, _ = ref.attention(q.float(), kc[:, :T].float(), vc[:, :T].float(), causal=True)
    assert _rel(o, want) < 1.5e-2 and _rel(dense, want) > 0.3
    with pytest.raises(ValueError, match="kv_start"):
        ops.attention(q[:, :10], kc[:, :T], vc[:, :T], causal=True, kv_start=kv[:, :10])


# ------------------------------------------------------------------------------------------------ model
def _tokens(B, T, V, seps, seed=0):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(SEP + 1, V, (B, T), generator=g)
    for b in range(B):
        for s in seps:
            idx[b, (s + 3 * b) % T] = SEP
    return idx.to(DEV)


MODELS = [("llama-tiny-swa", {}), ("gpt2-tiny", dict(sliding_window=16)),
          ("llama-tiny", dict(sliding_window=16, doc_mask=True, doc_sep_token=SEP))]


@pytest.mark.parametrize("name,kw", MODELS, ids=lambda v: v if isinstance(v, str) else "-".join(v) or "preset")
def test_model_hip_matches_reference_backend(name, kw):
    """Loss and every parameter gradient on the HIP path against the stock-torch backend from the same weights;
    tolerances of tests/test_doc_mask_gpu.py (loss 2e-2, gradients 6e-2).  The window is in force: without it the
    first block's qkv gradient differs by more than 0.2 (0.29 .. 0.79 with the reference backend on the CPU, see
    tests/test_sliding_window.py::test_window_moves_the_first_block_gradient)."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(10)
    cfg = get_preset(name).replace(context_length=128, **kw)
    m = GPT(cfg).to(DEV, torch.bfloat16)
    x = _tokens(2, 128, cfg.vocab_size, (5, 31, 64, 100) if cfg.doc_mask else ())
    y = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    _, l1 = m(x, y, return_logits=False)
    l1.backward()
    g1 = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    m.zero_grad()
    off = GPT(cfg.replace(sliding_window=None, sliding_window_pattern=0)).to(DEV, torch.bfloat16)
    off.load_state_dict(m.state_dict())
    with ops.backend("torch"):
        _, l2 = m(x, y)
        l2.backward()
        _, l3 = off(x, y)
        l3.backward()
    assert abs(l1.item() - l2.item()) < 2e-2
    for n, p in m.named_parameters():
        assert _rel(g1[n], p.grad) < 6e-2, (n, _rel(g1[n], p.grad))
    n = "attn_blocks.0.attn.qkv.weight"
    assert _rel(dict(off.named_parameters())[n].grad, dict(m.named_parameters())[n].grad) > 0.2


class _Batches:
    """A stand-in for the trainer's loader: fixed batches that change from step to step."""

    def __init__(self, B, T, V):
        self.B, self.T, self.V, self.i = B, T, V, 0

    def next(self):
        i, self.i = self.i, self.i + 1
        x = _tokens(self.B, self.T, self.V, (), seed=100 + i)
        return x, torch.roll(x, -1, 1)


@pytest.mark.parametrize("name,kw", MODELS[:2], ids=["llama-tiny-swa", "gpt2-tiny-w16"])
def test_trainer_captured_step(name, kw, tmp_path, monkeypatch):
    """Trainer steps with the captured (hipGraph) step against the eager step from the same seed and batches: loss
    curves within 2e-3 and weights within 1e-3, the bounds of tests/test_doc_mask_gpu.py."""
    from config.config import default_config
    from pretraining_llm_amd.train.trainer import Trainer
    monkeypatch.delenv("TORCH_COMPILE", raising=False)
    base = dict(default_config)
    base.update(model_preset=name, t_batch_size=4, seq_len=128, t_train_steps=4, t_lr=1e-3, warmup_steps=1,
                log_interval=1, t_eval_steps=1000, eval_at_start=False, t_out_path=None, synthetic_data=True,
                synthetic_tokens=200_000, synthetic_dir=str(tmp_path), max_grad_norm=1.0, device="cuda", **kw)
    curves, weights = {}, {}
    for comp in (True, False):
        recs = []
        tr = Trainer(dict(base, compile=comp), log=lambda *_: None)
        assert tr.mcfg.layer_window(0) == (kw.get("sliding_window") or 32)
        tr.train_loader = _Batches(4, 128, tr.mcfg.vocab_size)
        tr.metrics.log = recs.append
        tr.train()
        torch.cuda.synchronize()
        assert tr.use_graph == comp and (tr.gstep is not None) == comp
        curves[comp] = [r["train_loss"] for r in recs]
        weights[comp] = tr.opt.master.clone()
    assert len(curves[True]) == 4 and all(math.isfinite(v) for v in curves[True])
    for a, b in zip(curves[True], curves[False]):
        assert abs(a - b) < 2e-3 * max(1.0, abs(b)), (curves[True], curves[False])
    rel = ((weights[True] - weights[False]).norm() / weights[False].norm()).item()
    assert rel < 1e-3, rel


# ------------------------------------------------------------------------------------------------ serving
def _swa_model(seed=4):
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(seed)
    return GPT(get_preset("llama-tiny-swa")).to(device=DEV, dtype=torch.bfloat16).eval()


def test_continuous_server_matches_generate():
    """Slots at their own positions, most of them past the window (W = 32 < max_len = 160): one window, one count
    per slot.  Prompt lengths and token counts of tests/test_server_gpu.py."""
    from pretraining_llm_amd.inference.server import ContinuousGenerationServer, GenRequest
    model = _swa_model()
    g = torch.Generator().manual_seed(5)
    reqs = [(torch.randint(0, model.config.vocab_size, (n,), generator=g).tolist(), k)
            for n, k in [(9, 12), (33, 5), (3, 40), (64, 8), (17, 1), (40, 16)]]
    srv = ContinuousGenerationServer(model, max_batch=4, max_len=160)
    try:
        res = [f.result(timeout=120) for f in [srv.submit(GenRequest(p, max_new_tokens=k, temperature=0.0))
                                                for p, k in reqs]]
    finally:
        srv.close()
    for (p, k), r in zip(reqs, res):
        ref = model.generate(torch.tensor([p], device=DEV), max_new_tokens=k, temperature=0.0,
                             cuda_graph=True)[0].tolist()
        assert r.tokens == ref, (len(p), k)


def test_batched_server_matches_generate():
    from pretraining_llm_amd.inference.server import GenerationServer, GenRequest
    model = _swa_model()
    prompts = [[(7 * i + j) % 500 for j in range(40)] for i in range(6)]  # longer than the window
    srv = GenerationServer(model, max_batch=8, max_wait_ms=300.0)
    try:
        futs = [srv.submit(GenRequest(p, max_new_tokens=24, temperature=0.0)) for p in prompts]
        res = [f.result(timeout=120) for f in futs]
    finally:
        srv.close()
    assert all(r.batch_size == 6 for r in res)
    ref = model.generate(torch.tensor(prompts, device=DEV), max_new_tokens=24, temperature=0.0,
                         cuda_graph=True).tolist()
    assert [r.tokens for r in res] == ref


# ------------------------------------------------------------------------------------------------ decode chain
PROMPT, STEPS = 96, 24
# worst step of the dense llama-tiny on the existing path: max(decode_chain_errors(dense)[0]) measured on an MI355X
DENSE_CHAIN_ERR = 4.857e-3
CHAIN_BOUND = 2 * DENSE_CHAIN_ERR


def decode_chain_errors(model, others=()):
    """Prefill ``PROMPT`` tokens, then ``STEPS`` greedy steps replayed from one captured DecodeGraph.  Per step the
    relative Frobenius error of the chain's fp32 last-position logits against ``model(idx)`` (recompute), and
    against each model of ``others`` on the same tokens.  -> [errors vs model, errors vs others[0], ...]"""
    from pretraining_llm_amd.inference.generate import DecodeGraph, KVCache, forward_cached
    cfg = model.config
    B = 2
    idx = torch.randint(0, cfg.vocab_size, (B, PROMPT), generator=torch.Generator().manual_seed(21)).to(DEV)
    cache = KVCache(cfg.n_blocks, B, PROMPT + STEPS, cfg.n_kv_head, cfg.head_dim, torch.bfloat16, DEV)
    graph = DecodeGraph(model, cache, B, DEV)  # before the prefill, which overwrites the warm-up's row 0
    logits = forward_cached(model, idx, cache, 0)
    errs = [[] for _ in range(1 + len(others))]
    with torch.no_grad():
        for _ in range(STEPS):
            nxt = logits.argmax(-1, keepdim=True)
            pos = idx.shape[1]
            idx = torch.cat([idx, nxt], 1)
            logits = graph(nxt, pos).clone()
            for e, mdl in zip(errs, (model,) + tuple(others)):
                e.append(_rel(logits, mdl(idx)[0][:, -1].float()))
    return errs


def _chain_models():
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(12)
    dense = GPT(get_preset("llama-tiny")).to(device=DEV, dtype=torch.bfloat16).eval()
    swa = GPT(dense.config.replace(sliding_window=16)).to(device=DEV, dtype=torch.bfloat16).eval()
    swa.load_state_dict(dense.state_dict())
    return dense, swa


def test_decode_chain_matches_recompute():
    """A captured decode chain of a model whose layers are all local (llama-tiny, W = 16: prompt 96, 24 steps, every
    step far past the window) against ``model(idx)`` at every step, by the relative Frobenius error of the fp32
    last-position logits.  The bound is twice what the dense llama-tiny shows on the existing path for the same
    quantity (measured 4.857e-3 on an MI355X -> 9.71e-3): another split partition and key count move the last bits
    of bf16 activations, nothing more.  Measured for the windowed model: 5.50e-3.  Against a recompute with the window
    off the same quantity must exceed ten times the bound (measured: at least 0.435 at every step)."""
    dense, swa = _chain_models()
    assert all(b.attn.window == 16 for b in swa.attn_blocks)
    own, off = decode_chain_errors(swa, (dense,))
    print(f"decode chain: worst step {max(own):.3e} (bound {CHAIN_BOUND:.3e}); window off: least {min(off):.3e}")
    assert len(own) == STEPS and max(own) < CHAIN_BOUND, own
    assert min(off) > 10 * CHAIN_BOUND, off
