"""Document masking on the GPU: ``ops.attention_packed`` / ``ops.attention_proj`` with bounds against fp32 reference
math, the model with ``doc_mask`` on the HIP path against the reference backend, and the captured (hipGraph) step
replayed on batches whose separators sit elsewhere.  (The kernels themselves: tests/test_attention_seg_gpu.py.)"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEP = 7


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _tokens(B, T, V, seps, seed=0):
    """Random tokens above SEP with separators at the given positions of every row (shifted by 3 per row)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(SEP + 1, V, (B, T), generator=g)
    for b in range(B):
        for s in seps:
            idx[b, (s + 3 * b) % T] = SEP
    return idx.to(DEV)


# ------------------------------------------------------------------------------------------------ attention ops
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("proj", [False, True])
def test_attention_with_bounds_matches_fp32_reference(D, proj):
    """attention_packed / attention_proj with bounds (RoPE on) against ref.rope -> ref.attention(bounds=) in fp32
    under autograd.  Tolerances of tests/test_qk_norm_gpu.py::test_attention_with_gains_matches_fp32_reference:
    output 1.5e-2, dq / dk / dv 3e-2 (relative Frobenius error)."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(43 + D)
    B, T, H, Hkv = 2, 300, 4, 2
    C = H * D
    bounds = ops.doc_bounds(_tokens(B, T, 64, (0, 31, 64, 130, 255, 256)), SEP)
    assert bounds[0].max() > 256 and bounds[0].is_cuda
    qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV) * 0.8).bfloat16().requires_grad_()
    cos, sin = ops.rope_cache(T + 64, D, 10000.0, DEV)
    kw = dict(rope_cos=cos, rope_sin=sin, bounds=bounds)
    if proj:
        w = (torch.randn(C, C, device=DEV) * 0.05).bfloat16().requires_grad_()
        if D == 64:
            assert ops.attn_proj_ok(qkv, H, Hkv, w, None)  # the fused-projection path (delta handed to attn_bwd)
            o = ops.attention_proj(qkv, H, Hkv, w, None, **kw)
        else:
            o = ops.linear(ops.attention_packed(qkv, H, Hkv, **kw), w, None)
    else:
        o = ops.attention_packed(qkv, H, Hkv, **kw)
    do = torch.randn_like(o)
    o.backward(do)
    qkvf = qkv.detach().float().requires_grad_()
    q, k, v = ops._split_qkv(qkvf, H, Hkv, D)
    qr, kr = ref.rope(q, cos[:T], sin[:T]), ref.rope(k, cos[:T], sin[:T])
    of = ref.attention(qr, kr, v, causal=True, scale=1 / math.sqrt(D), bounds=bounds)[0].reshape(B, T, C)
    plain = ref.attention(qr, kr, v, causal=True, scale=1 / math.sqrt(D))[0].reshape(B, T, C)
    assert _rel(plain, of) > 0.3  # the mask matters at this shape
    if proj:
        of = of @ w.detach().float().t()
    of.backward(do.float())
    assert _rel(o, of) < 1.5e-2, _rel(o, of)
    gq, gk, gv = ops._split_qkv(qkv.grad, H, Hkv, D)
    rq, rk, rv = ops._split_qkv(qkvf.grad, H, Hkv, D)
    for a, b, n in ((gq, rq, "q"), (gk, rk, "k"), (gv, rv, "v")):
        assert _rel(a, b) < 3e-2, (n, _rel(a, b))


def test_stock_sdpa_branch_builds_the_mask():
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(2)
    B, T, H, Hkv, D = 2, 96, 4, 2, 64
    bounds = ops.doc_bounds(_tokens(B, T, 64, (10, 40)), SEP)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV)
    with ops.backend("torch"):
        o = ops.attention_packed(qkv, H, Hkv, bounds=bounds)
    q, k, v = ops._split_qkv(qkv, H, Hkv, D)
    of = ref.attention(q, k, v, causal=True, scale=1 / math.sqrt(D), bounds=bounds)[0].reshape(B, T, H * D)
    assert _rel(o, of) < 1e-3, _rel(o, of)


# ------------------------------------------------------------------------------------------------ model
@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_model_hip_matches_reference_backend(name):
    """Loss and every parameter gradient on the HIP path against the stock-torch backend from the same weights;
    tolerances of tests/test_qk_norm_gpu.py::test_model_hip_matches_reference_backend (loss 2e-2, gradients 6e-2)."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(10)
    cfg = get_preset(name).replace(context_length=128, doc_mask=True, doc_sep_token=SEP)
    m = GPT(cfg).to(DEV, torch.bfloat16)
    x = _tokens(2, 128, cfg.vocab_size, (5, 31, 64, 100))
    y = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    _, l1 = m(x, y, return_logits=False)
    l1.backward()
    g1 = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    m.zero_grad()
    with ops.backend("torch"):
        _, l2 = m(x, y)
        l2.backward()
        g2 = {n: p.grad.float().clone() for n, p in m.named_parameters()}
        m.zero_grad()
        _, l3 = m(x, y, doc_mask=False)
        l3.backward()
    assert abs(l1.item() - l2.item()) < 2e-2
    for n, p in m.named_parameters():
        assert _rel(g1[n], g2[n]) < 6e-2, (n, _rel(g1[n], g2[n]))
    # the mask is in force: the first block's value projection sees another gradient without it
    n = "attn_blocks.0.attn.qkv.weight"
    assert _rel(dict(m.named_parameters())[n].grad, g2[n]) > 0.2


def test_bounds_follow_the_batch_in_a_captured_graph():
    """doc_bounds + attention forward / backward captured once in a hipGraph: replayed on tokens whose separators
    sit elsewhere, the outputs are bit-equal to the eager call on those tokens (and differ from the capture's)."""
    from pretraining_llm_amd import ops
    torch.manual_seed(3)
    B, T, H, Hkv, D = 2, 300, 4, 2, 64
    qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV) * 0.8).bfloat16().requires_grad_()
    do = torch.randn(B, T, H * D, device=DEV).bfloat16()
    idx_a, idx_b = _tokens(B, T, 64, (31, 200), seed=1), _tokens(B, T, 64, (64, 130, 256), seed=2)

    def run(idx):
        o = ops.attention_packed(qkv, H, Hkv, bounds=ops.doc_bounds(idx, SEP))
        (g,) = torch.autograd.grad(o, qkv, do)
        return o.detach(), g

    want_a, want_b = run(idx_a), run(idx_b)
    assert not torch.equal(want_a[0], want_b[0])
    static = idx_a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static)
    for idx, want in ((idx_b, want_b), (idx_a, want_a)):
        static.copy_(idx)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


class _Batches:
    """A stand-in for the trainer's loader: fixed batches whose separators move from step to step."""

    def __init__(self, B, T, V):
        self.B, self.T, self.V, self.i = B, T, V, 0

    def next(self):
        i, self.i = self.i, self.i + 1
        x = _tokens(self.B, self.T, self.V, ((11 + 17 * i) % self.T, (70 + 29 * i) % self.T), seed=100 + i)
        y = torch.roll(x, -1, 1)
        return x, y


@pytest.mark.parametrize("name", ["llama-tiny", "gpt2-tiny"])
def test_trainer_captured_step(name, tmp_path, monkeypatch):
    """Trainer steps with the captured (hipGraph) step (one eager warm-up step, then replays on batches whose
    separators sit elsewhere) against the eager step from the same seed and batches: the loss curves agree within
    the 2e-3 of tests/test_compile_gpu.py's graph-against-eager tests and the weights within its 1e-3."""
    from config.config import default_config
    from pretraining_llm_amd.train.trainer import Trainer
    monkeypatch.delenv("TORCH_COMPILE", raising=False)
    base = dict(default_config)
    base.update(model_preset=name, t_batch_size=4, seq_len=128, t_train_steps=4, t_lr=1e-3, warmup_steps=1,
                log_interval=1, t_eval_steps=1000, eval_at_start=False, t_out_path=None, synthetic_data=True,
                synthetic_tokens=200_000, synthetic_dir=str(tmp_path), max_grad_norm=1.0, device="cuda",
                doc_mask=True, doc_sep_token=SEP)
    curves, weights = {}, {}
    for comp in (True, False):
        recs = []
        tr = Trainer(dict(base, compile=comp), log=lambda *_: None)
        assert tr.mcfg.doc_mask and tr.mcfg.doc_sep_token == SEP
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
