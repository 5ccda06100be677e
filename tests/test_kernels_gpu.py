"""Numerics of every gfx950 HIP kernel against a plain PyTorch fp32 reference of the same op.

All tests here need the MI355X and the in-tree extension (``pretraining_llm_amd/_C.so``);
they fail loudly if the extension is missing (no silent fallback)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _ops():
    return torch.ops.pllm


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ----------------------------------------------------------------- norms
@pytest.mark.parametrize("C", [128, 768, 1024, 2048])
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_norm_fwd_bwd(C, rms, with_res):
    from pretraining_llm_amd import ops
    torch.manual_seed(0)
    N = 517
    x = torch.randn(N, C, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    r = torch.randn(N, C, device=DEV, dtype=torch.bfloat16, requires_grad=True) if with_res else None
    w = (1 + 0.1 * torch.randn(C, device=DEV)).bfloat16().requires_grad_()
    b = None if rms else (0.1 * torch.randn(C, device=DEV)).bfloat16().requires_grad_()
    fn = ops.rms_norm if rms else ops.layer_norm
    if rms:
        y, s = fn(x, w, 1e-5, r)
    else:
        y, s = fn(x, w, b, 1e-5, r)
    dy = torch.randn_like(y)
    ds = torch.randn_like(s) if with_res else None
    outs = [y] + ([s] if with_res else [])
    grads = [dy] + ([ds] if with_res else [])
    torch.autograd.backward(outs, grads)
    # fp32 reference
    xf = x.detach().float().requires_grad_()
    rf = r.detach().float().requires_grad_() if with_res else None
    wf = w.detach().float().requires_grad_()
    bf = b.detach().float().requires_grad_() if b is not None else None
    sf = xf + rf if with_res else xf
    sq = sf.to(torch.bfloat16).float() if with_res else sf  # kernel normalises the bf16-rounded sum
    if rms:
        yf = sq * torch.rsqrt(sq.pow(2).mean(-1, keepdim=True) + 1e-5) * wf
    else:
        yf = F.layer_norm(sq, (C,), wf, bf, 1e-5)
    of = [yf] + ([sf] if with_res else [])
    torch.autograd.backward(of, [g.float() for g in grads])
    assert _rel(y, yf) < 1e-2
    assert _rel(x.grad, xf.grad) < 2e-2
    assert _rel(w.grad, wf.grad) < 2e-2
    if b is not None:
        assert _rel(b.grad, bf.grad) < 2e-2
    if with_res:
        assert _rel(s, sf) < 1e-2
        assert _rel(r.grad, rf.grad) < 2e-2


@pytest.mark.parametrize("C", [768, 1024])
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_norm_fwd_prefetch_path(C, rms, with_res):
    """>= 32768 rows of <= 1024 elements take the persistent two-row-prefetch forward; a ragged row count checks
    the clamped tail loads and the odd last row of each wave."""
    from pretraining_llm_amd import ops
    torch.manual_seed(1)
    N = 40001
    x = torch.randn(N, C, device=DEV, dtype=torch.bfloat16)
    r = torch.randn(N, C, device=DEV, dtype=torch.bfloat16) if with_res else None
    w = (1 + 0.1 * torch.randn(C, device=DEV)).bfloat16()
    b = None if rms else (0.1 * torch.randn(C, device=DEV)).bfloat16()
    with torch.no_grad():
        y, s = ops.rms_norm(x, w, 1e-5, r) if rms else ops.layer_norm(x, w, b, 1e-5, r)
    sq = (x.float() + r.float()).bfloat16().float() if with_res else x.float()
    if rms:
        yf = sq * torch.rsqrt(sq.pow(2).mean(-1, keepdim=True) + 1e-5) * w.float()
    else:
        yf = F.layer_norm(sq, (C,), w.float(), b.float(), 1e-5)
    assert _rel(y, yf) < 1e-2
    # every row written (a skipped row would leave garbage / zeros far from the reference)
    assert ((y.float() - yf).abs().amax(-1) < 0.1).all()
    if with_res:
        assert torch.equal(s, sq.bfloat16())


# ----------------------------------------------------------------- activations
@pytest.mark.parametrize("kind", ["gelu", "relu"])
def test_activation(kind):
    from pretraining_llm_amd import ops
    torch.manual_seed(1)
    x = torch.randn(333, 3072, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y = getattr(ops, kind)(x)
    dy = torch.randn_like(y)
    y.backward(dy)
    xf = x.detach().float().requires_grad_()
    yf = F.gelu(xf, approximate="tanh") if kind == "gelu" else torch.relu(xf)
    yf.backward(dy.float())
    assert _rel(y, yf) < 1e-2
    assert _rel(x.grad, xf.grad) < 1e-2


def test_swiglu():
    from pretraining_llm_amd import ops
    torch.manual_seed(2)
    gu = torch.randn(129, 2 * 688, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y = ops.swiglu(gu)
    dy = torch.randn_like(y)
    y.backward(dy)
    gf = gu.detach().float().requires_grad_()
    g, u = gf.chunk(2, -1)
    yf = F.silu(g) * u
    yf.backward(dy.float())
    assert _rel(y, yf) < 1e-2
    assert _rel(gu.grad, gf.grad) < 1e-2


def test_rope_packed_roundtrip():
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(3)
    B, T, H, Hkv, D = 2, 64, 4, 2, 128
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    cos, sin = ops.rope_cache(T, D, 10000.0, DEV)
    out = ops.rope_packed(qkv, cos, sin, H, Hkv)
    q, k, v = ops._split_qkv(qkv.detach().float(), H, Hkv, D)
    qr, kr = ref.rope(q, cos, sin), ref.rope(k, cos, sin)
    exp = torch.cat([qr.reshape(B, T, -1), kr.reshape(B, T, -1), v.reshape(B, T, -1)], -1)
    assert _rel(out, exp) < 1e-2
    g = torch.randn_like(out)
    out.backward(g)
    qkvf = qkv.detach().float().requires_grad_()
    q2, k2, v2 = ops._split_qkv(qkvf, H, Hkv, D)
    e2 = torch.cat([ref.rope(q2, cos, sin).reshape(B, T, -1), ref.rope(k2, cos, sin).reshape(B, T, -1),
                    v2.reshape(B, T, -1)], -1)
    e2.backward(g.float())
    assert _rel(qkv.grad, qkvf.grad) < 1e-2


# ----------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("V", [50304, 32000, 512])
def test_cross_entropy_fused(V):
    from pretraining_llm_amd import ops
    torch.manual_seed(4)
    N, C = 300, 256
    h = (torch.randn(N, C, device=DEV) * 0.5).bfloat16().requires_grad_()
    W = (torch.randn(V, C, device=DEV) * 0.05).bfloat16().requires_grad_()
    t = torch.randint(0, V, (N,), device=DEV)
    t[::7] = -100
    loss = ops.lm_head_cross_entropy(h, W, None, t)
    loss.backward()
    hf, Wf = h.detach().float().requires_grad_(), W.detach().float().requires_grad_()
    logits = (hf @ Wf.t()).bfloat16().float()
    lf = F.cross_entropy(logits, t, ignore_index=-100)
    lf.backward()
    assert abs(loss.item() - lf.item()) < 2e-3 * max(1.0, lf.item())
    assert _rel(h.grad, hf.grad) < 3e-2
    assert _rel(W.grad, Wf.grad) < 3e-2
    # forward-only path
    with torch.no_grad():
        l2 = ops.cross_entropy(logits.bfloat16(), t)
    assert abs(l2.item() - lf.item()) < 2e-3 * max(1.0, lf.item())


# ----------------------------------------------------------------- embedding
@pytest.mark.parametrize("with_pos", [True, False])
def test_embedding(with_pos):
    from pretraining_llm_amd import ops
    torch.manual_seed(5)
    V, C, B, T = 1000, 256, 4, 96
    wte = torch.randn(V, C, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    wpe = torch.randn(T, C, device=DEV, dtype=torch.bfloat16, requires_grad=True) if with_pos else None
    idx = torch.randint(0, 50, (B, T), device=DEV)  # many repeats -> exercises the segmented sum
    x = ops.embedding(idx, wte, wpe)
    dx = torch.randn_like(x)
    x.backward(dx)
    wtef = wte.detach().float().requires_grad_()
    wpef = wpe.detach().float().requires_grad_() if with_pos else None
    xf = F.embedding(idx, wtef) + (wpef[:T] if with_pos else 0)
    xf.backward(dx.float())
    assert _rel(x, xf) < 1e-2
    assert _rel(wte.grad, wtef.grad) < 1e-2
    if with_pos:
        assert _rel(wpe.grad, wpef.grad) < 1e-2
    # determinism: same inputs, same bits
    wte.grad = None
    x2 = ops.embedding(idx, wte, wpe)
    x2.backward(dx)
    g1 = wte.grad.clone()
    wte.grad = None
    x3 = ops.embedding(idx, wte, wpe)
    x3.backward(dx)
    assert torch.equal(g1, wte.grad)


@pytest.mark.parametrize("kind", ["zipf", "boundary_runs", "single_id"])
def test_embedding_bwd_skewed_ids(kind):
    """Skewed token distributions (Zipf as in real text, runs of exactly chunk-sized / chunk-crossing
    lengths, one id everywhere): the chunked two-phase backward matches an fp64 index_add, into
    fp32 and bf16 gradient targets, and is bitwise reproducible."""
    torch.manual_seed(11)
    V, C, B, T = 5000, 768, 8, 1024
    N = B * T
    if kind == "zipf":
        z = torch.distributions.Pareto(1.0, 1.0).sample((N,)).floor().long() - 1
        idx = (z.clamp_max(V - 1) * 7919 % V).view(B, T).to(DEV)
    elif kind == "boundary_runs":
        lens = [64, 128, 1, 63, 65, 127, 129, 2, 191, 64 * 5 + 3]
        ids, i = [], 0
        while len(ids) < N:
            ids += [i % V] * lens[i % len(lens)]
            i += 1
        idx = torch.tensor(ids[:N])[torch.randperm(N)].view(B, T).to(DEV)
    else:
        idx = torch.full((B, T), 17, device=DEV)
    dx = torch.randn(B, T, C, device=DEV).bfloat16()
    ref = torch.zeros(V, C, dtype=torch.float64, device=DEV).index_add_(0, idx.view(-1), dx.view(N, C).double())
    g32 = torch.randn(V, C, device=DEV)
    base = g32.double().clone()
    torch.ops.pllm.embedding_bwd_acc(dx, idx, V, 0, False, g32)
    assert _rel(g32.double() - base, ref) < 1e-5, _rel(g32.double() - base, ref)
    g32b = base.float().clone()
    torch.ops.pllm.embedding_bwd_acc(dx, idx, V, 0, False, g32b)
    assert torch.equal(g32, g32b)
    gb, _ = torch.ops.pllm.embedding_bwd(dx, idx, V, 0, False)
    assert _rel(gb.double(), ref) < 1e-2


# ----------------------------------------------------------------- AdamW
def test_adamw_flat_matches_torch():
    torch.manual_seed(6)
    n = 4096 + 64
    p32 = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV).bfloat16()
    ref_p = p32.clone().requires_grad_()
    opt = torch.optim.AdamW([ref_p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    master, m, v = p32.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb = p32.bfloat16()
    for step in range(1, 4):
        ref_p.grad = g.float() * 0.5
        opt.step()
        torch.ops.pllm.adamw_(pb, master, m, v, g, 1e-2, 0.9, 0.999, 1e-8, 0.01, step, 0.5, None, None)
    torch.cuda.synchronize()
    assert _rel(master, ref_p.detach()) < 1e-5
    assert _rel(pb, ref_p.detach()) < 1e-2


def test_sumsq():
    x = torch.randn(1 << 20, device=DEV).bfloat16()
    s = torch.ops.pllm.sumsq(x)
    assert abs(s.item() - x.float().pow(2).sum().item()) / x.float().pow(2).sum().item() < 1e-4


# ----------------------------------------------------------------- attention
def _attn_ref(q, k, v, causal, scale):
    B, T, H, D = q.shape
    S, Hkv = k.shape[1], k.shape[2]
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    if Hkv != H:
        kf = kf.repeat_interleave(H // Hkv, 1)
        vf = vf.repeat_interleave(H // Hkv, 1)
    s = qf @ kf.transpose(-1, -2) * scale
    if causal:
        mask = torch.ones(T, S, dtype=torch.bool, device=q.device).tril(S - T)
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, -1)
    return (p @ vf).transpose(1, 2), torch.logsumexp(s, -1)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [128, 200, 1024])
@pytest.mark.parametrize("causal", [True, False])
def test_attention_fwd(D, T, causal):
    torch.manual_seed(7)
    B, H = 2, 4
    q = torch.randn(B, T, H, D, device=DEV, dtype=torch.bfloat16)
    k = torch.randn(B, T, H, D, device=DEV, dtype=torch.bfloat16)
    v = torch.randn(B, T, H, D, device=DEV, dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    o, lse = torch.ops.pllm.attn_fwd(q, k, v, causal, scale)
    oref, lref = _attn_ref(q, k, v, causal, scale)
    assert _rel(o, oref) < 1e-2, _rel(o, oref)
    assert (lse - lref).abs().max().item() < 2e-2


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_attention_fwd_lazy_max_rescale_branch(D, causal):
    """The forward moves its running max lazily (only past a 2^8 threshold): force the rescale
    branch -- scores of large dynamic range (x6) so row maxima grow by more than the threshold at
    later tiles, plus spikes: one key per head aligned with one query at a chosen late tile so the
    max jumps far (guide §5.4 rule 26) -- and check the FULL output against fp32."""
    torch.manual_seed(11)
    B, H, T = 2, 4, 640
    q = torch.randn(B, T, H, D, device=DEV) * 2.5
    k = torch.randn(B, T, H, D, device=DEV) * 2.5
    v = torch.randn(B, T, H, D, device=DEV)
    # spike: key 450 of head 0 (tile 7) matches query 500 strongly; key 130 of head 1 matches
    # query 600 (an early tile jumping late rows' max only after many tiles were accumulated)
    k[:, 450, 0] = q[:, 500, 0] * 3.0
    k[:, 130, 1] = q[:, 600, 1] * 3.0
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    scale = 1 / math.sqrt(D)
    o, lse = torch.ops.pllm.attn_fwd(q, k, v, causal, scale)
    oref, lref = _attn_ref(q, k, v, causal, scale)
    assert _rel(o, oref) < 1.5e-2, _rel(o, oref)
    assert (o.float() - oref).abs().max().item() < 0.1
    assert ((lse - lref).abs() / lref.abs().clamp_min(1.0)).max().item() < 1e-2


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [128, 192, 512])
@pytest.mark.parametrize("gqa", [1, 2])
def test_attention_packed_fwd_bwd(D, T, gqa):
    from pretraining_llm_amd import ops
    torch.manual_seed(8)
    B, H = 2, 4
    Hkv = H // gqa
    qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV) * 0.7).bfloat16().requires_grad_()
    o = ops.attention_packed(qkv, H, Hkv, causal=True)
    do = torch.randn_like(o)
    o.backward(do)
    qkvf = qkv.detach().float().requires_grad_()
    q, k, v = ops._split_qkv(qkvf, H, Hkv, D)
    of, _ = _attn_ref(q, k, v, True, 1 / math.sqrt(D))
    of = of.reshape(B, T, H * D)
    of.backward(do.float())
    assert _rel(o, of) < 1e-2
    assert _rel(qkv.grad, qkvf.grad) < 2.5e-2, _rel(qkv.grad, qkvf.grad)
    # per-part check so a wrong dq/dk/dv cannot hide in the packed norm
    gq, gk, gv = ops._split_qkv(qkv.grad, H, Hkv, D)
    rq, rk, rv = ops._split_qkv(qkvf.grad, H, Hkv, D)
    for a, b in ((gq, rq), (gk, rk), (gv, rv)):
        assert _rel(a, b) < 3e-2


def test_attention_decode_alignment():
    """T < S (KV-cache decode): queries aligned to the end of the keys."""
    torch.manual_seed(9)
    B, H, D, S = 2, 4, 64, 300
    q = torch.randn(B, 1, H, D, device=DEV, dtype=torch.bfloat16)
    k = torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    v = torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    o, _ = torch.ops.pllm.attn_fwd(q, k, v, True, 1 / math.sqrt(D))
    oref, _ = _attn_ref(q, k, v, True, 1 / math.sqrt(D))
    assert _rel(o, oref) < 1e-2


# ----------------------------------------------------------------- whole model
@pytest.mark.parametrize("D,H,Hkv,B,S", [(64, 12, 12, 1, 1000), (64, 12, 12, 8, 37), (128, 16, 4, 2, 2049),
                                          (32, 4, 4, 3, 64), (128, 8, 1, 4, 517), (64, 4, 2, 1, 1)])
def test_attention_decode_kernel(D, H, Hkv, B, S):
    """Split-KV decode kernel vs the fp32 reference, on a strided cache view [:, :S] of a
    larger [B, S_max, Hkv, D] buffer, with and without the device-side key count."""
    from pretraining_llm_amd import ops
    torch.manual_seed(S)
    kc = torch.randn(B, S + 40, Hkv, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(B, S + 40, Hkv, D, device="cuda", dtype=torch.bfloat16)
    q = torch.randn(B, 1, H, D, device="cuda", dtype=torch.bfloat16)
    k, v = kc[:, :S], vc[:, :S]
    ref_o, _ = _attn_ref(q, k, v, False, 1.0 / math.sqrt(D))
    o = _ops().attn_decode(q, k, v, 1.0 / math.sqrt(D))
    assert o.shape == (B, 1, H, D)
    assert _rel(o, ref_o) < 1e-2
    # the dispatcher routes one-query attention to the same kernel
    assert _rel(ops.attention(q, k, v, causal=True), ref_o) < 1e-2
    # device key count over the whole cache buffer == host slicing
    n = torch.tensor([S], dtype=torch.int32, device="cuda")
    o2 = ops.attention_decode(q, kc, vc, seqlen=n)
    assert torch.equal(o2, o) or _rel(o2, ref_o) < 1e-2


@pytest.mark.parametrize("M", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("N,K", [(777, 768), (2000, 512), (3072, 768), (768, 3072), (9000, 256), (50304, 768)])
def test_gemv_skinny_gemm(M, N, K):
    """Decode-sized projection kernel (csrc/gemv.hip) vs fp32 torch, with and without bias,
    on a row-strided x view; ops.linear routes <= 8-row inference calls to it."""
    from pretraining_llm_amd import ops
    torch.manual_seed(M * 7 + N)
    xb = torch.randn(M, 2 * K, device=DEV, dtype=torch.bfloat16)
    x = xb[:, :K]
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) * K ** -0.5
    b = torch.randn(N, device=DEV, dtype=torch.bfloat16)
    ref = x.float() @ w.float().t()
    assert _rel(_ops().gemv(x, w, None)[0], ref) < 5e-3
    assert _rel(_ops().gemv(x, w, b)[0], ref + b.float()) < 5e-3
    with torch.no_grad():
        assert _rel(ops.linear(x.reshape(1, M, K), w, b).reshape(M, N), ref + b.float()) < 5e-3


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("rms", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("N,K", [(2304, 768), (9000, 512)])
def test_gemv_norm_prologue_act_epilogue(M, rms, with_res, act, N, K):
    """Decode fusion (csrc/gemv.hip): act(norm(x + res) W^T + b) and the residual stream x + res
    from one launch vs fp32 torch (LayerNorm / RMSNorm, GELU-tanh / ReLU)."""
    torch.manual_seed(M + 10 * rms + 100 * act + N)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16) * 2 + 0.5
    r = torch.randn(M, K, device=DEV, dtype=torch.bfloat16) if with_res else None
    g = (1 + 0.1 * torch.randn(K, device=DEV)).bfloat16()
    be = None if rms else (0.1 * torch.randn(K, device=DEV)).bfloat16()
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) * K ** -0.5
    b = torch.randn(N, device=DEV, dtype=torch.bfloat16)
    out = _ops().gemv(x, w, b, r, g, be, 1e-5, rms, act)
    s = x.float() + r.float() if with_res else x.float()
    if with_res:
        assert _rel(out[1], s) < 5e-3
    else:
        assert out[1].numel() == 0
    if rms:
        h = s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + 1e-5) * g.float()
    else:
        h = torch.nn.functional.layer_norm(s, (K,), g.float(), be.float(), 1e-5)
    ref = h @ w.float().t() + b.float()
    if act == 1:
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    elif act == 2:
        ref = torch.relu(ref)
    assert _rel(out[0], ref) < 1e-2


def test_gemv_kv_cache_append():
    """QKV decode projection appends its K/V columns to the caches at the device position;
    other cache rows stay untouched and an out-of-range position writes nothing."""
    torch.manual_seed(3)
    B, S, Hkv, D, H, K = 3, 16, 2, 64, 4, 256
    N = (H + 2 * Hkv) * D
    x = torch.randn(B, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) * K ** -0.5
    g = torch.ones(K, device=DEV, dtype=torch.bfloat16)
    kc = torch.zeros(B, S, Hkv, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    pos = torch.tensor([5], device=DEV)
    y = _ops().gemv(x, w, None, None, g, None, 1e-5, 1, 0, kc, vc, pos, H * D)[0]
    assert torch.equal(kc[:, 5].reshape(B, -1), y[:, H * D:(H + Hkv) * D])
    assert torch.equal(vc[:, 5].reshape(B, -1), y[:, (H + Hkv) * D:])
    kc[:, 5] = 0
    vc[:, 5] = 0
    assert not kc.any() and not vc.any()
    _ops().gemv(x, w, None, None, g, None, 1e-5, 1, 0, kc, vc, torch.tensor([S], device=DEV), H * D)
    torch.cuda.synchronize()
    assert not kc.any() and not vc.any()


@pytest.mark.parametrize("preset", ["gpt2-tiny", "llama-tiny", "ref-small"])
def test_fused_decode_step_matches_full_forward(preset):
    """KV-cache decode step (fused norm->projection->activation skinny GEMMs) == the last-position
    logits of a full, uncached training-path forward."""
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached, forward_decode
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(5)
    cfg = get_preset(preset).replace(vocab_size=512, context_length=64)
    if preset == "ref-small":  # reference architecture (ReLU, no W_o, biased untied head), tiny dims
        cfg = cfg.replace(n_embed=128, n_head=4, n_kv_head=4, n_blocks=2, ffn_hidden=512)
    m = GPT(cfg).to(DEV, torch.bfloat16).eval()
    idx = torch.randint(0, 512, (2, 20), device=DEV)
    with torch.no_grad():
        full, _ = m(idx)
        cache = KVCache(cfg.n_blocks, 2, 64, cfg.n_kv_head, cfg.head_dim, torch.bfloat16, idx.device)
        pre = forward_cached(m, idx[:, :-1], cache, 0)
        pos_t = torch.tensor([19], device=DEV)
        dec = forward_decode(m, idx[:, -1:], cache, pos_t, (pos_t + 1).int())
    assert _rel(pre, full[:, -2].float()) < 3e-2
    assert _rel(dec, full[:, -1].float()) < 3e-2


@pytest.mark.parametrize("preset", ["gpt2-tiny", "llama-tiny"])
def test_graphed_decode_matches_eager(preset):
    """generate(cuda_graph=True) (one hipGraph replay per token, device-side position and
    key count) == eager KV-cache decoding, greedy."""
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(11)
    cfg = get_preset(preset).replace(vocab_size=512, context_length=96)
    m = GPT(cfg).to(DEV, torch.bfloat16).eval()
    idx = torch.randint(0, 512, (3, 9), device=DEV)
    a = m.generate(idx, 40, temperature=0.0, cuda_graph=False)
    b = m.generate(idx, 40, temperature=0.0, cuda_graph=True)
    assert torch.equal(a, b)


def test_model_hip_matches_reference_path():
    """One GPT-2-tiny forward/backward on the HIP kernels vs the same model on stock torch ops."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(10)
    cfg = get_preset("gpt2-tiny").replace(context_length=128)
    m = GPT(cfg).to(DEV, torch.bfloat16)
    x = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    y = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    _, l1 = m(x, y, return_logits=False)
    l1.backward()
    g1 = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    m.zero_grad()
    with ops.backend("torch"):
        _, l2 = m(x, y)
        l2.backward()
    assert abs(l1.item() - l2.item()) < 2e-2
    for n, p in m.named_parameters():
        assert _rel(g1[n], p.grad) < 6e-2, n


@pytest.mark.parametrize("preset", ["gpt2-tiny", "llama-tiny", "ref-small"])
def test_model_direct_grad_accumulation_matches_reference(preset):
    """With FlatAdamW the HIP backward adds weight/bias gradients straight into the flat buffer
    (beta=1 GEMMs, fused bias grads in norm/activation kernels); compare against the stock
    torch path accumulating through autograd into the same buffer."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT, get_preset
    from pretraining_llm_amd.train.optim import FlatAdamW
    torch.manual_seed(11)
    cfg = get_preset(preset).replace(context_length=128, vocab_size=1024)
    if preset == "ref-small":
        cfg = cfg.replace(n_blocks=2, n_embed=256, n_head=4)
    m = GPT(cfg).to(DEV, torch.bfloat16)
    opt = FlatAdamW(m, lr=1e-3)
    x = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    y = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    for _ in range(2):  # twice: the second pass accumulates on top of the first
        _, l1 = m(x, y, return_logits=False)
        l1.backward()
    g_hip = opt.flat_grad.float().clone()
    opt.zero_grad()
    with ops.backend("torch"):
        for _ in range(2):
            _, l2 = m(x, y)
            l2.backward()
    g_ref = opt.flat_grad.float().clone()
    assert abs(l1.item() - l2.item()) < 2e-2
    for i, (n, p) in enumerate(zip(opt.names, opt.params)):
        a, b = opt.grad_view(i).float(), None
        o = opt.offsets[i]
        a = g_hip[o:o + p.numel()]
        b = g_ref[o:o + p.numel()]
        assert _rel(a, b) < 6e-2, (n, _rel(a, b))


def test_bias_grad_kernels():
    torch.manual_seed(12)
    dy = torch.randn(3000, 2304, device=DEV).bfloat16()
    g = torch.ops.pllm.bias_grad(dy)
    assert _rel(g, dy.float().sum(0)) < 5e-3
    acc = torch.randn(2304, device=DEV).bfloat16()
    ref = acc.float() + dy.float().sum(0)
    torch.ops.pllm.bias_grad(dy, acc)
    assert _rel(acc, ref) < 5e-3
    x = torch.randn(3000, 3072, device=DEV).bfloat16()
    d = torch.randn(3000, 3072, device=DEV).bfloat16()
    b = torch.zeros(3072, device=DEV).bfloat16()
    dx = torch.ops.pllm.act_bwd_bias(d, x, 1, b)
    xf = x.float().requires_grad_()
    torch.nn.functional.gelu(xf, approximate="tanh").backward(d.float())
    assert _rel(dx, xf.grad) < 1e-2
    assert _rel(b, xf.grad.sum(0)) < 1e-2
    # fp32 targets: sums of the bf16 values added in fp32
    acc32 = torch.randn(2304, device=DEV)
    ref32 = acc32.double() + dy.double().sum(0)
    torch.ops.pllm.bias_grad(dy, acc32)
    assert _rel(acc32.double(), ref32) < 1e-6
    b32 = torch.zeros(3072, device=DEV)
    dx2 = torch.ops.pllm.act_bwd_bias(d, x, 1, b32)
    assert torch.equal(dx2, dx)
    assert _rel(b32.double(), dx.double().sum(0)) < 1e-6


# (2048, 200, 136): tiles past P and Q; (4096, 768, 768) / (2048, 512, 2304): split-K slab path;
# (1024, 4096, 4096): 256 tiles -> single slice, accumulated in the kernel epilogue
@pytest.mark.parametrize("M,P,Q", [(2048, 200, 136), (4096, 768, 768), (2048, 512, 2304), (1024, 4096, 4096),
                                   (640, 1024, 256)])
def test_wgrad_kernel(M, P, Q):
    torch.manual_seed(13)
    dy = (torch.randn(M, P, device=DEV) * 0.3).bfloat16()
    x = torch.randn(M, Q, device=DEV).bfloat16()
    ref = dy.float().t() @ x.float()
    out = torch.ops.pllm.wgrad(dy, x)
    assert _rel(out, ref) < 5e-3, _rel(out, ref)
    assert torch.equal(out, torch.ops.pllm.wgrad(dy, x))  # deterministic across calls
    acc = torch.randn(P, Q, device=DEV).bfloat16()
    ref2 = acc.float() + ref
    torch.ops.pllm.wgrad(dy, x, acc)
    assert _rel(acc, ref2) < 5e-3
    # fp32 gradient target (FlatAdamW's default): accumulated in fp32, error at fp32 level
    acc32 = torch.randn(P, Q, device=DEV)
    ref3 = acc32.double() + dy.double().t() @ x.double()
    torch.ops.pllm.wgrad(dy, x, acc32)
    assert _rel(acc32.double(), ref3) < 1e-5, _rel(acc32.double(), ref3)
    # the one-barrier kernel (csrc/gemm_wgrad.hip) with either MFMA shape computes the same product
    try:
        for variant in (16, 32):
            torch.ops.pllm.wgrad_set_mfma(variant)
            assert _rel(torch.ops.pllm.wgrad(dy, x), ref) < 5e-3, variant
            acc32 = torch.randn(P, Q, device=DEV)
            ref3 = acc32.double() + dy.double().t() @ x.double()
            torch.ops.pllm.wgrad(dy, x, acc32)
            assert _rel(acc32.double(), ref3) < 1e-5, (variant, _rel(acc32.double(), ref3))
    finally:
        torch.ops.pllm.wgrad_set_mfma(0)
    # strided (non-contiguous rows) operands, e.g. a column slice of a packed buffer
    big = torch.randn(M, P + 64, device=DEV).bfloat16()
    v = big[:, 32:32 + P]
    out3 = torch.ops.pllm.wgrad(v, x)
    assert _rel(out3, v.float().t() @ x.float()) < 5e-3
    with pytest.raises(RuntimeError):
        torch.ops.pllm.wgrad(dy[:M - 8], x[:M - 8])  # token count must be a multiple of 64


@pytest.mark.parametrize("M,P,Q", [(2048, 200, 136), (4096, 768, 768), (2048, 512, 2304), (1024, 4096, 4096),
                                   (8192, 2304, 768)])
@pytest.mark.parametrize("bias_f32", [True, False])
def test_wgrad_fused_bias_grad(M, P, Q, bias_f32):
    """wgrad(..., bias_acc): the bias gradient (column sums of dy) added inside the weight-gradient GEMM
    (all-ones MFMAs; split-K partial rows summed in slice order) or, on the 32x32x16 kernel, by the
    bias_grad kernels -- against fp64 sums; the weight gradient itself is unchanged."""
    torch.manual_seed(17)
    dy = (torch.randn(M, P, device=DEV) * 0.3).bfloat16()
    x = torch.randn(M, Q, device=DEV).bfloat16()
    w0 = torch.randn(P, Q, device=DEV)
    try:
        for variant in (0, 16, 32):
            torch.ops.pllm.wgrad_set_mfma(variant)
            b0 = torch.randn(P, device=DEV)
            b0 = b0 if bias_f32 else b0.bfloat16()
            acc, bacc = w0.clone(), b0.clone()
            torch.ops.pllm.wgrad(dy, x, acc, bacc)
            ref_b = b0.double() + dy.double().sum(0)
            tol = 1e-6 if bias_f32 else 1e-2
            assert _rel(bacc.double(), ref_b) < tol, (variant, _rel(bacc.double(), ref_b))
            acc2 = w0.clone()
            torch.ops.pllm.wgrad(dy, x, acc2)
            assert torch.equal(acc, acc2), variant  # the GEMM result does not change
            bacc2 = b0.clone()
            torch.ops.pllm.wgrad(dy, x, w0.clone(), bacc2)
            assert torch.equal(bacc, bacc2), variant  # deterministic
    finally:
        torch.ops.pllm.wgrad_set_mfma(0)
    with pytest.raises(RuntimeError):
        torch.ops.pllm.wgrad(dy, x, None, torch.zeros(P, device=DEV))  # bias_acc needs out_acc


def test_graphed_train_step_matches_eager():
    """A hipGraph-captured step (fwd, bwd, clip, AdamW, zero_grad) reproduces eager steps."""
    from pretraining_llm_amd.models import GPT, get_preset
    from pretraining_llm_amd.parallel.dp import DataParallelEngine
    from pretraining_llm_amd.train.graph import GraphedTrainStep
    from pretraining_llm_amd.train.optim import FlatAdamW
    cfg = get_preset("gpt2-tiny").replace(context_length=128, vocab_size=1024, n_head=2)
    xs = [torch.randint(0, 1024, (4, 128), device=DEV) for _ in range(6)]
    ys = [torch.randint(0, 1024, (4, 128), device=DEV) for _ in range(6)]

    def make():
        torch.manual_seed(14)
        m = GPT(cfg).to(DEV, torch.bfloat16)
        o = FlatAdamW(m, lr=1e-3, max_grad_norm=1.0)
        return m, o, DataParallelEngine(o)

    m1, o1, e1 = make()
    eager = []
    for i in range(6):
        _, loss = m1(xs[i], ys[i], return_logits=False)
        loss.backward()
        o1.step(grad_scale=e1.finish_grad_sync())
        o1.zero_grad()
        eager.append(loss.item())
    m2, o2, e2 = make()
    g = GraphedTrainStep(m2, o2, e2, 4, 128, torch.device(DEV), warmup=2)
    # capture() runs steps 0 and 1 eagerly on (x0, y0); feed the same data as the eager run
    g.x.copy_(xs[0]); g.y.copy_(ys[0])
    o2.prepare_graph_step(1e-3); g._body()
    g.capture(xs[1], ys[1], 1e-3)  # warmup=2 -> two more eager steps on (x1, y1): redo eager ref below
    torch.cuda.synchronize()
    # compare only the replayed part against an eager model that saw the same batches
    m3, o3, e3 = make()
    seq = [(xs[0], ys[0]), (xs[1], ys[1]), (xs[1], ys[1])]
    for x, y in seq:
        _, loss = m3(x, y, return_logits=False)
        loss.backward()
        o3.step(grad_scale=e3.finish_grad_sync())
        o3.zero_grad()
    for i in range(2, 6):
        lg = g(xs[i], ys[i], 1e-3).item()
        _, le = m3(xs[i], ys[i], return_logits=False)
        le.backward()
        o3.step(grad_scale=e3.finish_grad_sync())
        o3.zero_grad()
        assert abs(lg - le.item()) < 1e-3 * max(1.0, abs(le.item())), (i, lg, le.item())
    assert eager[0] > 0


def test_attention_block_bwd_partial_keys():
    """Context-parallel building block: the backward of each key block, given the final
    o/lse of the whole row, sums to the full attention gradient (HIP kernels)."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(21)
    B, T, H, Hkv, D = 2, 256, 4, 2, 64
    q = torch.randn(B, 2 * T, H, D, device=DEV).bfloat16()
    k = torch.randn(B, 2 * T, Hkv, D, device=DEV).bfloat16()
    v = torch.randn(B, 2 * T, Hkv, D, device=DEV).bfloat16()
    do = torch.randn(B, 2 * T, H, D, device=DEV).bfloat16()
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    of, _ = ref.attention(qf, kf, vf, causal=True)
    of.backward(do.float())
    # second query half: key block 0 fully visible, key block 1 = the causal diagonal
    q2, do2 = q[:, T:], do[:, T:]
    o0, l0 = ops.attention(q2, k[:, :T], v[:, :T], causal=False, return_lse=True)
    o1, l1 = ops.attention(q2, k[:, T:], v[:, T:], causal=True, return_lse=True)
    lse = torch.logaddexp(l0, l1)
    o = (o0.float() * torch.exp(l0 - lse).transpose(1, 2).unsqueeze(-1)
         + o1.float() * torch.exp(l1 - lse).transpose(1, 2).unsqueeze(-1)).bfloat16()
    assert _rel(o, of[:, T:]) < 1e-2
    g0 = ops.attention_block_bwd(do2, q2, k[:, :T], v[:, :T], o, lse, causal=False)
    g1 = ops.attention_block_bwd(do2, q2, k[:, T:], v[:, T:], o, lse, causal=True)
    assert _rel(g0[0].float() + g1[0].float(), qf.grad[:, T:]) < 2e-2
    # keys of block 1 are only seen by the second query half
    assert _rel(g1[1], kf.grad[:, T:]) < 2e-2
    assert _rel(g1[2], vf.grad[:, T:]) < 2e-2


def test_fused_sampling_distribution():
    """Gumbel-max kernel: greedy == argmax, masked logits never drawn, frequencies match softmax(l/T)."""
    torch.manual_seed(22)
    V = 8
    base = torch.tensor([2.0, 1.0, 0.5, 0.0, -1.0, float("-inf"), 1.5, -0.5], device=DEV)
    rows = 40000
    logits = base.repeat(rows, 1)
    ids = _ops().sample(logits, 0.7, 1234).view(-1)
    assert ids.dtype == torch.int64 and int(ids.max()) < V
    assert not bool((ids == 5).any())
    freq = torch.bincount(ids, minlength=V).float() / rows
    p = torch.softmax(base / 0.7, 0)
    assert (freq - p).abs().max().item() < 0.01, (freq, p)
    # different seeds -> different draws; same seed -> same draws
    assert torch.equal(ids, _ops().sample(logits, 0.7, 1234).view(-1))
    assert not torch.equal(ids, _ops().sample(logits, 0.7, 99).view(-1))
    big = torch.randn(3, 50304, device=DEV)
    assert torch.equal(_ops().sample(big, 0.0, 0).view(-1), big.argmax(-1))
    assert torch.equal(_ops().sample(big.bfloat16(), 0.0, 0).view(-1), big.bfloat16().argmax(-1))


def test_transposed_weight_shadows_track_steps():
    """FlatAdamW's W^T shadows (used by the backward data-gradient GEMMs) stay equal to the
    weights through optimizer steps, and training with them matches training without."""
    from pretraining_llm_amd.models import GPT, get_preset
    from pretraining_llm_amd.train.optim import FlatAdamW
    cfg = get_preset("gpt2-tiny").replace(context_length=128, vocab_size=1024)
    xs = [torch.randint(0, 1024, (2, 128), device=DEV) for _ in range(3)]
    losses = {}
    for shadow in (True, False):
        torch.manual_seed(23)
        m = GPT(cfg).to(DEV, torch.bfloat16)
        opt = FlatAdamW(m, lr=1e-3, transposed_shadow=shadow)
        assert bool(opt.shadowed) == shadow
        out = []
        for x in xs:
            _, loss = m(x, x.roll(-1, 1), return_logits=False)
            loss.backward()
            opt.step()
            opt.zero_grad()
            out.append(loss.item())
        for p in opt.shadowed:
            assert torch.equal(p._pllm_wT, p.t())
        losses[shadow] = (out, opt.flat_param.float().clone())
    assert max(abs(a - b) for a, b in zip(losses[True][0], losses[False][0])) < 1e-2
    assert _rel(losses[True][1], losses[False][1]) < 1e-2


def test_batched_transpose_kernel():
    torch.manual_seed(24)
    shapes = [(72, 200), (1024, 56), (64, 64), (8, 8), (2304, 768)]
    src = [torch.randn(s, device=DEV).bfloat16() for s in shapes]
    dst = [torch.empty(s[1], s[0], device=DEV, dtype=torch.bfloat16) for s in shapes]
    desc = _ops().transpose_plan(src, dst)
    tiles = sum(((r + 63) // 64) * ((c + 63) // 64) for r, c in shapes)
    _ops().transpose_run(desc, tiles)
    for s, d in zip(src, dst):
        assert torch.equal(d, s.t())
    with pytest.raises(RuntimeError):
        _ops().transpose_plan([torch.randn(12, 20, device=DEV).bfloat16()],
                              [torch.empty(20, 12, device=DEV, dtype=torch.bfloat16)])


def test_norm_and_embedding_fp32_grad_targets():
    """norm backward / embedding backward add their parameter gradients into fp32 targets (the
    optimizer's default flat-gradient dtype) at fp32 accuracy."""
    torch.manual_seed(25)
    N, C = 1000, 768
    x = torch.randn(N, C, device=DEV).bfloat16()
    w = (1 + 0.1 * torch.randn(C, device=DEV)).bfloat16()
    b = (0.1 * torch.randn(C, device=DEV)).bfloat16()
    y, _, mean, rstd = _ops().norm_fwd(x, None, w, b, 1e-5, False)
    s = x  # no residual: the normalised stream is x itself
    dy = torch.randn(N, C, device=DEV).bfloat16()
    dx16, dw16, db16 = _ops().norm_bwd(dy, s, w, mean, rstd, None, True, False)
    dw32 = torch.full((C,), 0.5, device=DEV)
    db32 = torch.full((C,), -0.5, device=DEV)
    xb32 = torch.zeros(C, device=DEV)
    dx32 = _ops().norm_bwd_acc(dy, s, w, mean, rstd, None, True, False, dw32, db32, xb32)
    assert torch.equal(dx32, dx16)
    xh = (s.double() - mean.double()[:, None]) * rstd.double()[:, None]
    assert _rel(dw32.double() - 0.5, (dy.double() * xh).sum(0)) < 1e-4
    assert _rel(db32.double() + 0.5, dy.double().sum(0)) < 1e-6
    assert _rel(xb32.double(), dx32.double().sum(0)) < 1e-6
    # embedding
    V, T, B = 500, 64, 8
    wte = torch.randn(V, C, device=DEV).bfloat16()
    wpe = torch.randn(T, C, device=DEV).bfloat16()
    idx = torch.randint(0, 40, (B, T), device=DEV)
    d = torch.randn(B, T, C, device=DEV).bfloat16()
    gte = torch.ones(V, C, device=DEV)
    gpe = torch.ones(T, C, device=DEV)
    _ops().embedding_bwd_acc(d, idx, V, T, True, gte, gpe)
    ref_te = torch.ones(V, C, device=DEV, dtype=torch.float64).index_add_(0, idx.reshape(-1), d.double().reshape(-1, C))
    assert _rel(gte.double(), ref_te) < 1e-6
    assert _rel(gpe.double(), 1 + d.double().sum(0)) < 1e-6


def test_fp32_grad_accumulation_matches_big_batch():
    """8 micro-steps of batch 1 accumulated into the fp32 flat gradient == one step of batch 8
    (HIP path), to within what bf16 activations allow; and the fp32 buffer reproduces the
    bf16-gradient run's accumulation error with far less drift."""
    from pretraining_llm_amd.models import GPT, get_preset
    from pretraining_llm_amd.train.optim import FlatAdamW
    cfg = get_preset("gpt2-tiny").replace(context_length=128, vocab_size=1024)
    x = torch.randint(0, 1024, (8, 128), device=DEV)
    y = torch.randint(0, 1024, (8, 128), device=DEV)
    errs = {}
    for gd in (torch.float32, torch.bfloat16):
        torch.manual_seed(26)
        m = GPT(cfg).to(DEV, torch.bfloat16)
        opt = FlatAdamW(m, lr=1e-3, grad_dtype=gd)
        assert opt.flat_grad.dtype == gd
        _, loss = m(x, y, return_logits=False)
        loss.backward()
        big = opt.flat_grad.double().clone()
        opt.zero_grad()
        for i in range(8):
            _, loss = m(x[i:i + 1], y[i:i + 1], return_logits=False)
            loss.backward()
        acc = opt.flat_grad.double() / 8
        errs[gd] = _rel(acc, big)
    assert errs[torch.float32] < 1e-2, errs
    assert errs[torch.float32] <= errs[torch.bfloat16], errs


def test_graphed_steps_without_host_sync_match_eager():
    """Several hipGraph replays queued back to back with NO host synchronisation in between
    (the host runs ahead of the GPU) reproduce eager steps: each replay must read its own
    step's lr / bias corrections (FlatAdamW.prepare_graph_step's guarded staging ring)."""
    from pretraining_llm_amd.models import GPT, get_preset
    from pretraining_llm_amd.parallel.dp import DataParallelEngine
    from pretraining_llm_amd.train.graph import GraphedTrainStep
    from pretraining_llm_amd.train.optim import FlatAdamW
    cfg = get_preset("gpt2-tiny").replace(context_length=128, vocab_size=1024, n_head=2)
    xs = [torch.randint(0, 1024, (4, 128), device=DEV) for _ in range(10)]
    lrs = [1e-3 * (1 + 0.3 * i) for i in range(10)]

    def make():
        torch.manual_seed(27)
        m = GPT(cfg).to(DEV, torch.bfloat16)
        o = FlatAdamW(m, lr=1e-3, max_grad_norm=1.0)
        return m, o, DataParallelEngine(o)

    m1, o1, e1 = make()
    g = GraphedTrainStep(m1, o1, e1, 4, 128, torch.device(DEV), warmup=1).capture(xs[0], xs[0].roll(-1, 1), lrs[0])
    losses = [g(xs[i], xs[i].roll(-1, 1), lrs[i]).clone() for i in range(1, 10)]  # no sync in between
    torch.cuda.synchronize()
    m2, o2, e2 = make()
    ref = []
    for i in range(10):
        o2.param_groups[0]["lr"] = lrs[i]
        _, loss = m2(xs[i], xs[i].roll(-1, 1), return_logits=False)
        loss.backward()
        o2.step(grad_scale=e2.finish_grad_sync())
        o2.zero_grad()
        ref.append(loss.item())
    got = [l.item() for l in losses]
    for a, b in zip(got, ref[1:]):
        assert abs(a - b) < 1e-3 * max(1.0, abs(b)), (got, ref)
    # bf16-level noise moves small-gradient Adam updates (~0.4 % measured); a replay reading
    # another step's lr (+-30 % per step here) would be off by ~10x that
    assert _rel(o1.master, o2.master) < 2e-2


@pytest.mark.parametrize("chunk", [128, 8192])
@pytest.mark.parametrize("with_bias", [False, True])
def test_lm_head_ce_chunked(chunk, with_bias, monkeypatch):
    """Chunked LM head + CE (logits workspace of `chunk` rows, backward GEMMs and head-bias
    column sums done per chunk in the forward, ragged last chunk) vs fp32 torch; into fp32 flat
    gradient targets and as plain autograd gradients; no-grad evaluation path too."""
    from pretraining_llm_amd import ops
    monkeypatch.setattr(ops, "CE_CHUNK_ROWS", chunk)
    torch.manual_seed(28)
    N, C, V = 1000, 256, 50304
    h = (torch.randn(N, C, device=DEV) * 0.5).bfloat16().requires_grad_()
    W = (torch.randn(V, C, device=DEV) * 0.05).bfloat16().requires_grad_()
    b = (torch.randn(V, device=DEV) * 0.1).bfloat16().requires_grad_() if with_bias else None
    t = torch.randint(0, V, (N,), device=DEV)
    t[::5] = -100
    loss = ops.lm_head_cross_entropy(h, W, b, t)
    (loss * 0.5).backward()  # upstream scale folded in the backward
    hf, Wf = h.detach().float().requires_grad_(), W.detach().float().requires_grad_()
    bf = b.detach().float().requires_grad_() if with_bias else None
    logits = hf @ Wf.t() + (bf if with_bias else 0)
    lf = F.cross_entropy(logits, t, ignore_index=-100)
    (lf * 0.5).backward()
    assert abs(loss.item() - lf.item()) < 3e-3 * lf.item()
    assert _rel(h.grad, hf.grad) < 3e-2
    assert _rel(W.grad, Wf.grad) < 3e-2
    if with_bias:
        assert _rel(b.grad, bf.grad) < 3e-2
    with torch.no_grad():
        le = ops.lm_head_cross_entropy(h, W, b, t)
    assert abs(le.item() - loss.item()) < 1e-4 * loss.item()
    # fp32 flat-gradient targets (FlatAdamW params): gradients added, not returned
    W.grad = None
    W._pllm_flat_grad = True
    W._pllm_gradbuf = torch.ones(V, C, device=DEV)
    ops.lm_head_cross_entropy(h, W, b, t).backward()
    assert W.grad is None
    assert _rel(W._pllm_gradbuf.double() - 1, 2 * Wf.grad.double()) < 3e-2
    # an untouched slot (lazy zeroing's first writer of the step): the chunks write straight into it during the
    # forward -- over stale NaN -- and the backward scales it in place by the upstream gradient (3 here; and 1)
    for up in (3.0, 1.0):
        W._pllm_gradbuf = torch.full((V, C), float("nan"), device=DEV)
        W._pllm_grad_fresh = True
        (ops.lm_head_cross_entropy(h, W, b, t) * up).backward()
        assert W._pllm_grad_fresh is False and W.grad is None
        assert not W._pllm_gradbuf.isnan().any()
        assert _rel(W._pllm_gradbuf.double(), 2 * up * Wf.grad.double()) < 3e-2


def test_lm_head_ce_two_calls_on_one_weight():
    """3 ce(h1, t1) + 0.5 ce(h2, t2) on one weight whose slot is fresh: the first call writes dW1 into the slot
    in its forward and keeps it reserved, the second call's backward (it runs first) finds no slot and returns
    0.5 dW2 as a tensor, the first call's backward scales the slot by 3, releases it and notifies, and the
    optimizer's post-accumulate hook folds the tensor in last: 3 dW1 + 0.5 dW2.  Scaling after the second call had
    added into the slot would give 3 (dW1 + 0.5 dW2), off by |dW2| / |3 dW1 + 0.5 dW2|: 0.32-0.33 in the fp32
    reference on the CPU for independent inputs of these sizes (|dW2| / |dW1| = 0.98-1.00), ten times the bound.
    Then the stale reservation: a forward under grad mode whose backward never runs leaves the slot reserved, and
    FlatAdamW's _clear_unwritten (zeroed, written) and zero_grad (fresh) both end that."""
    import torch.nn as nn
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.train.optim import FlatAdamW, _fold_grad
    torch.manual_seed(29)
    N, C, V = 128, 64, 512
    W = (torch.randn(V, C, device=DEV) * 0.05).bfloat16().requires_grad_()
    hs = [(torch.randn(N, C, device=DEV) * 0.5).bfloat16().requires_grad_() for _ in range(2)]
    ts = [torch.randint(0, V, (N,), device=DEV) for _ in range(2)]
    dws = []
    for h, t in zip(hs, ts):  # fp32 torch gradient of each call alone
        Wf = W.detach().float().requires_grad_()
        F.cross_entropy(h.detach().float() @ Wf.t(), t).backward()
        dws.append(Wf.grad.double())
    want, wrong = 3 * dws[0] + 0.5 * dws[1], 3 * (dws[0] + 0.5 * dws[1])
    assert _rel(wrong, want) > 0.3  # the inputs tell the two apart
    log = []
    W._pllm_grad_ready = lambda: log.append("W")
    W._pllm_flat_grad = True
    W._pllm_gradbuf = torch.full((V, C), float("nan"), device=DEV)
    W._pllm_grad_fresh = True
    W.register_post_accumulate_grad_hook(_fold_grad)  # as FlatAdamW does for fp32 slots of bf16 parameters
    ce = [ops.lm_head_cross_entropy(h, W, None, t) for h, t in zip(hs, ts)]
    loss = 3.0 * ce[0] + 0.5 * ce[1]
    assert W._pllm_grad_reserved is True and W._pllm_grad_fresh is False
    loss.backward()
    err = _rel(W._pllm_gradbuf.double(), want)
    print(f"two calls: rel err {err:.3e} (the wrong order would give {_rel(wrong, want):.3f})")
    assert err < 3e-2
    assert W._pllm_grad_reserved is False and W._pllm_grad_fresh is False and W.grad is None
    assert log == ["W"]  # the slot's one direct write; the folded part is the hook's to report
    # a forward that never gets its backward
    model = nn.Sequential(nn.Linear(C, C, bias=False), nn.Linear(C, V, bias=False))
    model = model.to(device=DEV, dtype=torch.bfloat16)
    opt = FlatAdamW(model, lr=1e-3, lazy_zero=True)
    Wm = model[1].weight
    assert opt.lazy_zero and Wm._pllm_grad_fresh is True
    for end in (opt._clear_unwritten, opt.zero_grad):
        ops.lm_head_cross_entropy(hs[0], Wm, None, ts[0])
        assert Wm._pllm_grad_reserved is True and Wm._pllm_grad_fresh is False
        assert ops._take(Wm) == (None,)
        end()
        assert Wm._pllm_grad_reserved is False
        assert Wm._pllm_grad_fresh is True or (Wm._pllm_gradbuf == 0).all()  # fresh, or zero and written
        assert ops._take(Wm, whole=True)[0][0] is Wm._pllm_gradbuf
        opt.zero_grad()


@pytest.mark.parametrize("D,T,H,Hkv,B", [(32, 1024, 4, 4, 2), (64, 2048, 4, 2, 1), (64, 4096, 2, 2, 1),
                                         (128, 2048, 4, 1, 1), (128, 4096, 2, 2, 1), (64, 1000, 4, 4, 2)])
def test_attention_bwd_long_sequences(D, T, H, Hkv, B):
    """Backward at the shipped sequence lengths (2048 / 4096, several key blocks and dQ slabs),
    D = 32 / 64 (fused-role kernel) and 128 (key-stationary kernel), GQA, ragged T, vs fp32 torch; a
    forced multi-pass run (bounded dQ workspace) is bit-identical to the single-pass one."""
    torch.manual_seed(T + D)
    q = torch.randn(B, T, H, D, device=DEV).bfloat16()
    k = torch.randn(B, T, Hkv, D, device=DEV).bfloat16()
    v = torch.randn(B, T, Hkv, D, device=DEV).bfloat16()
    do = torch.randn(B, T, H, D, device=DEV).bfloat16()
    scale = 1 / math.sqrt(D)
    o, lse = torch.ops.pllm.attn_fwd(q, k, v, True, scale)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    of, _ = _attn_ref(qf, kf, vf, True, scale)
    of.backward(do.float())
    try:
        ref = [torch.empty_like(t) for t in (q, k, v)]
        torch.ops.pllm.attn_bwd(do, q, k, v, o, lse, *ref, True, scale)
        for a, b, n in zip(ref, (qf.grad, kf.grad, vf.grad), ("dq", "dk", "dv")):
            assert _rel(a, b) < 2e-2, (n, _rel(a, b))
        torch.ops.pllm.attn_bwd_set_workspace_mb(1e-3)  # one key block per pass
        got = [torch.empty_like(t) for t in (q, k, v)]
        torch.ops.pllm.attn_bwd(do, q, k, v, o, lse, *got, True, scale)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
    finally:
        torch.ops.pllm.attn_bwd_set_workspace_mb(4096)


@pytest.mark.parametrize("D,Hkv", [(64, 4), (128, 2), (64, 1), (32, 2)])
def test_attention_fused_rope_fwd_bwd(D, Hkv):
    """RoPE with the HIP attention == rotate-half RoPE + attention in fp32 torch, gradients
    w.r.t. the UNROTATED packed qkv: rope_qk rotates q / k once, the backward rotates dq / dk
    back while storing them."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(29 + D)
    B, T, H = 2, 640, 4
    qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV) * 0.8).bfloat16().requires_grad_()
    cos, sin = ops.rope_cache(T + 64, D, 10000.0, DEV)  # table longer than T, as in the model
    o = ops.attention_packed(qkv, H, Hkv, causal=True, rope_cos=cos, rope_sin=sin)
    do = torch.randn_like(o)
    o.backward(do)
    qkvf = qkv.detach().float().requires_grad_()
    q, k, v = ops._split_qkv(qkvf, H, Hkv, D)
    qr, kr = ref.rope(q, cos[:T], sin[:T]), ref.rope(k, cos[:T], sin[:T])
    of, _ = _attn_ref(qr, kr, v, True, 1 / math.sqrt(D))
    of = of.reshape(B, T, H * D)
    of.backward(do.float())
    assert _rel(o, of) < 1.5e-2, _rel(o, of)
    gq, gk, gv = ops._split_qkv(qkv.grad, H, Hkv, D)
    rq, rk, rv = ops._split_qkv(qkvf.grad, H, Hkv, D)
    for a, b, n in ((gq, rq, "q"), (gk, rk, "k"), (gv, rv, "v")):
        assert _rel(a, b) < 3e-2, (n, _rel(a, b))


@pytest.mark.parametrize("M,P,Q", [(4096, 50304, 768), (2048, 50304, 2048), (1024, 11008, 2048), (8192, 65536, 256),
                                   (4096, 4104, 4104), (1024, 4352, 4096),
                                   (32768, 11008, 2048)])  # llama gate/up: the remainder in two rounds of 5 slices
def test_wgrad_hybrid(M, P, Q):
    """Hybrid weight gradients (the default, csrc/wgrad_pp.hip: more tiles than workgroups -> whole tiles for
    the grid's whole rounds, the remaining tiles as slices of the last round, finished by the ordered fix-up;
    edge tiles included): fp64 reference, accumulation into a non-zero gradient, OVERWRITE of a NaN-filled
    target (every tile must be written: lazy zeroing and the LM head's first chunk rely on it), run-to-run
    determinism, and agreement with the slice kernel."""
    torch.manual_seed(31)
    dy = (torch.randn(M, P, device=DEV) * 0.3).bfloat16()
    x = torch.randn(M, Q, device=DEV).bfloat16()
    w0 = torch.randn(P, Q, device=DEV)
    prod = dy.double().t() @ x.double()
    ref = w0.double() + prod
    acc = w0.clone()
    torch.ops.pllm.wgrad(dy, x, acc)
    acc2 = w0.clone()
    torch.ops.pllm.wgrad(dy, x, acc2)
    assert _rel(acc.double(), ref) < 1e-5, _rel(acc.double(), ref)
    assert torch.equal(acc, acc2)  # deterministic
    ow = torch.full((P, Q), float("nan"), device=DEV)
    torch.ops.pllm.wgrad(dy, x, ow, None, True)
    assert not ow.isnan().any(), "tiles left unwritten by the overwrite path"
    assert _rel(ow.double(), prod) < 1e-5, _rel(ow.double(), prod)
    try:
        torch.ops.pllm.wgrad_set_hy(0)  # the slice kernel as the reference
        acc3 = w0.clone()
        torch.ops.pllm.wgrad(dy, x, acc3)
        ow3 = torch.full((P, Q), float("nan"), device=DEV)
        torch.ops.pllm.wgrad(dy, x, ow3, None, True)
    finally:
        torch.ops.pllm.wgrad_set_hy(1)  # the shipped default
    # two fp32 summation orders over M tokens (1.03e-6 apart at M = 32768)
    tol = 1e-6 if M <= 8192 else 3e-6
    assert _rel(acc.double(), acc3.double()) < tol
    assert _rel(ow.double(), ow3.double()) < tol


def test_lm_head_ce_overwrite_nan_buffer():
    """GPT-2's LM head shape class (C = 768, V = 50304: 591 weight-gradient tiles, more than the CUs, so the
    hybrid kernel runs) with the first chunk OVERWRITING a dw buffer that the caching allocator hands back
    full of NaN: the weight gradient must still match fp32 torch everywhere."""
    from pretraining_llm_amd import ops
    torch.manual_seed(41)
    N, C, V = 4096, 768, 50304
    junk = torch.full((V, C), float("nan"), device=DEV)  # same-size block for the op's torch.empty
    del junk
    h = (torch.randn(N, C, device=DEV) * 0.5).bfloat16().requires_grad_()
    W = (torch.randn(V, C, device=DEV) * 0.05).bfloat16().requires_grad_()
    t = torch.randint(0, V, (N,), device=DEV)
    loss = ops.lm_head_cross_entropy(h, W, None, t)
    loss.backward()
    Wf = W.detach().float().requires_grad_()
    F.cross_entropy(h.detach().float() @ Wf.t(), t).backward()
    assert not W.grad.isnan().any()
    assert _rel(W.grad, Wf.grad) < 3e-2, _rel(W.grad, Wf.grad)


@pytest.mark.parametrize("M,P,Q", [(4096, 4096, 8192), (8192, 2304, 768), (4096, 50304, 768), (2048, 200, 136)])
def test_wgrad_pp_kernel(M, P, Q):
    """The ping-pong weight-gradient kernel (csrc/wgrad_pp.hip; wgrad's default for fp32 targets):
    persistent workgroups with several (slice, tile) items each, edge tiles, the split-K slab and the
    single-slice accumulate paths -- against fp64 math and against the one-barrier kernel it replaces."""
    torch.manual_seed(23)
    dy = (torch.randn(M, P, device=DEV) * 0.3).bfloat16()
    x = torch.randn(M, Q, device=DEV).bfloat16()
    w0 = torch.randn(P, Q, device=DEV)
    ref = w0.double() + dy.double().t() @ x.double()
    acc = w0.clone()
    torch.ops.pllm.wgrad(dy, x, acc)
    assert _rel(acc.double(), ref) < 1e-5, _rel(acc.double(), ref)
    acc2 = w0.clone()
    torch.ops.pllm.wgrad(dy, x, acc2)
    assert torch.equal(acc, acc2)  # deterministic
    try:
        torch.ops.pllm.wgrad_set_mfma(100)  # the one-barrier kernel
        acc3 = w0.clone()
        torch.ops.pllm.wgrad(dy, x, acc3)
    finally:
        torch.ops.pllm.wgrad_set_mfma(0)
    assert _rel(acc.double(), acc3.double()) < 1e-6
    # bias gradient on the side (all-ones MFMAs on the first column tile's items)
    # (a bias gradient keeps the plain slice plan: with more tiles than CUs the no-bias call above took the
    # hybrid split, whose sliced last round sums in another order -- compare against that plan's result)
    b0 = torch.randn(P, device=DEV)
    acc4, bacc = w0.clone(), b0.clone()
    torch.ops.pllm.wgrad(dy, x, acc4, bacc)
    try:
        torch.ops.pllm.wgrad_set_hy(0)
        acc5 = w0.clone()
        torch.ops.pllm.wgrad(dy, x, acc5)
    finally:
        torch.ops.pllm.wgrad_set_hy(1)
    assert torch.equal(acc4, acc5)
    assert _rel(bacc.double(), b0.double() + dy.double().sum(0)) < 1e-6


@pytest.mark.parametrize("D", [32, 64, 128])
def test_lse_merge_kernel(D):
    """Ring attention's fused LSE merge (lse_merge_) vs the torch formula of parallel/context.py, on
    strided accumulator views (a T-chunk of a bigger buffer) with fully masked (-inf) rows on either side."""
    torch.manual_seed(29)
    B, T, H = 2, 96, 4
    full = torch.randn(B, 2 * T, H, D, device=DEV)
    o_acc = full[:, T:]                      # strided view, as the per-chunk accumulators
    lfull = torch.randn(B, H, 2 * T, device=DEV)
    lse_acc = lfull[:, :, T:]
    o = torch.randn(B, T, H, D, device=DEV).bfloat16()
    lse = torch.randn(B, H, T, device=DEV)
    lse_acc[:, :, :5] = float("-inf")        # accumulator rows not yet seen
    lse[:, :, 3:8] = float("-inf")           # block rows fully masked (rows 3, 4: both)
    ref_o, ref_l = o_acc.clone(), lse_acc.clone()
    before = full[:, :T].clone()
    new = torch.logaddexp(ref_l, lse)
    a = torch.exp(ref_l - new).nan_to_num_(0.0).transpose(1, 2).unsqueeze(-1)
    b = torch.exp(lse - new).nan_to_num_(0.0).transpose(1, 2).unsqueeze(-1)
    ref_o = ref_o * a + o.float() * b
    torch.ops.pllm.lse_merge_(o_acc, lse_acc, o, lse)
    assert torch.allclose(lse_acc, new, rtol=1e-5, atol=1e-5, equal_nan=True)
    assert torch.allclose(o_acc, ref_o, rtol=1e-5, atol=1e-5)
    assert torch.equal(full[:, :T], before)  # the rest of the buffer is untouched


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T,S,H,Hkv,B,causal", [(2048, 2048, 4, 2, 1, True), (1000, 1000, 2, 2, 2, True),
                                                 (512, 512, 2, 1, 2, False), (320, 384, 2, 2, 1, True),
                                                 (300, 340, 2, 1, 1, True), (96, 700, 2, 2, 1, False)])
def test_attention_bwd_key_stationary(D, T, S, H, Hkv, B, causal):
    """The backward that ships for each head dim -- D = 128: the key-stationary kernel (csrc/attn_bwd_ks.hip:
    4 waves x 64 keys, dK / dV in the accumulator file, one barrier per query slice); D = 64: the fused-role
    kernel (csrc/attention.hip) -- vs fp32 math: causal and not, GQA, ragged T, queries aligned to the END of
    longer key rows (S > T, offset 64 = 32-aligned and 40 = the per-element masked path), ragged key blocks
    (S = 340, 700), and a forced one-key-block-per-pass run (bit-identical)."""
    torch.manual_seed(T + S + D)
    q = torch.randn(B, T, H, D, device=DEV).bfloat16()
    k = torch.randn(B, S, Hkv, D, device=DEV).bfloat16()
    v = torch.randn(B, S, Hkv, D, device=DEV).bfloat16()
    do = torch.randn(B, T, H, D, device=DEV).bfloat16()
    scale = 1 / math.sqrt(D)
    o, lse = torch.ops.pllm.attn_fwd(q, k, v, causal, scale)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    of, _ = _attn_ref(qf, kf, vf, causal, scale)
    of.backward(do.float())
    try:
        got = [torch.empty_like(t) for t in (q, k, v)]
        torch.ops.pllm.attn_bwd(do, q, k, v, o, lse, *got, causal, scale)
        for a, b, n in zip(got, (qf.grad, kf.grad, vf.grad), ("dq", "dk", "dv")):
            assert not a.isnan().any(), n
            assert _rel(a, b) < 2e-2, (n, _rel(a, b))
        torch.ops.pllm.attn_bwd_set_workspace_mb(1e-3)  # one key block per pass
        got2 = [torch.empty_like(t) for t in (q, k, v)]
        torch.ops.pllm.attn_bwd(do, q, k, v, o, lse, *got2, causal, scale)
        for a, b in zip(got2, got):
            assert torch.equal(a, b)
    finally:
        torch.ops.pllm.attn_bwd_set_workspace_mb(4096)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T,S", [(200, 264), (300, 340)])
def test_attention_bwd_key_stationary_rope_offset(D, T, S):
    """RoPE with queries aligned to the END of longer key rows (S > T; offsets 64 and 40, the latter not a
    multiple of 32): q is rotated at positions t + S - T and k at s (the rope op), the forward and the
    backward run on the rotated heads and the backward rotates dq / dk back -- under the kernel that ships
    for the head dim (fused-role D = 64, key-stationary D = 128).  Against fp32 rotate-half RoPE + causal
    attention, gradients w.r.t. the UNROTATED q / k."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(T + S + D + 5)
    B, H, Hkv = 2, 4, 2
    q = (torch.randn(B, T, H, D, device=DEV) * 0.8).bfloat16()
    k = (torch.randn(B, S, Hkv, D, device=DEV) * 0.8).bfloat16()
    v = torch.randn(B, S, Hkv, D, device=DEV).bfloat16()
    do = torch.randn(B, T, H, D, device=DEV).bfloat16()
    cos, sin = ops.rope_cache(S + 32, D, 10000.0, DEV)
    scale = 1 / math.sqrt(D)
    qf, kf, vf = (t.float().requires_grad_() for t in (q, k, v))
    qr = ref.rope(qf, cos[S - T:S], sin[S - T:S])
    kr = ref.rope(kf, cos[:S], sin[:S])
    of, _ = _attn_ref(qr, kr, vf, True, scale)
    of.backward(do.float())
    qrot = torch.ops.pllm.rope(q.view(B, T, H * D), cos, sin, H, H, T, S - T, False).view(B, T, H, D)
    krot = torch.ops.pllm.rope(k.view(B, S, Hkv * D), cos, sin, Hkv, Hkv, S, 0, False).view(B, S, Hkv, D)
    o, lse = torch.ops.pllm.attn_fwd(qrot, krot, v, True, scale)
    assert _rel(o, of) < 1.5e-2, _rel(o, of)
    got = [torch.empty_like(t) for t in (q, k, v)]
    torch.ops.pllm.attn_bwd(do, qrot, krot, v, o, lse, *got, True, scale, cos, sin)
    for a, b, n in zip(got, (qf.grad, kf.grad, vf.grad), ("dq", "dk", "dv")):
        assert not a.isnan().any(), n
        assert _rel(a, b) < 3e-2, (n, _rel(a, b))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_scale_inplace_unit_fast_path(dtype):
    """torch.ops.pllm.scale_ (the LM-head backward's upstream-gradient scale): x *= s in place for bf16 / fp32,
    and a bit-exact no-op when s == 1 (the kernel returns before touching x)."""
    torch.manual_seed(5)
    x = (torch.randn(1 << 20, device=DEV) * 3).to(dtype)
    x[::7] = float("nan")
    ref = x.clone()
    torch.ops.pllm.scale_(x, torch.tensor([1.0], device=DEV))
    assert torch.equal(x.isnan(), ref.isnan()) and torch.equal(x[~x.isnan()], ref[~ref.isnan()])
    torch.ops.pllm.scale_(x, torch.tensor([-0.375], device=DEV))
    want = (ref.float() * -0.375).to(dtype)
    assert torch.equal(x.isnan(), want.isnan()) and torch.equal(x[~x.isnan()], want[~want.isnan()])


def test_grad_norm_clip_matches_torch():
    """torch.ops.pllm.grad_norm_clip (the optimizer's norm + clip coefficient in two launches) vs the torch
    expression it replaced: norm = sqrt(sum g^2) * grad_scale, clip = min(max_norm / (norm + 1e-6), 1); both
    the clipping and the non-clipping side; deterministic."""
    torch.manual_seed(9)
    g = torch.randn(3 * 2 ** 20 + 64, device=DEV)
    for scale, max_norm in ((0.5, 1.0), (1.0, 1e6)):
        out = torch.ops.pllm.grad_norm_clip(g, scale, max_norm)
        norm = g.double().pow(2).sum().sqrt() * scale
        clip = min(max_norm / (norm.item() + 1e-6), 1.0)
        assert abs(out[0].item() - norm.item()) < 1e-5 * norm.item()
        assert abs(out[1].item() - clip) < 1e-5 * clip
        assert torch.equal(torch.ops.pllm.grad_norm_clip(g, scale, max_norm), out)
