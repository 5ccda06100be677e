"""Attention sinks on the GPU: ``attn_fwd`` / ``attn_decode`` with ``sinks``, ``attn_bwd`` on the sink-inclusive lse
(through ``delta_out`` and with a ready ``delta``) and ``attn_sink_bwd`` against the fp64 references and budgets of
``_attn_sink_refs.py`` on every case; the bit-identity contracts of the plain path; the ops against fp32 reference
math under autograd; and the model (``llama-tiny-sinks``): HIP path against the reference backend, the captured
training step against the eager one, the flat-gradient slot, and greedy generation through every decode path and
both servers."""
import math

import pytest
import torch

import _attention_refs as A
import _attn_sink_refs as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
P = torch.ops.pllm


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _dev(t):
    return None if t is None else t.to(DEV)


def _fwd(inp):
    o, lse = P.attn_fwd(_dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"]), True, inp["scale"],
                        _dev(inp.get("kv_start")), _dev(inp["sinks"]))
    return dict(o=o, lse=lse)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", K.fwd_cases(), ids=str)
def test_attn_fwd_with_sinks(case):
    inp, _ = K.fwd_case(case)
    K.check_all(K.fwd_checks(case, _fwd(inp)))


@pytest.mark.parametrize("case", K.window_cases(), ids=str)
def test_attn_fwd_with_sinks_and_kv_start(case):
    inp, _ = K.fwd_case(case, True)
    K.check_all(K.fwd_checks(case, _fwd(inp), True))


@pytest.mark.parametrize("case", [("randn", 257, 257, 32, 2), ("randn", 300, 340, 64, 1), ("randn", 129, 129, 128, 4),
                                  ("randn", 1, 65, 64, 4)], ids=str)
def test_plain_path_is_bit_identical(case):
    """``sinks=None`` is the call without the argument, and sinks of -inf change no bit of o or lse (M = m,
    2^0 = 1, 2^-inf = 0, all exact), plain and with kv_start; a sink of +inf gives o = 0 and lse = +inf, no NaN."""
    inp, _ = K.fwd_case(case)
    q, k, v = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"])
    o0, l0 = P.attn_fwd(q, k, v, True, inp["scale"])
    o1, l1 = P.attn_fwd(q, k, v, True, inp["scale"], None, None)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    off = torch.full((K.H,), -math.inf, dtype=BF16, device=DEV)
    o2, l2 = P.attn_fwd(q, k, v, True, inp["scale"], None, off)
    assert torch.equal(o0, o2) and torch.equal(l0, l2)
    if case[1] == case[2]:
        ks = K.window_start(case[1], 17).to(torch.int32).expand(K.B, -1).contiguous().to(DEV)
        o3, l3 = P.attn_fwd(q, k, v, True, inp["scale"], ks)
        o4, l4 = P.attn_fwd(q, k, v, True, inp["scale"], ks, off)
        assert torch.equal(o3, o4) and torch.equal(l3, l4) and not torch.equal(l3, l0)
    mixed = torch.tensor([math.inf, -math.inf, 0.0, math.inf], dtype=BF16, device=DEV)
    o5, l5 = P.attn_fwd(q, k, v, True, inp["scale"], None, mixed)
    assert torch.isfinite(o5).all() and not torch.isnan(l5).any()
    assert not o5[:, :, 0].any() and not o5[:, :, 3].any() and torch.isposinf(l5[:, 0]).all()
    assert torch.equal(o5[:, :, 1], o0[:, :, 1]) and torch.equal(l5[:, 1], l0[:, 1])


def test_host_checks_reject_bad_sinks():
    inp, _ = K.fwd_case(("randn", 33, 33, 32, 2))
    q, k, v = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"])
    s = _dev(inp["sinks"])
    for bad, msg in ((s.float(), "bf16"), (s[:3], "shape"), (s.cpu(), "device"), (s.repeat(2)[::2], "contiguous")):
        with pytest.raises(RuntimeError, match=msg):
            P.attn_fwd(q, k, v, True, inp["scale"], None, bad)
    with pytest.raises(RuntimeError, match="shape"):
        P.attn_decode(q[:, :1], k, v, inp["scale"], None, 0, s[:2])
    lse = torch.zeros(2, 4, 8, device=DEV)
    with pytest.raises(RuntimeError, match="sinks"):
        P.attn_sink_bwd(lse, lse, s[:3], None, False)
    with pytest.raises(RuntimeError, match="delta"):
        P.attn_sink_bwd(lse, lse[:, :, :4].contiguous(), s, None, False)


# ------------------------------------------------------------------------------------------------ backward
def _run_bwd(inp, delta=None, delta_out=None):
    q, k, v = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"])
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    P.attn_bwd(_dev(inp["do"]), q, k, v, _dev(inp["o"]), _dev(inp["lse"]), dq, dk, dv, True, inp["scale"], None, None,
               delta, None, None, delta_out)
    return dict(dq=dq, dk=dk, dv=dv)


@pytest.mark.parametrize("case", K.bwd_cases(), ids=str)
def test_attn_bwd_on_the_sink_inclusive_lse(case):
    """The backward kernels unchanged, fed the reference's sink-inclusive lse and bf16 o, under the existing
    attn_dq / attn_dk / attn_dv budgets: once keeping the pre-pass's delta (``delta_out``) and once with a ready
    ``delta``; the sink gradient from either delta under its own bound."""
    inp, ref = K.bwd_case(case)
    keep = torch.full(inp["lse"].shape, math.nan, device=DEV)
    out = _run_bwd(inp, delta_out=keep)
    K.check_all(K.bwd_checks(case, out))
    assert torch.isfinite(keep).all()
    sinks, lse = _dev(inp["sinks"]), _dev(inp["lse"])
    ds = torch.zeros(K.H, device=DEV)
    P.attn_sink_bwd(lse, keep, sinks, ds, True)
    K.check("sink_ds", ds, ref["ds"], "ds from delta_out")
    ready = _dev(inp["delta"])
    out2 = _run_bwd(inp, delta=ready)
    K.check_all(K.bwd_checks(case, out2))
    K.check("sink_ds", P.attn_sink_bwd(lse, ready, sinks, None, False), ref["ds"], "ds from the ready delta")
    # a ready delta wins over delta_out, which is then left alone
    untouched = torch.full(inp["lse"].shape, 7.0, device=DEV)
    out3 = _run_bwd(inp, delta=ready, delta_out=untouched)
    assert torch.equal(out3["dq"], out2["dq"]) and (untouched == 7.0).all()


@pytest.mark.parametrize("case", K.DS_CASES, ids=str)
def test_attn_sink_bwd(case):
    inp, ref = K.ds_case(case)
    lse, delta, sinks = _dev(inp["lse"]), _dev(inp["delta"]), _dev(inp["sinks"])
    Hq = case[1]
    fresh = P.attn_sink_bwd(lse, delta, sinks, None, False)
    assert fresh.dtype == BF16 and fresh.shape == (Hq,)
    K.check("sink_ds", fresh, ref, "fresh bf16")
    zeros, nans = torch.zeros(Hq, device=DEV), torch.full((Hq,), math.nan, device=DEV)
    e = P.attn_sink_bwd(lse, delta, sinks, zeros, False)
    assert e.numel() == 0
    K.check("sink_ds", zeros, ref, "fp32 slot")
    P.attn_sink_bwd(lse, delta, sinks, nans, True)
    assert torch.equal(nans, zeros), "overwrite into NaN != add into zeros"
    fill = torch.linspace(-3.0, 5.0, Hq, device=DEV)
    acc = fill.clone()
    P.attn_sink_bwd(lse, delta, sinks, acc, False)
    assert torch.equal(acc, fill + zeros), "accumulate is not fill + gradient"
    again = torch.zeros(Hq, device=DEV)
    P.attn_sink_bwd(lse, delta, sinks, again, False)
    assert torch.equal(again, zeros) and torch.equal(P.attn_sink_bwd(lse, delta, sinks, None, False), fresh)
    acc16 = torch.zeros(Hq, device=DEV, dtype=BF16)  # a bf16 flat gradient
    P.attn_sink_bwd(lse, delta, sinks, acc16, True)
    assert torch.equal(acc16, fresh)


def _opcheck_cases():
    r = lambda *s: torch.randn(*s, device=DEV).to(BF16)  # noqa: E731
    B, T, H, Hkv, D = 2, 40, 4, 2, 64
    sinks = r(H)
    lse, delta = torch.randn(B, H, T, device=DEV) + 3, torch.randn(B, H, T, device=DEV)
    q, k, v = r(B, T, H, D), r(B, T, Hkv, D), r(B, T, Hkv, D)
    o, lse_f = P.attn_fwd(q, k, v, True, 0.125, None, sinks)
    return [
        ("attn_sink_bwd", (lse, delta, sinks, None, False)),
        ("attn_sink_bwd", (lse, delta, sinks, torch.zeros(H, device=DEV), False)),
        ("attn_sink_bwd", (lse, delta, sinks, torch.zeros(H, device=DEV), True)),
        ("attn_fwd", (q, k, v, True, 0.125, None, sinks)),
        ("attn_decode", (q[:, :1].contiguous(), k, v, 0.125, torch.tensor([33], dtype=torch.int32, device=DEV), 16,
                         sinks)),
        ("attn_bwd", (r(B, T, H, D), q, k, v, o, lse_f, torch.empty_like(q), torch.empty_like(k), torch.empty_like(v),
                      True, 0.125, None, None, None, None, None, torch.empty_like(lse_f))),
    ]


@pytest.mark.parametrize("i", range(6))
def test_opcheck_fake_matches_kernel(i):
    torch.manual_seed(i)
    name, args = _opcheck_cases()[i]
    torch.library.opcheck(getattr(P, name).default, args, test_utils=("test_schema", "test_faketensor"))


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("case", K.decode_cases(), ids=str)
def test_attn_decode_with_sinks(case):
    """Host, device-scalar and per-row key counts, with and without the window of 64: one split (the fold in the
    workgroup's merge) and several (the combine kernel's extra partial); a count of 0 gives zeros."""
    D, Hq, Hkv, Bb, S, counts, W, fam = case
    inp, ref = K.decode_case(case)
    seqlen = None
    if counts is not None:
        seqlen = torch.tensor([counts] if isinstance(counts, int) else list(counts), dtype=torch.int32, device=DEV)
    o = P.attn_decode(_dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"]), inp["scale"], seqlen, W, _dev(inp["sinks"]))
    K.check("sink_decode_o", o, ref, "o")
    for b, n in enumerate(inp["counts"]):
        if n == 0:
            assert not o[b].any()


def test_attn_decode_plain_path_is_bit_identical():
    inp, _ = A.decode_case((64, 8, 4, 2, 1000, None))
    q, k, v = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"])
    off = torch.full((8,), -math.inf, dtype=BF16, device=DEV)
    for kk, vv in ((k, v), (k[:, :60], v[:, :60])):  # 16 splits / 1 split
        o0 = P.attn_decode(q, kk, vv, inp["scale"])
        assert torch.equal(o0, P.attn_decode(q, kk, vv, inp["scale"], None, 0, None))
        assert torch.equal(o0, P.attn_decode(q, kk, vv, inp["scale"], None, 0, off))


# ------------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "rope-qknorm-bounds"])
def test_attention_ops_with_sinks_match_fp32_reference(D, proj, extras):
    """attention_packed / attention_proj with sinks against ref.attention(sinks=) in fp32 under autograd, with the
    gradients of qkv, W_o and the sinks.  D = 64 with the projection takes delta from the GEMM epilogue, everything
    else from ``delta_out``.  Tolerances of tests/test_qk_norm_gpu.py::test_attention_with_gains_matches_fp32_reference
    (output 1.5e-2, gradients 3e-2, relative Frobenius error); the sink gradient is a sum of the same P dO o products
    as dq and takes its 3e-2."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(43 + D)
    B, T, H, Hkv = 2, 160, 4, 2
    C = H * D
    qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV) * 0.8).bfloat16().requires_grad_()
    sinks = (2.0 + torch.randn(H, device=DEV)).bfloat16().requires_grad_()
    kw, bounds, cos = {}, None, None
    if extras:
        wq = (1 + 0.2 * torch.randn(D, device=DEV)).bfloat16()
        wk = (1 + 0.2 * torch.randn(D, device=DEV)).bfloat16()
        cos, sin = ops.rope_cache(T + 64, D, 10000.0, DEV)
        bounds = ops.window_bounds(B, T, 40, DEV)
        kw = dict(rope_cos=cos, rope_sin=sin, q_norm_weight=wq, k_norm_weight=wk, qk_norm_eps=1e-5, bounds=bounds)
    w = (torch.randn(C, C, device=DEV) * 0.05).bfloat16().requires_grad_() if proj else None
    if proj and D == 64:
        assert ops.attn_proj_ok(qkv, H, Hkv, w, None)  # the fused-projection path: delta from the GEMM
        o = ops.attention_proj(qkv, H, Hkv, w, None, sinks=sinks, **kw)
    else:
        o = ops.attention_packed(qkv, H, Hkv, sinks=sinks, **kw)
        o = ops.linear(o, w, None) if proj else o
    do = torch.randn_like(o)
    o.backward(do)
    qkvf, sf = qkv.detach().float().requires_grad_(), sinks.detach().float().requires_grad_()
    wf = w.detach().float().requires_grad_() if proj else None
    q, k, v = ops._split_qkv(qkvf, H, Hkv, D)
    if extras:
        q = ref.rope(ref.qk_norm(q, wq.float(), 1e-5), cos[:T], sin[:T])
        k = ref.rope(ref.qk_norm(k, wk.float(), 1e-5), cos[:T], sin[:T])
    of = ref.attention(q, k, v, causal=True, scale=1 / math.sqrt(D), bounds=bounds, sinks=sf)[0].reshape(B, T, C)
    if proj:
        of = of @ wf.t()
    of.backward(do.float())
    assert _rel(o, of) < 1.5e-2, _rel(o, of)
    gq, gk, gv = ops._split_qkv(qkv.grad, H, Hkv, D)
    rq, rk, rv = ops._split_qkv(qkvf.grad, H, Hkv, D)
    pairs = [(gq, rq, "q"), (gk, rk, "k"), (gv, rv, "v"), (sinks.grad, sf.grad, "sinks")]
    if proj:
        pairs.append((w.grad, wf.grad, "W_o"))
    for a, b, n in pairs:
        assert _rel(a, b) < 3e-2, (n, _rel(a, b))
    # the sink is in force: its share of the softmax is the reference's
    assert 0.02 < float(torch.exp(sf.detach().view(1, H, 1) - ref.attention(
        q.detach(), k.detach(), v.detach(), causal=True, scale=1 / math.sqrt(D), bounds=bounds,
        sinks=sf.detach())[1]).mean()) < 0.98


# ------------------------------------------------------------------------------------------------ model
def _sinks_model(seed=4, **kw):
    """llama-tiny-sinks with the sinks away from their zero initialisation: a dropped or misplaced sink shows."""
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(seed)
    cfg = get_preset("llama-tiny-sinks")
    cfg = cfg.replace(**kw) if kw else cfg
    m = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("attn.sinks"):
                p.copy_(1.5 + torch.randn_like(p))
    return cfg, m


def test_model_hip_matches_reference_backend():
    """Loss and every parameter gradient (the sinks' among them) on the HIP path against the stock-torch backend
    from the same weights; tolerances of tests/test_sliding_window_gpu.py (loss 2e-2, gradients 6e-2).  With
    activation checkpointing the recompute carries the sink too: the same gradients."""
    from pretraining_llm_amd import ops
    cfg, m = _sinks_model(10)
    assert cfg.attn_sinks and cfg.layer_window(0) == 32 and cfg.layer_window(1) is None
    x = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    y = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    _, l1 = m(x, y, return_logits=False)
    l1.backward()
    g1 = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    names = [n for n in g1 if n.endswith("attn.sinks")]
    assert len(names) == cfg.n_blocks and all(g1[n].abs().sum() > 0 for n in names)
    m.zero_grad()
    with ops.backend("torch"):
        _, l2 = m(x, y)
        l2.backward()
    assert abs(l1.item() - l2.item()) < 2e-2
    g2 = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    for n in g1:
        assert _rel(g1[n], g2[n]) < 6e-2, (n, _rel(g1[n], g2[n]))
    m.zero_grad()
    m.config.activation_checkpointing = True
    m.train()
    assert m.use_checkpointing(x)
    _, l3 = m(x, y, return_logits=False)
    l3.backward()
    assert abs(l3.item() - l2.item()) < 2e-2
    for n, p in m.named_parameters():
        assert _rel(p.grad, g2[n]) < 6e-2, (n, _rel(p.grad, g2[n]))


class _Batches:
    def __init__(self, B, T, V):
        self.B, self.T, self.V, self.i = B, T, V, 0

    def next(self):
        i, self.i = self.i, self.i + 1
        x = torch.randint(0, self.V, (self.B, self.T), generator=torch.Generator().manual_seed(100 + i)).to(DEV)
        return x, torch.roll(x, -1, 1)


def test_trainer_captured_step_and_flat_gradient_slot(tmp_path, monkeypatch):
    """Trainer steps with the captured (hipGraph) step against the eager step from the same seed and batches: loss
    curves within 2e-3 and weights within 1e-3, the bounds of tests/test_sliding_window_gpu.py.  The sink gradient
    sits in the optimizer's fp32 flat-gradient slot (lazy zeroing on: the first write overwrites) and AdamW moves
    the sinks off their zero initialisation."""
    from config.config import default_config
    from pretraining_llm_amd.train.trainer import Trainer
    monkeypatch.delenv("TORCH_COMPILE", raising=False)
    monkeypatch.setenv("PLLM_AB", "lazy_zero=1")
    base = dict(default_config)
    base.update(model_preset="llama-tiny-sinks", t_batch_size=4, seq_len=128, t_train_steps=4, t_lr=1e-3,
                warmup_steps=1, log_interval=1, t_eval_steps=1000, eval_at_start=False, t_out_path=None,
                synthetic_data=True, synthetic_tokens=200_000, synthetic_dir=str(tmp_path), max_grad_norm=1.0,
                device="cuda")
    curves, weights, sinks = {}, {}, {}
    for comp in (True, False):
        recs = []
        tr = Trainer(dict(base, compile=comp), log=lambda *_: None)
        assert tr.mcfg.attn_sinks and (tr.opt.lazy_zero or not comp)
        tr.train_loader = _Batches(4, 128, tr.mcfg.vocab_size)
        tr.metrics.log = recs.append
        slots, zero_grad = {}, tr.opt.zero_grad
        idx = [(i, n) for i, n in enumerate(tr.opt.names) if n.endswith("attn.sinks")]
        assert len(idx) == tr.mcfg.n_blocks

        def snap_then_zero(*a, _tr=tr, _slots=slots, _idx=idx, _zero=zero_grad, **k):
            for i, n in _idx:
                _slots[n] = _tr.opt.grad_view(i).clone()
            return _zero(*a, **k)
        tr.opt.zero_grad = snap_then_zero
        tr.train()
        torch.cuda.synchronize()
        assert tr.use_graph == comp and (tr.gstep is not None) == comp
        for n, g in slots.items():
            assert g.dtype == F32 and g.shape == (tr.mcfg.n_head,) and torch.isfinite(g).all() and g.abs().sum() > 0, n
        curves[comp] = [r["train_loss"] for r in recs]
        weights[comp] = tr.opt.master.clone()
        sinks[comp] = {n: p.detach().float().clone() for n, p in tr.model.named_parameters()
                       if n.endswith("attn.sinks")}
    assert len(curves[True]) == 4 and all(math.isfinite(v) for v in curves[True])
    for a, b in zip(curves[True], curves[False]):
        assert abs(a - b) < 2e-3 * max(1.0, abs(b)), (curves[True], curves[False])
    rel = ((weights[True] - weights[False]).norm() / weights[False].norm()).item()
    assert rel < 1e-3, rel
    for comp in (True, False):
        assert len(sinks[comp]) == 2 and all(s.abs().min() > 0 for s in sinks[comp].values()), sinks[comp]


def test_greedy_generation_is_the_same_on_every_path():
    """Prompt longer than the local layer's window (40 > 32): the uncached recompute, the KV-cache path (prefill +
    one-token steps) and the captured DecodeGraph give the same greedy tokens."""
    cfg, m = _sinks_model(4)
    m.eval()
    idx = torch.randint(0, cfg.vocab_size, (2, 40), generator=torch.Generator().manual_seed(7)).to(DEV)
    a = m.generate(idx, 16, temperature=0.0, use_cache=False)
    b = m.generate(idx, 16, temperature=0.0, use_cache=True)
    c = m.generate(idx, 16, temperature=0.0, use_cache=True, cuda_graph=True)
    assert a.shape == (2, 56)
    assert torch.equal(a, b), (a[:, 40:].tolist(), b[:, 40:].tolist())
    assert torch.equal(b, c), (b[:, 40:].tolist(), c[:, 40:].tolist())
    # the sink is in force on these paths: without it the logits move by far more than bf16 rounding
    from pretraining_llm_amd.models import GPT
    off = GPT(cfg.replace(attn_sinks=False)).to(device=DEV, dtype=torch.bfloat16).eval()
    off.load_state_dict({k: v for k, v in m.state_dict().items() if not k.endswith("attn.sinks")})
    with torch.no_grad():
        assert _rel(off(idx)[0][:, -1], m(idx)[0][:, -1]) > 0.05


def test_continuous_server_matches_generate():
    """Slots at their own positions, most of them past the window; prompt lengths and token counts of
    tests/test_sliding_window_gpu.py."""
    from pretraining_llm_amd.inference.server import ContinuousGenerationServer, GenRequest
    _, model = _sinks_model(4)
    model.eval()
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
    _, model = _sinks_model(4)
    model.eval()
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
