"""QK-norm on the GPU (csrc/qk_norm.hip): ``qk_norm_rope`` and ``qk_norm_bwd_`` against the fp64 references and
budgets of ``_qk_norm_refs.py`` on every case, their contracts (v columns untouched, add / overwrite targets,
determinism, opcheck), the attention ops with gains against fp32 reference math, and the model: HIP path
against the reference backend, the captured training step, and KV-cache / hipGraph decode."""
import math

import pytest
import torch

import _qk_norm_refs as Q

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


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
    qk, rstd = torch.ops.pllm.qk_norm_rope(_dev(inp["qkv"]), _dev(inp["wq"]), _dev(inp["wk"]), inp["eps"], inp["H"],
                                           inp["Hkv"], _dev(inp["cos"]), _dev(inp["sin"]), inp["T"], inp["pos"])
    return dict(y=qk, rstd=rstd)


def _bwd(inp):
    """Both forms of the op on a case; also checks what the references do not: the v columns, overwrite vs add
    and run-to-run determinism."""
    H, Hkv, D = inp["H"], inp["Hkv"], inp["D"]
    nqk = (H + Hkv) * D
    qkv, wq, wk, rstd = _dev(inp["qkv"]), _dev(inp["wq"]), _dev(inp["wk"]), _dev(Q.rstd32(inp))
    run = lambda d, tq, tk, ow: torch.ops.pllm.qk_norm_bwd_(d, qkv, rstd, wq, wk, H, Hkv, tq, tk, ow)  # noqa: E731
    d1 = _dev(inp["dqkv"]).clone()
    dwq, dwk = run(d1, None, None, False)
    assert dwq.dtype == BF16 and dwq.shape == (D,) and dwk.shape == (D,)
    assert torch.equal(d1[:, nqk:], _dev(inp["dqkv"])[:, nqk:]), "v columns of dqkv changed"
    # accumulate into pre-filled fp32 targets
    d2 = _dev(inp["dqkv"]).clone()
    tq, tk = _dev(inp["fill"][0]).clone(), _dev(inp["fill"][1]).clone()
    e = run(d2, tq, tk, False)
    assert e[0].numel() == 0 and e[1].numel() == 0
    assert torch.equal(d1, d2), "dx differs between the fresh and the accumulating form"
    # overwrite into garbage == add into zeros, bit for bit; and a second call gives the same bits
    d3, d4 = _dev(inp["dqkv"]).clone(), _dev(inp["dqkv"]).clone()
    gq, gk = torch.full((D,), math.nan, device=DEV), torch.full((D,), -7e30, device=DEV)
    zq, zk = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    run(d3, gq, gk, True)
    run(d4, zq, zk, False)
    assert torch.equal(gq, zq) and torch.equal(gk, zk), "overwrite into garbage != add into zeros"
    assert torch.equal(d3, d1) and torch.equal(d4, d1), "dx is not deterministic"
    d5 = _dev(inp["dqkv"]).clone()
    dwq2, dwk2 = run(d5, None, None, False)
    assert torch.equal(dwq2, dwq) and torch.equal(dwk2, dwk) and torch.equal(d5, d1), "not deterministic"
    return dict(dx=d1[:, :nqk], dwq=dwq, dwk=dwk, dwq_acc=tq, dwk_acc=tk)


@pytest.mark.parametrize("case", Q.cases(), ids=Q.case_id)
def test_kernels_match_fp64_reference(case):
    inp = Q.inputs(**case)
    Q.check_all(Q.fwd_checks(inp, _fwd(inp)))
    Q.check_all(Q.bwd_checks(inp, _bwd(inp)))


def test_backward_many_grid_passes():
    """BIG_ROWS rows at (H, Hkv, D) = (2, 1, 32): every workgroup of the backward's capped grid accumulates its
    gain partials over 8-9 iterations, the last one ragged."""
    inp = Q.inputs(**Q.BIG)
    Q.check_all(Q.bwd_checks(inp, _bwd(inp)))


def test_identities():
    """No tables and all-ones gains at D = 64: qk is the normalised input, bit for bit with an fp32 torch
    evaluation up to the reduction's rounding (checked under the budget against fp64); with tables and QK-norm
    off, rope_qk's output is what it was (the rope op on the same rows)."""
    from pretraining_llm_amd import ops
    torch.manual_seed(3)
    B, T, H, Hkv, D = 2, 37, 4, 2, 64
    qkv = torch.randn(B * T, (H + 2 * Hkv) * D).to(BF16)
    ones = torch.ones(D).to(BF16)
    inp = dict(qkv=qkv, wq=ones, wk=ones, cos=None, sin=None, D=D, H=H, Hkv=Hkv, T=T, pos=0, eps=Q.EPS)
    out = _fwd(inp)
    Q.check_all(Q.fwd_checks(inp, out))
    x = Q._heads(qkv, H, Hkv, D, torch.float64)
    xn = x / (x.pow(2).mean(-1, keepdim=True) + Q.EPS).sqrt()
    assert _rel(out["y"].cpu(), xn.reshape(B * T, -1)) < 4e-3  # bf16 rounding of unit-RMS values
    # qk_norm off: the RoPE pre-pass is rope_qk as before
    cos, sin = ops.rope_cache(T + 8, D, 10000.0, DEV)
    q3 = qkv.to(DEV).view(B, T, -1)
    a = torch.ops.pllm.rope_qk(q3, cos, sin, H + 2 * Hkv, H + Hkv, T)
    b = torch.ops.pllm.rope(q3, cos, sin, H + 2 * Hkv, H + Hkv, T, 0, False)[..., : (H + Hkv) * D]
    assert torch.equal(a, b)
    o1 = ops.attention_packed(q3, H, Hkv, rope_cos=cos, rope_sin=sin)
    qk = ops._attn_packed_fwd(q3, H, Hkv, True, 1 / math.sqrt(D), cos, sin)[0]
    assert torch.equal(qk, a) and torch.isfinite(o1).all()


def test_host_checks_reject_bad_shapes():
    r = lambda *s: torch.randn(*s, device=DEV).to(BF16)  # noqa: E731
    op = torch.ops.pllm.qk_norm_rope
    with pytest.raises(RuntimeError, match="head dim"):
        op(r(4, 3 * 48), r(48), r(48), 1e-5, 1, 1, None, None, 4, 0)
    with pytest.raises(RuntimeError, match="multiple of T"):
        op(r(5, 3 * 64), r(64), r(64), 1e-5, 1, 1, None, None, 4, 0)
    tab = torch.rand(4, 32, device=DEV)
    with pytest.raises(RuntimeError, match="table shape"):
        op(r(4, 3 * 64), r(64), r(64), 1e-5, 1, 1, tab, tab, 4, 1)
    with pytest.raises(RuntimeError, match="bfloat16"):
        op(r(4, 3 * 64).float(), r(64), r(64), 1e-5, 1, 1, None, None, 4, 0)
    with pytest.raises(RuntimeError, match="rstd"):
        torch.ops.pllm.qk_norm_bwd_(r(4, 3 * 64), r(4, 3 * 64), torch.ones(4, 3, device=DEV), r(64), r(64), 1, 1,
                                    None, None, False)


def _opcheck_cases():
    r = lambda *s: torch.randn(*s, device=DEV).to(BF16)  # noqa: E731
    B, T, H, Hkv, D = 2, 16, 4, 2, 64
    W = (H + 2 * Hkv) * D
    cos, sin = (t.contiguous() for t in (torch.rand(T + 3, D // 2, device=DEV),) * 2)
    rstd = torch.rand(B * T, H + Hkv, device=DEV) + 0.5
    return [
        ("qk_norm_rope", (r(B, T, W), r(D), r(D), 1e-5, H, Hkv, cos, sin, T, 3)),
        ("qk_norm_rope", (r(B * T, W), r(D), r(D), 1e-5, H, Hkv, None, None, T, 0)),
        ("qk_norm_bwd_", (r(B, T, W), r(B, T, W), rstd, r(D), r(D), H, Hkv, None, None, False)),
        ("qk_norm_bwd_", (r(B, T, W), r(B, T, W), rstd, r(D), r(D), H, Hkv, torch.zeros(D, device=DEV),
                          torch.zeros(D, device=DEV), False)),
        ("qk_norm_bwd_", (r(B, T, W), r(B, T, W), rstd, r(D), r(D), H, Hkv, torch.zeros(D, device=DEV),
                          torch.zeros(D, device=DEV), True)),
    ]


@pytest.mark.parametrize("i", range(5))
def test_opcheck_fake_matches_kernel(i):
    torch.manual_seed(i)
    name, args = _opcheck_cases()[i]
    torch.library.opcheck(getattr(torch.ops.pllm, name).default, args, test_utils=("test_schema", "test_faketensor"))


# ------------------------------------------------------------------------------------------------ attention ops
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("proj", [False, True])
def test_attention_with_gains_matches_fp32_reference(D, proj):
    """attention_packed / attention_proj with gains against ref.qk_norm -> ref.rope -> ref.attention in fp32 under
    autograd.  Tolerances as tests/test_kernels_gpu.py::test_attention_fused_rope_fwd_bwd for the same
    quantities: output 1.5e-2, dq / dk / dv 3e-2 (relative Frobenius error); the gain gradients are sums of the
    same products as dq / dk and take their 3e-2."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(41 + D)
    B, T, H, Hkv = 2, 160, 4, 2
    C = H * D
    qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV) * 0.8).bfloat16().requires_grad_()
    wq = (1 + 0.2 * torch.randn(D, device=DEV)).bfloat16().requires_grad_()
    wk = (1 + 0.2 * torch.randn(D, device=DEV)).bfloat16().requires_grad_()
    cos, sin = ops.rope_cache(T + 64, D, 10000.0, DEV)
    kw = dict(rope_cos=cos, rope_sin=sin, q_norm_weight=wq, k_norm_weight=wk, qk_norm_eps=1e-5)
    if proj:
        w = (torch.randn(C, C, device=DEV) * 0.05).bfloat16().requires_grad_()
        if D == 64:
            assert ops.attn_proj_ok(qkv, H, Hkv, w, None)  # the fused-projection path
            o = ops.attention_proj(qkv, H, Hkv, w, None, **kw)
        else:
            o = ops.linear(ops.attention_packed(qkv, H, Hkv, **kw), w, None)
    else:
        o = ops.attention_packed(qkv, H, Hkv, **kw)
    do = torch.randn_like(o)
    o.backward(do)
    qkvf = qkv.detach().float().requires_grad_()
    wqf, wkf = wq.detach().float().requires_grad_(), wk.detach().float().requires_grad_()
    q, k, v = ops._split_qkv(qkvf, H, Hkv, D)
    qr = ref.rope(ref.qk_norm(q, wqf, 1e-5), cos[:T], sin[:T])
    kr = ref.rope(ref.qk_norm(k, wkf, 1e-5), cos[:T], sin[:T])
    of = ref.attention(qr, kr, v, causal=True, scale=1 / math.sqrt(D))[0].reshape(B, T, C)
    if proj:
        of = of @ w.detach().float().t()
    of.backward(do.float())
    assert _rel(o, of) < 1.5e-2, _rel(o, of)
    gq, gk, gv = ops._split_qkv(qkv.grad, H, Hkv, D)
    rq, rk, rv = ops._split_qkv(qkvf.grad, H, Hkv, D)
    for a, b, n in ((gq, rq, "q"), (gk, rk, "k"), (gv, rv, "v"), (wq.grad, wqf.grad, "wq"), (wk.grad, wkf.grad, "wk")):
        assert _rel(a, b) < 3e-2, (n, _rel(a, b))


def test_qk_norm_packed_standalone_gradients():
    """The stand-alone op (decode / direct use): outputs and gradients against autograd through the reference."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import reference as ref
    torch.manual_seed(5)
    B, T, H, Hkv, D, pos = 2, 19, 4, 2, 32, 4
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device=DEV).bfloat16().requires_grad_()
    wq = (1 + 0.2 * torch.randn(D, device=DEV)).bfloat16().requires_grad_()
    wk = (1 + 0.2 * torch.randn(D, device=DEV)).bfloat16().requires_grad_()
    cos, sin = ops.rope_cache(T + pos, D, 10000.0, DEV)
    q, k = ops.qk_norm_packed(qkv, wq, wk, 1e-5, H, Hkv, cos, sin, pos)
    dq, dk = torch.randn_like(q), torch.randn_like(k)
    torch.autograd.backward([q, k], [dq, dk])
    qkvf = qkv.detach().float().requires_grad_()
    wqf, wkf = wq.detach().float().requires_grad_(), wk.detach().float().requires_grad_()
    q0, k0, _ = ops._split_qkv(qkvf, H, Hkv, D)
    qf = ref.rope(ref.qk_norm(q0, wqf, 1e-5), cos[pos:pos + T], sin[pos:pos + T])
    kf = ref.rope(ref.qk_norm(k0, wkf, 1e-5), cos[pos:pos + T], sin[pos:pos + T])
    torch.autograd.backward([qf, kf], [dq.float(), dk.float()])
    for a, b, n in ((q, qf, "q"), (k, kf, "k"), (qkv.grad, qkvf.grad, "dqkv"), (wq.grad, wqf.grad, "dwq"),
                    (wk.grad, wkf.grad, "dwk")):
        assert _rel(a, b) < 1e-2, (n, _rel(a, b))  # bf16 outputs: 2^-8 relative per element
    assert not qkv.grad[..., (H + Hkv) * D:].any()


# ------------------------------------------------------------------------------------------------ model
def _qkn_cfg(name):
    from pretraining_llm_amd.models import get_preset
    if name == "gpt2-tiny":
        return get_preset("gpt2-tiny").replace(qk_norm=True)
    return get_preset(name)


@pytest.mark.parametrize("name", ["llama-tiny-qknorm", "gpt2-tiny"])
def test_model_hip_matches_reference_backend(name):
    """Loss and every parameter gradient on the HIP path against the stock-torch backend from the same weights;
    tolerances of tests/test_kernels_gpu.py::test_model_hip_matches_reference_path (loss 2e-2, gradients 6e-2)."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT
    torch.manual_seed(10)
    cfg = _qkn_cfg(name).replace(context_length=128)
    m = GPT(cfg).to(DEV, torch.bfloat16)
    with torch.no_grad():  # gains away from 1, so that a dropped or swapped gain shows
        for n, p in m.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                p.add_(0.3 * torch.randn_like(p))
    x = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    y = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    _, l1 = m(x, y, return_logits=False)
    l1.backward()
    g1 = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    assert any("q_norm" in n for n in g1) and any("k_norm" in n for n in g1)
    m.zero_grad()
    with ops.backend("torch"):
        _, l2 = m(x, y)
        l2.backward()
    assert abs(l1.item() - l2.item()) < 2e-2
    for n, p in m.named_parameters():
        assert _rel(g1[n], p.grad) < 6e-2, (n, _rel(g1[n], p.grad))


@pytest.mark.parametrize("name", ["llama-tiny-qknorm", "gpt2-tiny"])
def test_trainer_captured_step(name, tmp_path, monkeypatch):
    """Trainer steps with the captured (hipGraph) step and lazy zeroing (one eager warm-up step, then two
    replays): finite loss, non-zero q_norm / k_norm flat-gradient slots, bitwise equal across two runs from the
    same seed.  The step ends with zero_grad, so the slots are copied out just before it (the copies are part
    of the captured step: every replay refreshes them)."""
    from config.config import default_config
    from pretraining_llm_amd.train.trainer import Trainer
    monkeypatch.delenv("TORCH_COMPILE", raising=False)
    monkeypatch.setenv("PLLM_AB", "lazy_zero=1")
    base = dict(default_config)
    base.update(model_preset=name, t_batch_size=4, seq_len=128, t_train_steps=3, t_lr=1e-3, warmup_steps=1,
                log_interval=1, t_eval_steps=1000, eval_at_start=False, t_out_path=None, synthetic_data=True,
                synthetic_tokens=200_000, synthetic_dir=str(tmp_path), max_grad_norm=1.0, device="cuda",
                compile=True)
    if name == "gpt2-tiny":
        base.update(qk_norm=True)
    runs = []
    for _ in range(2):
        recs = []
        tr = Trainer(dict(base), log=lambda *_: None)
        assert tr.mcfg.qk_norm and tr.opt.lazy_zero
        tr.metrics.log = recs.append
        slots, zero_grad = {}, tr.opt.zero_grad
        gains = [(i, n) for i, n in enumerate(tr.opt.names) if "q_norm" in n or "k_norm" in n]

        def snap_then_zero(*a, _tr=tr, _slots=slots, _gains=gains, _zero=zero_grad, **k):
            for i, n in _gains:
                _slots[n] = _tr.opt.grad_view(i).clone()
            return _zero(*a, **k)
        tr.opt.zero_grad = snap_then_zero
        tr.train()
        torch.cuda.synchronize()
        assert tr.use_graph and tr.gstep is not None
        losses = [r["train_loss"] for r in recs]
        assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
        slots = {n: g.clone() for n, g in slots.items()}
        assert len(slots) == 2 * tr.mcfg.n_blocks
        for n, g in slots.items():
            assert g.dtype == F32 and torch.isfinite(g).all() and g.abs().sum() > 0, n
        runs.append((losses, slots, tr.opt.master.clone()))
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    assert torch.equal(runs[0][2], runs[1][2])


# ------------------------------------------------------------------------------------------------ decode
def _tiny_qkn_model():
    from pretraining_llm_amd.models import GPT, get_preset
    cfg = get_preset("llama-tiny-qknorm").replace(vocab_size=256, context_length=64)
    m = GPT(cfg).to(DEV, torch.bfloat16).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                p.add_(0.3 * torch.randn_like(p))
    return cfg, m


def test_kv_cache_generation_matches_recompute():
    """tests/test_models.py::test_kv_cache_generation_matches_recompute on llama-tiny-qknorm, on the GPU: the
    cached prefill and decode steps produce full-recompute logits (bf16: compared, not argmax-tied)."""
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached
    torch.manual_seed(3)
    cfg, m = _tiny_qkn_model()
    idx = torch.randint(0, 256, (2, 12), device=DEV)
    cache = KVCache(cfg.n_blocks, 2, 64, cfg.n_kv_head, cfg.head_dim, torch.bfloat16, DEV)
    with torch.no_grad():
        forward_cached(m, idx[:, :9], cache, 0)
        for t in range(9, 12):
            a = forward_cached(m, idx[:, t:t + 1], cache, t)
            b = m(idx[:, :t + 1])[0][:, -1].float()
            assert _rel(a, b) < 2e-2, (t, _rel(a, b))
    out = m.generate(idx[:, :5], 10, temperature=0.0, use_cache=True)
    assert out.shape == (2, 15)


def test_device_position_decode_and_graph_replay():
    """forward_decode (device position) against the host-position KV-cache step, as
    tests/test_models.py::test_device_position_decode_step_matches_cached, then a DecodeGraph with per-row
    positions replayed at three positions against the eager step: K is normalised before it is cached."""
    from pretraining_llm_amd.inference.generate import DecodeGraph, KVCache, forward_cached, forward_decode
    torch.manual_seed(6)
    cfg, m = _tiny_qkn_model()
    B = 2
    idx = torch.randint(0, 256, (B, 12), device=DEV)
    mk = lambda: KVCache(cfg.n_blocks, B, 64, cfg.n_kv_head, cfg.head_dim, torch.bfloat16, DEV)  # noqa: E731
    c1, c2, c3 = mk(), mk(), mk()
    for c in (c1, c2, c3):
        for t in c.k + c.v:
            t.zero_()
        forward_cached(m, idx[:, :6], c, 0)
    a = forward_cached(m, idx[:, 6:7], c1, 6)
    b = forward_decode(m, idx[:, 6:7], c2, torch.tensor([6], device=DEV), torch.tensor([7], dtype=torch.int32,
                                                                                      device=DEV))
    assert torch.allclose(a, b, atol=2e-2, rtol=2e-2)
    # the cached K is the normalised, rotated one, the same from both steps (layer 0: bit for bit; layer 1 sees
    # the two attention kernels' different summation orders)
    assert torch.equal(c1.k[0][:, :7], c2.k[0][:, :7])
    assert torch.allclose(c1.k[1][:, :7].float(), c2.k[1][:, :7].float(), atol=2e-2, rtol=2e-2)
    # normalised keys have RMS ~ 1 (gains 1 +- 0.3); the raw projection's are ~ 0.02 sqrt(C) at init
    assert abs(c1.k[0][:, :7].float().pow(2).mean().sqrt().item() - 1.0) < 0.3
    # per-row positions, captured once, replayed at three positions: row 1 runs one position behind row 0
    for c in (c2, c3):
        for t in c.k + c.v:
            t.zero_()
        forward_cached(m, idx[:, :6], c, 0)
    graph = DecodeGraph(m, c3, B, torch.device(DEV, 0), per_row=True)
    for t in c3.k + c3.v:  # the capture's warm-up wrote at position 0: restore the prefill
        t.zero_()
    forward_cached(m, idx[:, :6], c3, 0)
    for step in range(3):
        pos = torch.tensor([6 + step, 5 + step], device=DEV)
        tok = torch.stack([idx[0, 6 + step], idx[1, 5 + step]]).view(B, 1)
        e = forward_decode(m, tok, c2, pos, (pos + 1).int())
        g = graph(tok, pos).clone()
        assert torch.equal(e, g), step
        assert torch.equal(c2.k[0], c3.k[0]) and torch.equal(c2.k[1], c3.k[1])
        if step == 0:  # row 0 at position 6: the single-position step above
            assert torch.allclose(e[0], a[0], atol=2e-2, rtol=2e-2)
