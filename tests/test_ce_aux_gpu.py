"""The fused cross-entropy with z-loss and final-logit soft-capping on the GPU (``cross_entropy_aux``,
csrc/cross_entropy.hip): every case of ``_ce_aux_refs`` element by element against its fp64 reference under the
budgets calibrated in ``test_ce_aux_refs.py``, the op's contracts, the chunked LM head, and the model: HIP path
against the reference backend, the captured training step and KV-cache / hipGraph decode with the cap on.

Each kernel case is 6 rows.  The figures a case needs are printed before it asserts (``pytest -s``)."""
import math

import pytest
import torch
import torch.nn.functional as F

import _ce_aux_refs as A
import _streaming_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _ops():
    return torch.ops.pllm


def _d(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _run(inp, variant, z, c, inv_n=None, grad=True):
    """-> loss, lse, dlogits; ``variant`` as tests/test_streaming_edges_gpu.py::_ce_run: dlogits aliasing logits, a
    separate NaN-poisoned buffer, or column slices of NaN-padded buffers."""
    lg, t = _d(inp["logits"]), _d(inp["targets"])
    N, V = lg.shape
    inv = None if inv_n is None else torch.tensor([inv_n], device=DEV, dtype=F32)
    lse = torch.full((N,), math.nan, device=DEV, dtype=F32)
    if not grad:
        keep = lg.clone()
        loss = _ops().cross_entropy_aux(lg, t, None, R.IGNORE, inv, z, c, lse)
        assert torch.equal(_bits(lg), _bits(keep)), "logits changed"
        return loss, lse, None
    if variant == "alias":
        dl = lg.clone()
        return _ops().cross_entropy_aux(dl, t, dl, R.IGNORE, inv, z, c, lse), lse, dl
    if variant == "separate":
        dl = torch.full_like(lg, math.nan)
        keep = lg.clone()
        loss = _ops().cross_entropy_aux(lg, t, dl, R.IGNORE, inv, z, c, lse)
        assert torch.equal(_bits(lg), _bits(keep)), "logits changed"
        return loss, lse, dl
    src = torch.full((N, V + 24), math.nan, device=DEV, dtype=BF16)
    dst = torch.full((N, V + 24), math.nan, device=DEV, dtype=BF16)
    src[:, :V] = lg
    pad_src, pad_dst = _bits(src[:, V:]).clone(), _bits(dst[:, V:]).clone()
    loss = _ops().cross_entropy_aux(src[:, :V], t, dst[:, :V], R.IGNORE, inv, z, c, lse)
    assert torch.equal(_bits(src[:, V:]), pad_src) and torch.equal(_bits(dst[:, V:]), pad_dst), "padding written"
    assert torch.equal(_bits(src[:, :V]), _bits(lg)), "logits changed"
    return loss, lse, dst[:, :V]


def _check(inp, loss, lse, dl, z, c, inv_n=None, what=""):
    items = A.checks(inp, dict(loss=loss, lse=lse, dlogits=dl), z, c, inv_n)
    print(f"ce_aux {what}: budget needed {A.needed(items)} of {({k: v[1] for k, v in A.BUDGET.items()})}")
    A.check_all(items)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("variant", ["alias", "separate", "strided"])
@pytest.mark.parametrize("case", A.cases(), ids=A.case_id)
def test_cross_entropy_aux_edges(case, variant):
    z, c, V = case
    inp = R.ce_inputs(V)
    loss, lse, dl = _run(inp, variant, z, c)
    _check(inp, loss, lse, dl, z, c, what=f"{A.case_id(case)}/{variant}")
    assert lse[-1].item() == 0 and loss[-1].item() == 0 and not dl[-1].float().any()  # the ignored row
    assert torch.isfinite(dl.float()).all() and torch.isfinite(loss).all() and torch.isfinite(lse).all()


@pytest.mark.parametrize("z,c", [(0.5, 0.0), (0.5, 2.0)])
@pytest.mark.parametrize("V", [8, 4104, 131072])
def test_forward_only_explicit_inv_n_and_determinism(V, z, c):
    inp = R.ce_inputs(V)
    loss, lse, dl = _run(inp, "separate", z, c, inv_n=0.125)
    _check(inp, loss, lse, dl, z, c, inv_n=0.125, what=f"V{V} inv_n=0.125")
    # the forward-only form gives the training form's loss and lse bit for bit
    loss_f, lse_f, _ = _run(inp, None, z, c, grad=False)
    assert torch.equal(_bits(loss_f), _bits(loss)) and torch.equal(_bits(lse_f), _bits(lse))
    # without the lse output too
    loss_n = _ops().cross_entropy_aux(_d(inp["logits"]), _d(inp["targets"]), None, R.IGNORE, None, z, c, None)
    assert torch.equal(_bits(loss_n), _bits(loss))
    # the default inv_n is the explicit one at 1 / #valid, and two calls give the same bits
    n_valid = int((inp["targets"] != R.IGNORE).sum())
    a = _run(inp, "separate", z, c)
    b = _run(inp, "separate", z, c, inv_n=1.0 / n_valid)
    a2 = _run(inp, "separate", z, c)
    for u, v, w in zip(a, b, a2):
        assert torch.equal(_bits(u), _bits(v)) and torch.equal(_bits(u), _bits(w))


@pytest.mark.parametrize("variant", ["alias", "strided"])
def test_all_rows_ignored(variant):
    inp = R.ce_inputs(4104, all_ignored=True)
    loss, lse, dl = _run(inp, variant, 0.5, 2.0)  # inv_n = 1 / max(#valid, 1): clamped, nothing is NaN
    assert not loss.any() and not lse.any() and not dl.float().any()
    _check(inp, loss, lse, dl, 0.5, 2.0, what="all ignored")


@pytest.mark.parametrize("V", [8, 4104, 131072])
def test_both_off_is_the_plain_kernel_bit_for_bit(V):
    """z_loss = 0, softcap = 0: the shared arithmetic is the plain kernel's (loss, dlogits), and lse is loss + x_t."""
    inp = R.ce_inputs(V)
    lg, t = _d(inp["logits"]), _d(inp["targets"])
    d0, d1 = torch.full_like(lg, math.nan), torch.full_like(lg, math.nan)
    l0 = _ops().cross_entropy(lg, t, d0, R.IGNORE, None)
    lse = torch.empty(lg.shape[0], device=DEV, dtype=F32)
    l1 = _ops().cross_entropy_aux(lg, t, d1, R.IGNORE, None, 0.0, 0.0, lse)
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(d0), _bits(d1))
    assert torch.equal(_bits(_ops().cross_entropy(lg, t, None, R.IGNORE, None)),
                       _bits(_ops().cross_entropy_aux(lg, t, None, R.IGNORE, None, 0.0, 0.0, None)))
    R.check_all(R.ce_checks(inp, dict(loss=l1, dlogits=d1)))


def test_host_checks_and_opcheck():
    lg = torch.randn(6, 4104, device=DEV).to(BF16)
    t = torch.randint(0, 4104, (6,), device=DEV)
    op = _ops().cross_entropy_aux
    with pytest.raises(RuntimeError, match="z_loss"):
        op(lg, t, None, R.IGNORE, None, -1e-4, 0.0, None)
    with pytest.raises(RuntimeError, match="softcap"):
        op(lg, t, None, R.IGNORE, None, 0.0, -30.0, None)
    with pytest.raises(RuntimeError, match="lse"):
        op(lg, t, None, R.IGNORE, None, 1e-4, 0.0, torch.empty(5, device=DEV))
    with pytest.raises(RuntimeError, match="lse"):
        op(lg, t, None, R.IGNORE, None, 1e-4, 0.0, torch.empty(6, device=DEV, dtype=BF16))
    with pytest.raises(RuntimeError, match="lse"):
        op(lg, t, None, R.IGNORE, None, 1e-4, 0.0, torch.empty(6, 1, device=DEV))
    with pytest.raises(RuntimeError, match="multiples of 8"):
        op(lg[:, :4100], t, None, R.IGNORE, None, 1e-4, 0.0, None)
    with pytest.raises(RuntimeError, match="vocab too large"):
        op(torch.zeros(1, _ops().cross_entropy_max_vocab() + 8, device=DEV, dtype=BF16), t[:1], None, R.IGNORE, None,
           1e-4, 30.0, None)
    with pytest.raises(RuntimeError, match="dlogits layout"):
        op(lg, t, torch.empty(6, 4112, device=DEV, dtype=BF16)[:, :4104], R.IGNORE, None, 1e-4, 0.0, None)
    inv = torch.full((1,), 0.2, device=DEV)
    for args in ((lg, t, None, R.IGNORE, None, 1e-4, 30.0, None),
                 (lg.clone(), t, torch.empty_like(lg), R.IGNORE, inv, 0.5, 2.0, torch.empty(6, device=DEV))):
        torch.library.opcheck(op.default, args, test_utils=("test_schema", "test_faketensor"))


# ------------------------------------------------------------------------------------------------ LM head
@pytest.mark.parametrize("with_bias", [False, True])
def test_lm_head_ce_chunked_with_options(with_bias, monkeypatch):
    """Both options through the chunked LM head (3 row chunks of 128, the last ragged) against fp32 torch autograd of
    the formula; tolerances of tests/test_kernels_gpu.py::test_lm_head_ce_chunked (loss 3e-3 relative, gradients
    3e-2 relative Frobenius error).  z = 0.05 makes the z term's share of the gradient about a quarter."""
    from pretraining_llm_amd import ops
    monkeypatch.setattr(ops, "CE_CHUNK_ROWS", 128)
    torch.manual_seed(28)
    N, C, V, z, c = 300, 128, 4104, 0.05, 3.0
    h = (torch.randn(N, C, device=DEV) * 0.5).bfloat16().requires_grad_()
    W = (torch.randn(V, C, device=DEV) * 0.3).bfloat16().requires_grad_()
    b = (torch.randn(V, device=DEV) * 0.1).bfloat16().requires_grad_() if with_bias else None
    t = torch.randint(0, V, (N,), device=DEV)
    t[::5] = -100
    zt = torch.full((1,), math.nan, device=DEV)
    loss = ops.lm_head_cross_entropy(h, W, b, t, z_loss=z, softcap=c, z_out=zt)
    (loss * 0.5).backward()
    hf, Wf = h.detach().float().requires_grad_(), W.detach().float().requires_grad_()
    bf = b.detach().float().requires_grad_() if with_bias else None
    logits = hf @ Wf.t() + (bf if with_bias else 0)
    y = c * torch.tanh(logits / c)
    valid = (t != -100).float()
    zterm = z * (torch.logsumexp(y, -1).square() * valid).sum() / valid.sum()
    lf = F.cross_entropy(y, t, ignore_index=-100) + zterm
    (lf * 0.5).backward()
    assert (logits.detach().abs() > c).float().mean() > 0.05  # the cap bites
    assert abs(loss.item() - lf.item()) < 3e-3 * lf.item(), (loss.item(), lf.item())
    assert abs(zt.item() - zterm.item()) < 3e-3 * zterm.item() and zterm.item() > 0.1 * lf.item()
    assert _rel(h.grad, hf.grad) < 3e-2, _rel(h.grad, hf.grad)
    assert _rel(W.grad, Wf.grad) < 3e-2, _rel(W.grad, Wf.grad)
    if with_bias:
        assert _rel(b.grad, bf.grad) < 3e-2, _rel(b.grad, bf.grad)
    with torch.no_grad():  # the no-grad chunked path and the whole-logits path
        zt2 = torch.full((1,), math.nan, device=DEV)
        le = ops.lm_head_cross_entropy(h, W, b, t, z_loss=z, softcap=c, z_out=zt2)
        lw = ops.cross_entropy(F.linear(h, W, b), t, z_loss=z, softcap=c)
    assert abs(le.item() - loss.item()) < 1e-4 * loss.item() and abs(lw.item() - loss.item()) < 1e-4 * loss.item()
    assert abs(zt2.item() - zt.item()) < 1e-4 * zt.item()


# ------------------------------------------------------------------------------------------------ model
def _zl_cfg(**kw):
    from pretraining_llm_amd.models import get_preset
    return get_preset("llama-tiny-zloss").replace(**kw)


def _hot_head(m, gain=60.0):
    with torch.no_grad():  # logits past the cap (30) and a z term that shows
        m.lm_head.weight.mul_(gain)


def test_model_hip_matches_reference_backend():
    """Loss and every parameter gradient on the HIP path against the stock-torch backend from the same weights, with
    z_loss raised to 1e-2 so that the term carries weight; bounds of
    tests/test_qk_norm_gpu.py::test_model_hip_matches_reference_backend (loss 2e-2, gradients 6e-2)."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT
    torch.manual_seed(10)
    cfg = _zl_cfg(context_length=128, z_loss=1e-2)
    m = GPT(cfg).to(DEV, torch.bfloat16)
    _hot_head(m)
    x = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    y = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV)
    _, l1 = m(x, y, return_logits=False)
    l1.backward()
    z1 = m.z_term.clone()
    g1 = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    m.zero_grad()
    with ops.backend("torch"):
        lg, l2 = m(x, y)
        l2.backward()
    assert lg.abs().max() <= 30.0 and lg.abs().max() > 25.0  # handed out capped, and the cap bites
    assert abs(l1.item() - l2.item()) < 2e-2, (l1.item(), l2.item())
    assert z1.item() > 0.05 and abs(z1.item() - m.z_term.item()) < 2e-2
    for n, p in m.named_parameters():
        assert _rel(g1[n], p.grad) < 6e-2, (n, _rel(g1[n], p.grad))
    # eval: plain CE of the capped logits on both return paths
    m.eval()
    with torch.no_grad():
        le = m(x, y, return_logits=False)[1]
        lg_e, le2 = m(x, y)
        ce = F.cross_entropy(lg_e.float().reshape(-1, cfg.vocab_size), y.reshape(-1))
    assert abs(le.item() - ce.item()) < 2e-2 and abs(le2.item() - ce.item()) < 2e-2
    assert l1.item() - le.item() > 0.5 * z1.item()


def test_trainer_captured_step_refreshes_the_z_term(tmp_path, monkeypatch):
    """Trainer steps with the captured (hipGraph) step on llama-tiny-zloss (one eager warm-up step, then replays)
    against the same steps run eagerly: the same losses, and the logged z_loss follows them step by step -- a replay
    refreshes the model's z-term tensor."""
    from config.config import default_config
    from pretraining_llm_amd.train.trainer import Trainer
    monkeypatch.delenv("TORCH_COMPILE", raising=False)
    base = dict(default_config)
    base.update(model_preset="llama-tiny-zloss", z_loss=1e-2, t_batch_size=4, seq_len=128, t_train_steps=4, t_lr=3e-3,
                warmup_steps=1, log_interval=1, t_eval_steps=1000, eval_at_start=False, t_out_path=None,
                synthetic_data=True, synthetic_tokens=200_000, synthetic_dir=str(tmp_path), max_grad_norm=1.0,
                device="cuda")
    runs = {}
    for graphed in (True, False):
        recs = []
        tr = Trainer(dict(base, compile=graphed), log=lambda *_: None)
        tr.metrics.log = recs.append
        tr.train()
        torch.cuda.synchronize()
        assert tr.use_graph == graphed and (tr.gstep is not None) == graphed
        runs[graphed] = recs
    for a, b in zip(runs[True], runs[False]):
        assert math.isfinite(a["train_loss"]) and 0 < a["z_loss"] < a["train_loss"]
        # the two step implementations differ in kernel order only (lazy zeroing, fused clipping): bf16-level noise
        assert abs(a["train_loss"] - b["train_loss"]) < 2e-2, (a, b)
        assert abs(a["z_loss"] - b["z_loss"]) < 2e-2 * b["z_loss"] + 1e-4, (a, b)
    zs = [r["z_loss"] for r in runs[True]]
    assert len(zs) == 4 and len(set(zs[1:])) == 3, zs  # replays 2..4 each logged their own z term


def _tiny_capped_model():
    from pretraining_llm_amd.models import GPT
    cfg = _zl_cfg(vocab_size=256, context_length=64)
    m = GPT(cfg).to(DEV, torch.bfloat16).eval()
    _hot_head(m)
    return cfg, m


def test_kv_cache_generation_matches_recompute():
    """tests/test_qk_norm_gpu.py::test_kv_cache_generation_matches_recompute with the cap on and biting."""
    from pretraining_llm_amd.inference.generate import KVCache, forward_cached
    torch.manual_seed(3)
    cfg, m = _tiny_capped_model()
    idx = torch.randint(0, 256, (2, 12), device=DEV)
    cache = KVCache(cfg.n_blocks, 2, 64, cfg.n_kv_head, cfg.head_dim, torch.bfloat16, DEV)
    with torch.no_grad():
        forward_cached(m, idx[:, :9], cache, 0)
        for t in range(9, 12):
            a = forward_cached(m, idx[:, t:t + 1], cache, t)
            b = m(idx[:, :t + 1])[0][:, -1].float()
            assert a.abs().max() <= 30.0 and a.abs().max() > 20.0
            assert _rel(a, b) < 2e-2, (t, _rel(a, b))
    out = m.generate(idx[:, :5], 10, temperature=0.0, use_cache=True)
    assert out.shape == (2, 15)


def test_device_position_decode_and_graph_replay():
    """forward_decode (device position) against the host-position KV-cache step, then a DecodeGraph with per-row
    positions replayed at three positions against the eager step, as
    tests/test_qk_norm_gpu.py::test_device_position_decode_and_graph_replay: the cap is part of the captured step."""
    from pretraining_llm_amd.inference.generate import DecodeGraph, KVCache, forward_cached, forward_decode
    torch.manual_seed(6)
    cfg, m = _tiny_capped_model()
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
    assert b.abs().max() <= 30.0 and b.abs().max() > 20.0
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
        assert g.abs().max() <= 30.0
