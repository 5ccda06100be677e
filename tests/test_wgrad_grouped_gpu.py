"""The grouped whole-tile arm of the ping-pong weight-gradient kernel (csrc/wgrad_pp.hip, ``wgrad_group``) driven
by the deferral queue of ``ops``: small problem sets that mix every tile edge, on grids forced down to 8
workgroups so that one launch covers several rounds, a problem's row bands split across two launches and a
remainder is left for the end-of-backward flush; then a 2-block GPT with deferral on and off.

Tolerances.  A gradient element is a sum of M exact bf16 x bf16 products accumulated in fp32 and added once to
the target: |err| <= (M + 1) u S with u = 2^-24 and S = sum |dy||x| + |target|; the MFMA's internal order of the
adds is not specified, so twice that is allowed: (M + 2) 2^-23 S per element (bias: S = sum |dy| + |target|).
The whole-gradient bound is the one tests/test_gemm_gpu.py uses for ``wgrad``: relative Frobenius error < 1e-5."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 1024  # fp32 elements of sentinel before and after every target
SENT = -777.25
# (P, Q, bias): exact; ragged in both, 2 x 1 tiles; minimum P, 3 ragged Q tiles; 3 row bands with a bias
PROBLEMS = {"exact": (256, 256, False), "ragged": (264, 72, False), "thin": (8, 520, False), "bias": (768, 256, True)}
ORDERS = {"first": ["bias", "exact", "ragged", "thin"], "middle": ["exact", "ragged", "bias", "thin"],
          "last": ["exact", "ragged", "thin", "bias"]}


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _guarded(n, fill):
    buf = torch.full((n + 2 * GUARD,), SENT, device=DEV)
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n]


def _guards_ok(buf, n):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())


_CASES = {}


def _case(name, M, overwrite):
    """Inputs, the initial targets, the single-problem launch's result (default grid: unsliced) and the fp64
    reference with its per-element bounds -- computed once per (problem, M, overwrite) and never changed."""
    key = (name, M, overwrite)
    if key not in _CASES:
        P, Q, bias = PROBLEMS[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)) + M + int(overwrite))
        dy = (0.5 * torch.randn(M, P, generator=g)).bfloat16().to(DEV)
        x = torch.randn(M, Q, generator=g).bfloat16().to(DEV)
        w0 = torch.randn(P * Q, generator=g).to(DEV)
        b0 = torch.randn(P, generator=g).to(DEV)
        plan = list(torch.ops.pllm.wgrad_plan(M, P, Q, True, bias))
        assert plan[0] == 2 and plan[1] == 1, plan  # the ping-pong kernel, one slice: whole tiles
        single_w, single_b = w0.clone(), b0.clone()
        torch.ops.pllm.wgrad(dy, x, single_w.view(P, Q), single_b if bias else None, overwrite)
        init = torch.zeros_like(w0) if overwrite else w0
        ref = (dy.double().t() @ x.double()).view(-1) + init.double()
        tol = (M + 2) * 2.0 ** -23 * ((dy.double().abs().t() @ x.double().abs()).view(-1) + init.double().abs())
        bref = dy.double().sum(0) + b0.double()
        btol = (M + 2) * 2.0 ** -23 * (dy.double().abs().sum(0) + b0.double().abs())
        _CASES[key] = dict(dy=dy, x=x, w0=w0, b0=b0, single_w=single_w, single_b=single_b, ref=ref, tol=tol,
                           bref=bref, btol=btol, P=P, Q=Q, bias=bias)
    return _CASES[key]


class _Told:
    def __init__(self, log, tag):
        self._pllm_grad_ready = lambda: log.append(tag)


@pytest.mark.parametrize("overwrite", [True, False])
@pytest.mark.parametrize("order", ["first", "middle", "last"])
@pytest.mark.parametrize("persistent", [True, False])
@pytest.mark.parametrize("mode", ["stream", "bulk"])
def test_grouped_tiles(mode, persistent, order, overwrite):
    """``stream``: rounds of 8 tiles launched as the queue fills (row bands of one problem in two launches, a
    remainder for the flush); ``bulk``: everything queued first, so one launch of 16 tiles runs two rounds on 8
    workgroups (or 16 workgroups of one tile), each workgroup switching problem, row strides and token count
    between its items."""
    from pretraining_llm_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    names = [(n, M) for M in (128, 192) for n in ORDERS[order]]  # 2 x 9 = 18 tiles
    cases = [_case(n, M, overwrite) for n, M in names]
    q, told, launches = ops._WgradQueue(), [], []
    run_group, run_single = q.run_group, q.run_single
    q.run_group = lambda items, first, last: (launches.append(("group", len(items), first, last)),
                                              run_group(items, first, last))
    q.run_single = lambda *a: (launches.append(("single", tuple(a[2].shape))), run_single(*a))
    bufs, cuts = [], []
    try:
        ops.gemm_config(reserve_cus=0 if mode == "bulk" else cus - 8, persistent=persistent)
        for i, c in enumerate(cases):
            wbuf, w = _guarded(c["P"] * c["Q"], c["w0"])
            bbuf, b = _guarded(c["P"], c["b0"])
            bufs.append((wbuf, w, bbuf, b))
            q.armed = True  # (as inside a backward: the flush below stands for the engine's callback)
            q.push(c["dy"], c["x"], w.view(c["P"], c["Q"]), b if c["bias"] else None, overwrite,
                   (_Told(told, ("w", i)), _Told(told, ("b", i)) if c["bias"] else None))
            cuts.append(q.done0)
        if mode == "bulk":
            assert not launches and not told
            ops.gemm_config(reserve_cus=cus - 8)
        q.flush()
    finally:
        ops.gemm_config(reserve_cus=0, persistent=True)
    torch.cuda.synchronize()
    groups = [e for e in launches if e[0] == "group"]
    assert launches[-1][0] == "single", launches  # a remainder went to the single-problem plan
    if mode == "bulk":
        assert groups[0][3] - groups[0][2] > 8 and groups[0][1] > 4, launches  # more than one round of 8 workgroups
    else:
        assert len(groups) >= 2 and any(cuts), (launches, cuts)  # a problem's row bands in two launches
    # told once each, weight before its bias, in queue order
    assert told == [t for i, c in enumerate(cases) for t in ([("w", i)] + ([("b", i)] if c["bias"] else []))]
    for c, (wbuf, w, bbuf, b), (name, M) in zip(cases, bufs, names):
        tag = (name, M, launches)
        assert _guards_ok(wbuf, w.numel()) and _guards_ok(bbuf, b.numel()), tag
        err = (w.double() - c["ref"]).abs()
        assert bool((err <= c["tol"]).all()), (tag, float((err / c["tol"]).max()))
        assert float((w.double() - c["ref"]).norm() / c["ref"].norm()) < 1e-5, tag
        assert torch.equal(w, c["single_w"]), tag  # same main loop, same order: the single-problem launch's bits
        if c["bias"]:
            assert bool(((b.double() - c["bref"]).abs() <= c["btol"]).all()), tag
            assert torch.equal(b, c["single_b"]), tag
        else:
            assert torch.equal(b, c["b0"]), tag


def test_wgrad_group_rejects_bad_ranges():
    c = _case("exact", 128, True)
    w = torch.zeros(256, 256, device=DEV)
    e = torch.empty(0, device=DEV)
    with pytest.raises(RuntimeError):
        torch.ops.pllm.wgrad_group([c["dy"]], [c["x"]], [w], [e], [1], 0, 2)  # one tile only
    with pytest.raises(RuntimeError):
        torch.ops.pllm.wgrad_group([c["dy"][:64]], [c["x"][:64]], [w], [e], [1], 0, 1)  # a single K-tile
    with pytest.raises(RuntimeError):
        torch.ops.pllm.wgrad_group([c["dy"]] * 17, [c["x"]] * 17, [w] * 17, [e] * 17, [1] * 17, 0, 17)
    torch.ops.pllm.wgrad_group([c["dy"]], [c["x"]], [w], [e], [1], 0, 0)  # an empty range launches nothing
    assert float(w.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ autograd level
B, T = 2, 64


def _model():
    from pretraining_llm_amd.models import GPT, get_preset
    from pretraining_llm_amd.train.optim import FlatAdamW
    cfg = get_preset("gpt2-tiny").replace(vocab_size=512, context_length=T, n_embed=64, n_head=2, n_blocks=2)
    torch.manual_seed(0)
    model = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
    opt = FlatAdamW(model, lr=1e-3, lazy_zero=True)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (B, T), generator=g).to(DEV)
    y = torch.randint(0, cfg.vocab_size, (B, T), generator=g).to(DEV)
    return cfg, model, opt, x, y


_REF = {}


def _fp64_grads():
    """The same weights' gradients in fp64 on stock torch ops on the CPU (the pattern of tests/test_gemm_gpu.py)."""
    if not _REF:
        from pretraining_llm_amd import ops
        from pretraining_llm_amd.models import GPT
        cfg, _, _, x, y = _model()
        torch.manual_seed(0)
        ref = GPT(cfg).to(dtype=torch.bfloat16).double()  # the bf16-rounded initial weights, as _model's
        with ops.backend("torch"), torch.enable_grad():
            ref(x.cpu(), y.cpu(), return_logits=False)[1].backward()
        _REF.update({n: p.grad.reshape(-1) for n, p in ref.named_parameters() if p.grad is not None})
    return _REF


def _backward(defer, monkeypatch, steps=1, graph=False):
    """-> (flat gradient, {name: times told}, {name: slot complete when told}, names left fresh, launches)."""
    from pretraining_llm_amd import ops
    monkeypatch.setattr(ops, "WGRAD_DEFER", defer)
    monkeypatch.setattr(ops, "WGRAD_DEFER_MIN_SLICES", 1)  # queue the unsliced 128-token problems too
    cfg, model, opt, x, y = _model()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    launches = []
    q = ops._WgradQueue()
    run_group, run_single = q.run_group, q.run_single
    q.run_group = lambda items, first, last: (launches.append(("group", first, last)), run_group(items, first, last))
    q.run_single = lambda *a: (launches.append(("single",)), run_single(*a))
    monkeypatch.setattr(ops, "_WGRAD_QUEUE", q)
    told, snap = {}, {}
    for n, p in zip(opt.names, opt.params):
        def cb(n=n, p=p):
            told[n] = told.get(n, 0) + 1
            snap[n] = p._pllm_gradbuf.clone()
        p._pllm_grad_ready = cb
    try:
        ops.gemm_config(reserve_cus=cus - 8)  # rounds of 8 tiles: the two blocks' 8 one-tile problems
        opt.zero_grad()
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model(x, y, return_logits=False)[1].backward()  # warm-up (allocations, hipBLASLt choices)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            opt.zero_grad()
            told.clear()
            del launches[:]
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                model(x, y, return_logits=False)[1].backward()
            opt.flat_grad.fill_(float("nan"))  # the replay alone fills the fresh slots; the others add
            opt.zero_grad()
            for p in opt._fresh_params:
                p._pllm_grad_fresh = False
            gr.replay()
        else:
            for _ in range(steps):
                told.clear()
                model(x, y, return_logits=False)[1].backward()
    finally:
        ops.gemm_config(reserve_cus=0)
    torch.cuda.synchronize()
    fresh = [n for n, p in zip(opt.names, opt.params) if getattr(p, "_pllm_grad_fresh", False)]
    final = {n: p._pllm_gradbuf for n, p in zip(opt.names, opt.params)}
    complete = {n: torch.equal(snap[n], final[n]) for n in snap}
    return opt, told, complete, fresh, launches


def _check_against_fp64(opt, scale=1.0):
    """Every parameter's slot against the fp64 gradient.  The model computes in bf16, so the bound is the one
    the suite holds a bf16 model's parameter gradients to against full-precision math on the same weights
    (tests/test_gemm_gpu.py: relative Frobenius error < 5e-2); what deferral itself may change is pinned bit for
    bit in test_gpt_second_backward_accumulates."""
    ref = _fp64_grads()
    for n, p in zip(opt.names, opt.params):
        r = scale * ref[n]
        e = float((p._pllm_gradbuf.double().cpu().reshape(-1) - r).norm() / (r.norm() + 1e-30))
        print(f"{n}: rel {e:.3e}")
        assert e < 5e-2, (n, e)


@pytest.mark.parametrize("defer", [True, False])
def test_gpt_backward_deferred_and_immediate(defer, monkeypatch):
    opt, told, complete, fresh, launches = _backward(defer, monkeypatch)
    assert set(told) == set(opt.names)
    tied = {n for n, c in told.items() if c != 1}
    assert tied <= {"token_embed.weight"} and all(told[n] == 2 for n in tied), told  # (LM head + embedding scatter)
    assert fresh == []
    assert all(complete[n] for n in opt.names if n not in tied), complete
    if defer:
        assert [e for e in launches if e[0] == "group"] == [("group", 0, 8)], launches
    else:
        assert launches == []
    _check_against_fp64(opt)


def test_gpt_second_backward_accumulates(monkeypatch):
    opt, told, complete, fresh, launches = _backward(True, monkeypatch, steps=2)
    assert len([e for e in launches if e[0] == "group"]) == 2 and fresh == []
    _check_against_fp64(opt, scale=2.0)
    one = _backward(True, monkeypatch)[0].flat_grad.clone()
    off = _backward(False, monkeypatch, steps=2)[0].flat_grad
    two = _backward(True, monkeypatch, steps=2)[0].flat_grad
    assert torch.equal(two, off)  # whole tiles either way at 128 tokens: deferral changes no bit
    torch.testing.assert_close(two, 2 * one, rtol=2.0 ** -20, atol=1e-9)


def test_gpt_backward_under_graph_capture(monkeypatch):
    eager = _backward(True, monkeypatch)[0].flat_grad.clone()
    opt, told, complete, fresh, launches = _backward(True, monkeypatch, graph=True)
    assert ("group", 0, 8) in launches  # captured, not run eagerly around the graph
    assert torch.equal(opt.flat_grad, eager)


def test_default_thresholds_at_sliced_shapes(monkeypatch):
    """Two GPT-2-small blocks at 4096 tokens with the default settings: every block weight gradient is one the
    immediate plan slices (S > 1), so all are queued; on a 64-workgroup grid three whole rounds run grouped and
    the rest goes to the sliced single-problem plan.  Deferred and immediate differ only in the fp32 summation
    order of the weight gradients: each is within 1e-5 (relative Frobenius, the bound of tests/test_gemm_gpu.py
    for ``wgrad``) of the exact product of the same bf16 operands, so they are within 2e-5 of each other; every
    other gradient (but the QKV biases', summed inside those GEMMs) comes from the same deterministic kernels on the
    same inputs and keeps its bits."""
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT, get_preset
    from pretraining_llm_amd.train.optim import FlatAdamW
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cfg = get_preset("gpt2-small").replace(vocab_size=512, context_length=1024, n_blocks=2)
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, cfg.vocab_size, (4, 1024), generator=g).to(DEV)
    y = torch.randint(0, cfg.vocab_size, (4, 1024), generator=g).to(DEV)
    assert torch.ops.pllm.wgrad_plan(4096, 768, 768, True, False)[1] > 1
    res, absum = {}, []  # absum: column sums of |dy| of the problems with a fused bias, in the backward's order
    for defer in (True, False):
        monkeypatch.setattr(ops, "WGRAD_DEFER", defer)
        torch.manual_seed(0)
        model = GPT(cfg).to(device=DEV, dtype=torch.bfloat16)
        opt = FlatAdamW(model, lr=1e-3, lazy_zero=True)
        q, launches = ops._WgradQueue(), []
        run_group, run_single = q.run_group, q.run_single
        q.run_group = lambda items, first, last: (launches.append(last - first), run_group(items, first, last))
        q.run_single = lambda *a: (launches.append("single"), run_single(*a))
        push = q.push
        q.push = lambda dy2, x2, out, btgt, *a: (None if btgt is None else absum.append(dy2.float().abs().sum(0)),
                                                 push(dy2, x2, out, btgt, *a))[1]
        monkeypatch.setattr(ops, "_WGRAD_QUEUE", q)
        try:
            ops.gemm_config(reserve_cus=cus - 64)
            opt.zero_grad()
            model(x, y, return_logits=False)[1].backward()
        finally:
            ops.gemm_config(reserve_cus=0)
        torch.cuda.synchronize()
        assert not q.items and not [n for n, p in zip(opt.names, opt.params) if getattr(p, "_pllm_grad_fresh", False)]
        res[defer] = ({n: p._pllm_gradbuf.clone() for n, p in zip(opt.names, opt.params)}, launches)
    (gd, ld), (gi, li) = res[True], res[False]
    assert li == [] and sum(t for t in ld if t != "single") >= 128 and "single" in ld, ld  # 216 tiles, rounds of 64
    # the QKV bias gradients ride in their weight-gradient GEMMs (column sums of dy by MFMAs): the per-element
    # bound of the module docstring against the exact sum for each of the two, so twice it between them
    fused_bias = {"attn_blocks.1.attn.qkv.bias": 0, "attn_blocks.0.attn.qkv.bias": 1}
    assert len(absum) == 2
    for n in gd:
        if n.endswith("weight") and gd[n].numel() >= 768 * 768 and "embed" not in n:
            e = float((gd[n].double() - gi[n].double()).norm() / gi[n].double().norm())
            print(f"{n}: deferred vs immediate rel {e:.3e}")
            assert e < 2e-5, (n, e)
        elif n in fused_bias:
            tol = 2 * (4096 + 2) * 2.0 ** -23 * absum[fused_bias[n]].double()
            d = (gd[n].double() - gi[n].double()).abs()
            print(f"{n}: deferred vs immediate max err / bound {float((d / tol).max()):.3e}")
            assert bool((d <= tol).all()), n
        else:
            assert torch.equal(gd[n], gi[n]), n
