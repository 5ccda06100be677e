"""CPU checks of ``_streaming_refs``: every fp64 reference against an independent PyTorch double-precision
path to 1e-12 relative, and the calibration of the per-op budgets against a plain fp32 evaluation of the same
cases that ``test_streaming_edges_gpu.py`` runs on the HIP kernels."""
import math

import pytest
import torch
import torch.nn.functional as F

import _streaming_refs as R

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32


def _same(a, b, what, tol=1e-12):
    """max|a - b| <= tol max|b|: relative to the tensor's largest element, not per element.  Both sides are fp64
    evaluations of the same formula in a different order, so their difference is rounding noise of the large
    intermediate terms, about 1e-16 of the tensor's scale, whatever an element's own size."""
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert float((a - b).abs().max()) <= tol * scale, f"{what}: {float((a - b).abs().max())} vs scale {scale}"


# ------------------------------------------------------------------------------------ references vs PyTorch fp64
@pytest.mark.parametrize("rms", [0, 1])
@pytest.mark.parametrize("res", [0, 1])
@pytest.mark.parametrize("C,N", [(8, 3), (200, 6), (1032, 6)])
def test_norm_refs_match_torch_double(rms, res, C, N):
    inp = R.norm_inputs(rms, res, C, N)
    eps = R.f32r(inp["eps"])
    fw, mean32, rstd32 = R.norm_stats32(inp)
    sq = fw["s_bf16"].to(F64).requires_grad_()
    w = inp["w"].to(F64).requires_grad_()
    if inp["r"] is not None:
        assert torch.equal(fw["s_bf16"], (inp["x"].float() + inp["r"].float()).to(BF16))
    if rms:
        y = sq * torch.rsqrt(sq.pow(2).mean(-1, keepdim=True) + eps) * w
        params = [sq, w]
    else:
        b = inp["b"].to(F64).requires_grad_()
        y = F.layer_norm(sq, (C,), w, b, eps)
        params = [sq, w, b]
        _same(fw["mean"][0], sq.detach().mean(-1), "mean")
    _same(fw["rstd"][0], ((sq.detach() if rms else sq.detach() - sq.detach().mean(-1, keepdim=True)).pow(2).mean(-1)
                          + eps).rsqrt(), "rstd")
    _same(fw["y"][0], y.detach(), "y")
    # backward from the exact statistics (the kernel's fp32 ones differ at 1e-8)
    bw = R.norm_bwd_ref(inp["dy"], fw["s_bf16"], inp["w"], fw["mean"][0], fw["rstd"][0], inp["ds"], rms)
    grads = torch.autograd.grad(y, params, inp["dy"].to(F64))
    dx = grads[0] + (inp["ds"].to(F64) if inp["ds"] is not None else 0.0)
    _same(bw["dx"][0], dx, "dx")
    _same(bw["dw"][0], grads[1], "dw")
    if not rms:
        _same(bw["db"][0], grads[2], "db")
    _same(R.colsum_ref(bw["dx"][0])[0], dx.sum(0), "column sums of dx")


def test_activation_refs_match_torch_double():
    for data in ("randn", "grid"):
        inp = R.act_inputs("gelu", 8 * 257, data)
        x = inp["x"].to(F64).requires_grad_()
        y = F.gelu(x, approximate="tanh")
        (dx,) = torch.autograd.grad(y, x, inp["dy"].to(F64))
        _same(R.gelu_ref(inp["x"])[0], y.detach(), "gelu")
        _same(R.gelu_bwd_ref(inp["dy"], inp["x"])[0], dx, "gelu bwd")
        inp = R.act_inputs("relu", 8 * 257, data)
        x = inp["x"].to(F64).requires_grad_()
        y = F.relu(x)
        (dx,) = torch.autograd.grad(y, x, inp["dy"].to(F64))
        _same(R.relu_ref(inp["x"])[0], y.detach(), "relu")
        _same(R.relu_bwd_ref(inp["dy"], R.relu_of(inp["x"]))[0], dx, "relu bwd")
        inp = R.swiglu_inputs(5, 136, data)
        gu = inp["gu"].to(F64).requires_grad_()
        y = F.silu(gu[..., :136]) * gu[..., 136:]
        (dgu,) = torch.autograd.grad(y, gu, inp["dy"].to(F64))
        _same(R.swiglu_ref(inp["gu"])[0], y.detach(), "swiglu")
        _same(R.swiglu_bwd_ref(inp["dy"], inp["gu"])[0], dgu, "swiglu bwd")


@pytest.mark.parametrize("V", [8, 4104])
@pytest.mark.parametrize("all_ignored", [False, True])
def test_cross_entropy_ref_matches_torch_double(V, all_ignored):
    inp = R.ce_inputs(V, all_ignored)
    ref = R.ce_ref(inp["logits"], inp["targets"])
    x = inp["logits"].to(F64).requires_grad_()
    loss = F.cross_entropy(x, inp["targets"], ignore_index=R.IGNORE, reduction="none")
    _same(ref["loss"][0], loss.detach(), "loss")
    if all_ignored:
        assert float(ref["dlogits"][0].abs().max()) == 0.0
        return
    (dl,) = torch.autograd.grad(F.cross_entropy(x, inp["targets"], ignore_index=R.IGNORE), x)
    _same(ref["dlogits"][0], dl, "dlogits")
    _same(R.ce_ref(inp["logits"], inp["targets"], inv_n=0.125)["dlogits"][0],
          dl * 0.125 * int((inp["targets"] != R.IGNORE).sum()), "dlogits with inv_n")


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adamw_ref_matches_torch_double(step):
    inp = R.adamw_inputs(R.ADAMW_N[3], "f32", "pattern", "base")
    inp.update(step=step)
    hp = {k: R.f32r(inp[k]) for k in ("lr", "b1", "b2", "eps", "wd")}
    ref = R.adamw_ref(**inp)
    outs = {}
    for wd in (hp["wd"], 0.0):
        p = torch.nn.Parameter(inp["master"].to(F64))
        opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd)
        opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=inp["m"].to(F64).clone(),
                            exp_avg_sq=inp["v"].to(F64).clone())
        p.grad = inp["grad"].to(F64) * (R.f32r(inp["grad_scale"]) * R.f32r(inp["scale"]))
        opt.step()
        outs[wd] = (p.detach().clone(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
    on = inp["wd_mask"][torch.arange(inp["master"].numel()) // 64] != 0
    assert on.any() and not on.all()
    _same(ref["master"], torch.where(on, outs[hp["wd"]][0], outs[0.0][0]), "parameters")
    _same(ref["m"][0], outs[0.0][1], "m")
    _same(ref["v"][0], outs[0.0][2], "v")
    # the device-side scalars replace lr and both bias corrections
    bc1, bc2 = 1 - hp["b1"] ** step, 1 - hp["b2"] ** step
    hy = R.adamw_ref(**{**inp, "lr": 123.0, "step": 77,
                        "hyper": torch.tensor([hp["lr"], 1 / bc1, 1 / math.sqrt(bc2)], dtype=F64)})
    _same(hy["master"], ref["master"], "hyper")  # (the hyper tensor is fp64 here, so nothing is rounded to fp32)


def test_sumsq_refs_match_torch_double():
    x = R.sumsq_inputs(8 * 255, BF16)
    _same(R.sumsq_ref(x)[0], torch.linalg.vector_norm(x.to(F64)) ** 2, "sumsq")
    for max_norm in (1.0, 1e6):
        g = R.grad_norm_clip_ref(x, 0.5, max_norm)[0]
        n = torch.linalg.vector_norm(x.to(F64)) * 0.5
        _same(g, torch.stack([n, torch.clamp(R.f32r(max_norm) / (n + R.f32r(1e-6)), max=1.0)]), "grad_norm_clip")


def test_assert_close_ulps_reports_and_bounds():
    ref = torch.tensor([1.0, -2.0, 0.0, 1e-3], dtype=F64)
    R.assert_close_ulps(ref.to(BF16), ref, 1)
    out = ref.clone()
    out[1] = -2.0 - 2.0 * 2.0 ** -8 * 1.5  # 1.5 bf16 ulps of 2
    R.assert_close_ulps(out.to(F32), ref, 2, fmt=BF16)
    with pytest.raises(AssertionError, match=r"1 of 4 elements.*worst at \(1,\)"):
        R.assert_close_ulps(out.to(F32), ref, 1, fmt=BF16)
    R.assert_close_ulps(out.to(F32), ref, 1, abs_floor=torch.tensor([0, 2.0 ** -8, 0, 0]), fmt=BF16)
    with pytest.raises(AssertionError):  # a NaN is never within bound
        R.assert_close_ulps(torch.tensor([math.nan]), torch.tensor([0.0], dtype=F64), 10 ** 6, abs_floor=1e30)
    assert R.ulps_needed(out.to(F32), ref, fmt=BF16) == 2


# ------------------------------------------------------------------------------------ calibration of the budgets
def _model_items():
    """Every comparison of the GPU file, with the plain fp32 CPU evaluation in the kernel's place."""
    for case in R.norm_cases():
        inp = R.norm_inputs(*case)
        yield from R.norm_checks(inp, R.norm_model_outputs(inp))
    for kind in ("relu", "gelu"):
        for numel in R.ACT_NUMEL:
            for data in ("randn", "grid"):
                inp = R.act_inputs(kind, numel, data)
                yield from R.act_checks(kind, inp, (R.relu_model_f32 if kind == "relu" else R.gelu_model_f32)(**inp))
        for N, C in R.ACT_BIAS_SHAPES:
            for acc in (BF16, F32):
                inp = R.act_bias_inputs(kind, N, C)
                yield from R.act_bias_checks(kind, inp, R.act_bias_model_f32(kind, inp, acc), acc)
        for N, C in R.ACT_BIAS_GRID_SHAPES:
            inp = R.act_bias_inputs(kind, N, C, "grid")
            yield from R.act_bias_checks(kind, inp, R.act_bias_model_f32(kind, inp, F32), F32)
    for rows, Fd in R.SWIGLU_SHAPES:
        for data in ("randn", "grid"):
            inp = R.swiglu_inputs(rows, Fd, data)
            yield from R.swiglu_checks(inp, R.swiglu_model_f32(**inp))
    for V in R.CE_V:
        inp = R.ce_inputs(V)
        yield from R.ce_checks(inp, R.ce_model_f32(**inp))
        yield from R.ce_checks(inp, R.ce_model_f32(**inp, inv_n=0.125), inv_n=0.125)
    inp = R.ce_inputs(4104, all_ignored=True)
    yield from R.ce_checks(inp, R.ce_model_f32(**inp))
    for case in R.adamw_cases():
        inp = R.adamw_inputs(*case)
        yield from R.adamw_checks(inp, R.adamw_model_outputs(inp))
    for n in R.SUMSQ_N:
        for dt in (BF16, F32):
            x = R.sumsq_inputs(n, dt)
            yield ("sumsq", "sumsq", (x.float() ** 2).sum(), R.sumsq_ref(x))
            for max_norm in (1.0, 1e9):
                nrm = (x.float() ** 2).sum().sqrt() * 0.5
                out = torch.stack([nrm, torch.clamp(torch.tensor(max_norm) / (nrm + 1e-6), max=1.0)])
                yield ("sumsq", "grad_norm_clip", out, R.grad_norm_clip_ref(x, 0.5, max_norm))


def test_budgets_are_calibrated_on_the_fp32_model():
    measured, worst = {}, {}
    for it in _model_items():
        op, name, out, (ref, unit) = it[:4]
        fmt = it[4] if len(it) > 4 else None
        u = R.ulps_needed(out, ref, unit, fmt)
        if u >= measured.get(op, -1):
            measured[op], worst[op] = u, it
    print("measured smallest budgets:", measured)
    assert measured == {op: b[0] for op, b in R.BUDGET.items()}, "the table in _streaming_refs.py is stale"
    for op, (m, b) in R.BUDGET.items():
        assert b == 2 * m
        if m == 0:
            continue  # exact ops: nothing to loosen
        _, name, out, (ref, unit) = worst[op][:4]
        R.check(*worst[op][:1], out, (ref, unit), name, *worst[op][4:5])  # the worst case passes at the budget
        with pytest.raises(AssertionError):  # and fails at a zero budget
            R.assert_close_ulps(out, ref, 0, 0.0, what=f"{op}/{name}", fmt=worst[op][4] if len(worst[op]) > 4 else None)
