"""CPU checks of ``_gemm_refs``: every fp64 reference against an independent double-precision PyTorch path, the
calibration of the budget table on the fp32 models of the cases that ``test_gemm_edges_gpu.py`` runs on the HIP
kernels, and the defects that the per-element bound rejects (several of which the older whole-matrix criterion,
``||out - ref|| / ||ref|| < 5e-3``, accepts)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _gemm_refs as G
import _streaming_refs as S

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32
OLD_TOL = 5e-3  # the whole-matrix criterion of tests/test_gemm_gpu.py and the wgrad / gemv tests


def _same(a, b, what, tol=1e-12):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert float((a - b).abs().max()) <= tol * scale, f"{what}: {float((a - b).abs().max())} vs scale {scale}"


def _rejected(items):
    with pytest.raises(AssertionError, match="out of bound"):
        G.check_all(items)


# ------------------------------------------------------------------------------------ references vs PyTorch fp64
def test_gemm_refs_match_torch_double():
    M, N, K = 129, 264, 192
    inp, refs = G.gemm_inputs(M, N, K), G.gemm_refs(M, N, K)
    a, b, bias = (inp[k].to(F64) for k in ("a", "b", "bias"))
    _same(refs["c"][0], F.linear(a, b), "c")
    _same(refs["cb"][0], F.linear(a, b, bias), "c + bias")
    _same(refs["c7"][0], torch.einsum("mk,nk->mn", a, inp["b7"].to(F64)), "[gate | up]")
    _same(refs["cb"][1], S.E32 * (torch.einsum("mk,nk->mn", a.abs(), b.abs()) + bias.abs()), "unit")
    # the fused backward epilogues: act'(aux) d by autograd, d a bf16 data gradient
    out = G.gemm_model_outputs(M, N, K)
    items = {it[1]: it for it in G.gemm_checks(inp, refs, out)}
    d = out["c0"].to(F64)
    x = inp["aux"].to(F64).requires_grad_()
    (g3,) = torch.autograd.grad(F.gelu(x, approximate="tanh"), x, d)
    _same(items["o3"][3][0], g3, "gelu'(aux) d")
    x = inp["aux"].to(F64).requires_grad_()
    (g4,) = torch.autograd.grad(F.relu(x), x, d)
    _same(items["o4"][3][0], g4, "relu'(aux) d")
    gu = inp["gu"].to(F64).requires_grad_()
    (g5,) = torch.autograd.grad(F.silu(gu[:, :N]) * gu[:, N:], gu, d)
    _same(items["o5"][3][0], g5, "swiglu'(gu) d")
    _same(items["act1"][3][0], F.gelu(out["pre1"].to(F64), approximate="tanh"), "gelu(pre)")
    g7 = out["gu7"].to(F64)
    _same(items["a7"][3][0], F.silu(g7[:, :N]) * g7[:, N:], "silu(g) u")
    _same(items["b3_f32"][3][0], inp["fill"].to(F64) + out["o3"].to(F64).sum(0), "column sums")
    _same(items["b3_bf16"][3][0], inp["fill"].to(BF16).to(F64) + torch.einsum("mn->n", out["o3"].to(F64)), "column sums")


def test_exact_family_is_exact_and_carries_ties():
    for M, N, K in ((17, 72, 128), (300, 264, 64), (520, 776, 2112)):
        inp, refs = G.gemm_inputs(M, N, K, "exact"), G.gemm_refs(M, N, K, "exact")
        for k in ("a", "b", "b7", "bias"):  # integers that bf16 holds
            assert torch.equal(inp[k].float(), inp[k].float().round())
        ai, bi = inp["a"].long(), inp["b"].long()
        exact = ai @ bi.t()
        # every partial sum in any order is bounded by sum |a||b| < 2^24: exact in fp32
        assert int((ai.abs() @ bi.abs().t()).max()) + 4 < 2 ** 24
        assert torch.equal(refs["c"][0], exact.to(F64).to(F32).to(BF16).to(F64)) and refs["c"][1] == 0.0
        assert torch.equal(refs["cb"][0], (exact + inp["bias"].long()).to(F64).to(F32).to(BF16).to(F64))
        for r in (0, M - 1):
            assert exact[r, :4].tolist() == [257, 259, -257, -259] == exact[r, N - 4:].tolist()
            assert refs["c"][0][r, :4].tolist() == [256.0, 260.0, -256.0, -260.0]  # ties to even
        # most outputs need rounding: a truncating store differs on many of them
        assert float((exact.to(F64) != refs["c"][0]).double().mean()) > 0.25
        # the fp32 model reproduces the reference bitwise in either summation order
        for chunked in (False, True):
            out = G.gemm_model_outputs(M, N, K, "exact", chunked=chunked)
            for key, r in (("c0", "c"), ("c0b", "cb"), ("pre1", "cb"), ("gu7", "c7")):
                assert torch.equal(out[key].to(F64), refs[r][0]), (key, chunked)


def test_delta_ref_matches_torch_double():
    B, T, N, K = 3, 112, 320, 128
    inp = G.delta_inputs(B, T, N, K)
    out = G.delta_model_outputs(B, T, N, K)
    ref, unit = G.delta_ref(out["do6"], inp["o"], B, T)
    e = torch.einsum("bthd,bthd->bht", out["do6"].to(F64).view(B, T, N // 64, 64), inp["o"].to(F64).view(B, T, N // 64, 64))
    _same(ref, e, "delta")
    assert ref.shape == (B, N // 64, T) == unit.shape


def test_wgrad_refs_match_autograd_double():
    name = "tiles2x3"
    inp, r = G.wgrad_inputs(name), G.wgrad_refs(name)
    W = torch.zeros(inp["dy"].shape[1], inp["x"].shape[1], dtype=F64, requires_grad=True)
    b = torch.zeros(inp["dy"].shape[1], dtype=F64, requires_grad=True)
    gw, gb = torch.autograd.grad(F.linear(inp["x"].to(F64), W, b), (W, b), inp["dy"].to(F64))
    _same(r["w"], gw, "dW")
    _same(r["db"], gb, "db")
    _same(r["wa"], torch.einsum("mp,mq->pq", inp["dy"].to(F64).abs(), inp["x"].to(F64).abs()), "unit")
    items = {it[1]: it for it in G.wgrad_checks(name, G.wgrad_model_outputs(name))}
    _same(items["acc_bf16"][3][0], inp["acc0"].to(BF16).to(F64) + gw, "accumulated into bf16")
    _same(items["bias_f32"][3][0], inp["b0"].to(F64) + gb, "bias gradient")


@pytest.mark.parametrize("rms", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
def test_gemv_norm_ref_matches_torch_double(rms, with_res):
    M, N, K = 3, 1032, 768
    inp = G.gemv_inputs(M, N, K, 2 if rms else 1)
    ref = G.gemv_norm_ref(inp, rms, with_res)
    s = (inp["x"].float() + inp["res"].float()).to(BF16) if with_res else inp["x"]
    assert torch.equal(ref["s"][0], s.to(F64))
    sq = s.to(F64)
    if rms:
        n = sq * torch.rsqrt(sq.pow(2).mean(-1, keepdim=True) + S.f32r(G.GEMV_EPS)) * inp["gamma"].to(F64)
    else:
        n = F.layer_norm(sq, (K,), inp["gamma"].to(F64), inp["beta"].to(F64), S.f32r(G.GEMV_EPS))
    _same(ref["n"], n, "normalised input")
    _same(ref["y"][0], F.linear(n, inp["w"].to(F64), inp["bias"].to(F64)), "y")
    _same(G.gemv_ref(inp)[0], F.linear(inp["x"].to(F64), inp["w"].to(F64), inp["bias"].to(F64)), "plain y")


# ------------------------------------------------------------------------------------ calibration of the budgets
def _model_items():
    """Every comparison of the new rows in the GPU file, with the fp32 CPU models in the kernel's place."""
    for M, N, K in G.GEMM_SHAPES + (G.SWIGLU_F136,):
        for aux in ("randn", "grid") if (M, N, K) == G.GEMM_GRID_AUX else ("randn",):
            inp, refs = G.gemm_inputs(M, N, K, "randn", aux), G.gemm_refs(M, N, K, "randn", aux)
            for chunked in (False, True):
                yield from G.gemm_checks(inp, refs, G.gemm_model_outputs(M, N, K, aux=aux, chunked=chunked))
    for B, T, N, K in G.DELTA_CASES:
        for chunked in (False, True):
            yield from G.delta_checks(G.delta_inputs(B, T, N, K), B, T, G.delta_model_outputs(B, T, N, K, chunked))
    for name in G.WGRAD_CASES:
        for order in ("torch", "plan") + (("whole", "hybrid") if name in G.WGRAD_HYBRID else ()):
            yield from G.wgrad_checks(name, G.wgrad_model_outputs(name, order))
    for M, N, K, bias in G.gemv_cases():
        inp = G.gemv_inputs(M, N, K)
        for chain in (False, True):
            yield ("gemv_y", "y", G.gemv_model_outputs(inp, N, K, bias=bias, chain=chain)["y"], G.gemv_ref(inp, bias))
    for M, N, K, norm, wr in G.gemv_norm_cases():
        inp = G.gemv_inputs(M, N, K, norm)
        ref = G.gemv_norm_ref(inp, norm == 2, wr)
        for chain in (False, True):
            out = G.gemv_model_outputs(inp, N, K, norm, wr, chain=chain)
            yield ("gemv_norm_y", "y", out["y"], ref["y"])
            if wr:
                yield ("exact", "s", out["s"], ref["s"])


def test_budgets_are_calibrated_on_the_fp32_models():
    measured, worst = {}, {}
    for it in _model_items():
        op, name, out, (ref, unit) = it[:4]
        u = S.ulps_needed(out, ref, unit)
        if u >= measured.get(op, -1):
            measured[op], worst[op] = u, it
    print("measured smallest budgets:", measured)
    assert {op: m for op, m in measured.items() if op in G.BUDGET} == {op: b[0] for op, b in G.BUDGET.items()}, \
        "the table in _gemm_refs.py is stale"
    for op, m in measured.items():  # the rows taken over from _streaming_refs hold on these cases too
        assert m <= G.budget(op)[0], (op, m)
    for op, (m, b) in G.BUDGET.items():
        assert b == 2 * m and m > 0
        _, name, out, (ref, unit) = worst[op][:4]
        G.check_all([worst[op]])  # the worst case passes at the budget
        with pytest.raises(AssertionError):  # and fails at a zero budget
            S.assert_close_ulps(out, ref, 0, 0.0, what=f"{op}/{name}")


# ------------------------------------------------------------------------------------ the gap the checks close
# Each defect is injected into the fp32 model's output at a shape of the older tests or of the GPU file.  The
# layouts: 256 x 256 tiles, a wave 128 x 64, a lane 8 consecutive columns, a row tile 16 rows.
def test_truncating_store_is_rejected_by_the_exact_family_only():
    M, N, K = 300, 520, 128  # a shape of tests/test_gemm_gpu.py
    inp, refs = G.gemm_inputs(M, N, K), G.gemm_refs(M, N, K)
    c32 = inp["a"].float() @ inp["b"].float().t()
    trunc = G.bf16_trunc(c32)
    assert 2e-3 < G.rel_norm(trunc, refs["c"][0]) < OLD_TOL  # the older criterion accepts it
    # on random data a truncated value is within one bf16 ulp, as a correctly rounded one may be with the fp32
    # sum's own error: it is the exact family, with budget 0, that pins the rounding mode
    inp, refs = G.gemm_inputs(M, N, K, "exact"), G.gemm_refs(M, N, K, "exact")
    c32 = inp["a"].float() @ inp["b"].float().t()
    G.check_all(G.gemm_checks(inp, refs, dict(c0=c32.to(BF16))))
    _rejected(G.gemm_checks(inp, refs, dict(c0=G.bf16_trunc(c32))))
    assert G.rel_norm(G.bf16_trunc(c32), refs["c"][0]) < OLD_TOL


@functools.lru_cache(maxsize=None)
def _big():
    """(1024, 3072, 768), a shape of tests/test_gemm_gpu.py: operands and the fp32 product."""
    M, N, K = 1024, 3072, 768
    g = S._gen(21, M, N, K)
    a = torch.randn(M, K, generator=g).to(BF16)
    b = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16)
    return a, b, a.float() @ b.float().t()


def _block_items(a, b, out, rows, cols):
    """The gemm_c check of one block of C."""
    ref, ab = G.mm64(a[rows], b[cols])
    return [("gemm_c", "c0", out[rows, cols].to(BF16), (ref, S.E32 * ab))]


def test_one_lane_group_from_the_neighbouring_row_is_rejected():
    a, b, c32 = _big()
    bad = c32.to(BF16)
    rows, cols = slice(1008, 1024), slice(3064, 3072)
    G.check_all(_block_items(a, b, bad, rows, cols))
    bad[1023, cols] = bad[1022, cols]  # the last row of the last tile, its last lane group
    assert G.rel_norm(bad, c32) < OLD_TOL  # the older criterion accepts it
    _rejected(_block_items(a, b, bad, rows, cols))
    # and at a small ragged shape of the GPU file
    M, N, K = 257, 520, 128
    inp, refs = G.gemm_inputs(M, N, K), G.gemm_refs(M, N, K)
    c = G.gemm_model_outputs(M, N, K)["c0"].clone()
    c[256, 512:520] = c[255, 512:520]  # the one-row tile takes the previous tile's last row
    _rejected(G.gemm_checks(inp, refs, dict(c0=c)))


def test_missing_last_k_tile_in_one_fragment_is_rejected():
    a, b, c32 = _big()
    K = a.shape[1]
    bad = c32.clone()
    rows, cols = slice(1008, 1024), slice(3064, 3072)  # a 16 x 8 fragment of the last row tile
    bad[rows, cols] -= a[rows, K - 64:].float() @ b[cols, K - 64:].float().t()
    assert G.rel_norm(bad.to(BF16), c32) < OLD_TOL  # the older criterion accepts it
    G.check_all(_block_items(a, b, c32, rows, cols))
    _rejected(_block_items(a, b, bad, rows, cols))


def test_shifted_bias_group_is_rejected():
    M, N, K = 257, 520, 128
    inp, refs = G.gemm_inputs(M, N, K), G.gemm_refs(M, N, K)
    bias = inp["bias"].float().clone()
    bias[N - 8:] = inp["bias"].float()[N - 16:N - 8]
    bad = (inp["a"].float() @ inp["b"].float().t() + bias).to(BF16)
    _rejected(G.gemm_checks(inp, refs, dict(c0b=bad)))
    print("older criterion:", G.rel_norm(bad, refs["cb"][0]))


def test_stale_column_sum_group_is_rejected():
    M, N, K = 257, 264, 2048  # a one-row last tile: three of its four row groups hold no rows
    inp, refs = G.gemm_inputs(M, N, K), G.gemm_refs(M, N, K)
    out = G.gemm_model_outputs(M, N, K, chunked=True)
    keys = ("c0", "o3", "b3_f32", "b3_bf16")
    G.check_all(G.gemm_checks(inp, refs, {k: out[k] for k in keys}))
    for key, stale in (("b3_f32", 1e-3), ("b3_bf16", 0.25)):  # what an unwritten workspace row may hold
        bad = dict({k: out[k] for k in keys})
        bad[key] = (out[key].float() + stale).to(out[key].dtype)
        _rejected(G.gemm_checks(inp, refs, bad))


def test_missing_short_slice_is_rejected():
    name = "short_last"
    M, P, Q, Sn, sl, _ = G.WGRAD_CASES[name]
    assert M - (Sn - 1) * sl == 64  # the last slice is a single 64-token stage
    inp = G.wgrad_inputs(name)
    out = G.wgrad_model_outputs(name, "plan")
    G.check_all(G.wgrad_checks(name, out))
    last = G.wgrad_pieces_f32(inp["dy"], inp["x"], sl)[-1]
    for key in ("fresh", "acc_f32", "acc_bf16"):
        bad = out[key].float().clone()
        bad[:, :] -= last  # one tile: the whole of P x Q = 256 x 256
        _rejected(G.wgrad_checks(name, {key: bad.to(out[key].dtype)}))
    print("older criterion:", G.rel_norm((out["fresh"].float() - last).to(BF16), G.wgrad_refs(name)["w"]))


def test_hybrid_piece_added_twice_is_rejected():
    name = "hybrid"
    inp = G.wgrad_inputs(name)
    out = G.wgrad_model_outputs(name, "hybrid")
    G.check_all(G.wgrad_checks(name, out))
    piece = G.wgrad_pieces_f32(inp["dy"], inp["x"], 64 * G.WGRAD_HYBRID[name][3])[1]
    bad = out["acc_f32"].clone()
    bad[512:, 768:] += piece[512:, 768:]  # the last tile (8 x 8, ragged both ways), one of the sliced four
    _rejected(G.wgrad_checks(name, dict(acc_f32=bad)))
    print("older criterion:", G.rel_norm(bad.double(), inp["acc0"].double() + G.wgrad_refs(name)["w"]))


def test_gemv_last_wave_missing_is_rejected():
    M, N, K = 3, 2056, 768  # C = 4 columns per workgroup, 128 threads: the second wave holds chunks 64..95
    inp = G.gemv_inputs(M, N, K)
    assert G.gemv_form(N, K) == (4, 128)
    good = G.gemv_model_outputs(inp, N, K, chain=True)["y"]
    G.check_all([("gemv_y", "y", good, G.gemv_ref(inp))])
    y = inp["x"].float() @ inp["w"].float().t() + inp["bias"].float()
    cols = slice(2052, 2056)  # the last workgroup's column group
    y[:, cols] -= inp["x"].float()[:, 512:] @ inp["w"].float()[cols, 512:].t()
    _rejected([("gemv_y", "y", y.to(BF16), G.gemv_ref(inp))])
    print("older criterion:", G.rel_norm(y.to(BF16), G.gemv_ref(inp)[0]))
