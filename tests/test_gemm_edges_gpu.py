"""The GEMM family's HIP kernels, element by element against the fp64 references of ``_gemm_refs`` at tile edges
and on every dispatch arm: ``gemm_tn`` (csrc/gemm_pp.hip, its fallback csrc/gemm.hip), ``wgrad``
(csrc/gemm_wgrad.hip, csrc/wgrad_pp.hip and its hybrid form) and the decode ``gemv`` (csrc/gemv.hip).

Every case asserts the arm it was written for through ``torch.ops.pllm.gemm_plan`` / ``wgrad_plan``, so a changed
threshold or cost model fails here instead of moving the case onto another kernel.

gemm_tn shapes (M, N, K); tiles are 256 x 256, a wave covers 128 x 64, a lane 8 columns, a row tile 16 rows:
    (1, 8, 128)        one row, one lane group, two K-tiles with no middle one
    (17, 72, 128)      a second row tile, a second wave column
    (129, 264, 192)    one row into the second wave group, 8 columns into a second tile (aux also on the grid)
    (257, 520, 128)    a one-row tile
    (300, 264, 64)     K = 64: the fallback kernel under the default config
    (257, 264, 2048)   quadrant epilogues on
    (520, 776, 2112)   3 x 4 ragged tiles, an odd K-tile count, quadrant epilogues
    (520, 776, 192)    3 x 4 ragged tiles
Operands and aux are views inside NaN-padded buffers (an over-read in K or past a row shows as NaN), and the
column-sum workspace of epilogues 3 / 4 is handed back by the allocator full of NaN."""
import contextlib

import pytest
import torch

import _gemm_refs as G
import _streaming_refs as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DEFAULT = (16, 4, 4, 0, 1)   # mfma, group_m, phased (4: the ping-pong kernel), reserve_cus, persistent
ALL_CUS = 1 << 20            # reserve_cus that leaves the persistent grids their floor of 8 workgroups
SENT = 7.5


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _ops():
    return torch.ops.pllm


@contextlib.contextmanager
def gemm_config(mfma=16, group_m=4, phased=4, reserve=0, persistent=1):
    _ops().gemm_set_config(mfma, group_m, phased, reserve, persistent)
    try:
        yield
    finally:
        _ops().gemm_set_config(*DEFAULT)


def _padded(t, pad=64):
    """``t`` [R, C] as a column slice of a NaN-filled [R + 2, C + 2 pad] buffer on the device."""
    R, C = t.shape
    big = torch.full((R + 2, C + 2 * pad), float("nan"), dtype=t.dtype, device=DEV)
    big[1:R + 1, pad:pad + C] = t.to(DEV)
    return big[1:R + 1, pad:pad + C]


def _poison(rows, cols):
    """NaN-filled fp32 blocks of the column-sum workspace's size, freed so that the op's at::empty gets one of them
    (several: the op's small outputs may round to the same block size and take the first)."""
    blocks = [torch.full((rows, cols), float("nan"), dtype=F32, device=DEV) for _ in range(4)]
    del blocks


def _expect_plan(M, N, K, epi, phased=4, T=0, grid=None):
    """The arm a case was written for (``_gemm_refs.expect_gemm_plan``), asserted on the op's plan."""
    head, tail = G.expect_gemm_plan(M, N, K, epi, phased, T)
    plan = list(_ops().gemm_plan(M, N, K, epi, T))
    assert plan[:2] == head and plan[3:] == tail, (plan, (M, N, K, epi))
    if grid is not None:
        assert plan[2] == grid, plan
    return plan


def _run_gemm(inp, M, N, K, phased=4, grid=None, keys=None):
    """Every epilogue the contract allows at this shape -> the outputs ``_gemm_refs.gemm_checks`` names."""
    want = lambda k: keys is None or k in keys  # noqa: E731
    a, b, bias = _padded(inp["a"]), inp["b"].to(DEV), inp["bias"].to(DEV)
    out = {}
    for e in range(6):
        _expect_plan(M, N, K, e, phased, grid=grid)
    out["c0"] = _ops().gemm_tn(a, b, None, 0)[0]
    if want("c0b"):
        out["c0b"] = _ops().gemm_tn(a, b, bias, 0)[0]
    if want("pre1"):
        out["act1"], out["pre1"] = _ops().gemm_tn(a, b, bias, 1)
    if want("y2"):
        out["y2"] = _ops().gemm_tn(a, b, bias, 2)[0]
    if want("o3"):
        aux = _padded(inp["aux"])
        groups = _ops().gemm_plan(M, N, K, 3)[5]
        for e, ax in ((3, aux), (4, _padded(S.relu_of(inp["aux"])))):
            for nm, dt in (("f32", F32), ("bf16", BF16)):
                acc = inp["fill"].to(dt).to(DEV)
                _poison(groups, N)
                o = _ops().gemm_tn(a, b, None, e, ax, acc)[0]
                assert torch.equal(out.setdefault(f"o{e}", o), o)
                out[f"b{e}_{nm}"] = acc
        out["o5"] = _ops().gemm_tn(a, b, None, 5, _padded(inp["gu"]))[0]
    if want("gu7") and phased == 4 and K >= 128:
        _expect_plan(M, N, K, 7, phased)
        out["a7"], out["gu7"] = _ops().gemm_tn(a, inp["b7"].to(DEV), None, 7)
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.isfinite(v.float()).all(), f"{k}: not finite"
    return out


def _cpu(out):
    return {k: v.cpu() for k, v in out.items()}


EXACT_KEYS = ("c0", "c0b", "pre1", "gu7")
KERNELS = [(16, 4), (16, 0)]  # the default (ping-pong, with the fallback at K = 64) and the round-3 kernel


@pytest.mark.parametrize("mf,phased", KERNELS)
@pytest.mark.parametrize("data", ["randn", "exact"])
@pytest.mark.parametrize("M,N,K", G.GEMM_SHAPES)
def test_gemm_tn_edges(M, N, K, data, mf, phased):
    """Every epilogue at every edge shape, on the default kernel and the round-3 kernel.  ``exact``: integer
    operands, budget 0 on C (the rounding mode, ties included)."""
    aux = "grid" if (M, N, K) == G.GEMM_GRID_AUX and data == "randn" else "randn"
    inp, refs = G.gemm_inputs(M, N, K, data, aux), G.gemm_refs(M, N, K, data, aux)
    with gemm_config(mf, 4, phased):
        out = _run_gemm(inp, M, N, K, phased, keys=EXACT_KEYS if data == "exact" else None)
    G.check_all(G.gemm_checks(inp, refs, _cpu(out)))


@pytest.mark.parametrize("mf,phased", [(32, 0), (16, 2), (32, 2)])
@pytest.mark.parametrize("M,N,K", G.GEMM_TILED)
def test_gemm_tn_edges_other_fallback_kernels(M, N, K, mf, phased):
    """The fallback file's 32x32x16 and asymmetric-DMA instantiations on the 3 x 4-tile shapes."""
    inp, refs = G.gemm_inputs(M, N, K), G.gemm_refs(M, N, K)
    with gemm_config(mf, 4, phased):
        out = _run_gemm(inp, M, N, K, phased)
    G.check_all(G.gemm_checks(inp, refs, _cpu(out)))


GRIDS = {"grid8": dict(reserve=ALL_CUS), "per_tile": dict(persistent=0), "group_m1": dict(group_m=1),
         "group_m3": dict(group_m=3), "grid8_group_m3": dict(reserve=ALL_CUS, group_m=3)}


@pytest.mark.parametrize("variant", list(GRIDS))
@pytest.mark.parametrize("M,N,K", G.GEMM_TILED)
def test_gemm_tn_grids_agree_bitwise(M, N, K, variant):
    """12 tiles on 8 workgroups (some run two tiles, some one: the only way to the quadrant epilogues' carry from
    tile to tile -- aux rows, column sums -- at a small shape), one workgroup per tile, and tile groups with a
    short last group: every output of every epilogue equals the default grid's bit for bit (which
    ``test_gemm_tn_edges`` holds against fp64)."""
    inp = G.gemm_inputs(M, N, K)
    base = _run_gemm(inp, M, N, K, grid=12)
    with gemm_config(**GRIDS[variant]):
        out = _run_gemm(inp, M, N, K, grid=8 if "grid8" in variant else 12)
    assert set(out) == set(base)
    for k in base:
        assert torch.equal(out[k], base[k]), k


@pytest.mark.parametrize("phased", [4, 0])
@pytest.mark.parametrize("B,T,N,K", G.DELTA_CASES)
def test_gemm_tn_delta_edges(B, T, N, K, phased):
    """Epilogue 6 with batch boundaries inside a tile (T = 112), on the fallback arm (T = 200) and, on 3 x 4 tiles,
    on a grid of 8 workgroups: dO equals the epilogue-0 output bitwise, dO and delta hold against fp64."""
    M = B * T
    inp = G.delta_inputs(B, T, N, K)
    a, b, o = _padded(inp["a"]), inp["b"].to(DEV), _padded(inp["o"])
    grids = [dict()] + ([dict(reserve=ALL_CUS)] if N > 768 else [])
    outs = []
    for g in grids:
        with gemm_config(16, 4, phased, **g):
            plan = _expect_plan(M, N, K, 6, phased, T)
            assert plan[0] == int(phased == 4 and T % 16 == 0) and (not g or plan[2] == 8), plan
            do, delta = _ops().gemm_tn(a, b, None, 6, o, None, T)
            assert delta.shape == (B, N // 64, T) and delta.dtype == F32
            assert torch.equal(do, _ops().gemm_tn(a, b, None, 0)[0])
            outs.append((do, delta))
    G.check_all(G.delta_checks(inp, B, T, dict(do6=outs[0][0].cpu(), delta6=outs[0][1].cpu())))
    for do, delta in outs[1:]:
        assert torch.equal(do, outs[0][0]) and torch.equal(delta, outs[0][1])


@pytest.mark.parametrize("data", ["randn", "exact"])
def test_gemm_tn_swiglu_forward_f136(data):
    """Epilogue 7 at F = 136: a 128-column tile plus 8 columns, gate and up rows 136 apart in W1."""
    M, N, K = G.SWIGLU_F136
    inp, refs = G.gemm_inputs(M, N, K, data), G.gemm_refs(M, N, K, data)
    plan = _expect_plan(M, N, K, 7)
    assert plan[4] == 2
    a7, gu7 = _ops().gemm_tn(_padded(inp["a"]), inp["b7"].to(DEV), None, 7)
    assert a7.shape == (M, N) and gu7.shape == (M, 2 * N)
    G.check_all(G.gemm_checks(inp, refs, dict(a7=a7.cpu(), gu7=gu7.cpu())))


# ------------------------------------------------------------------------------------------------ wgrad
def _sentinel_view(t, dtype):
    """``t`` [P, Q] as a view in the middle of a sentinel-filled buffer."""
    P, Q = t.shape
    buf = torch.full((P * Q + 128,), SENT, dtype=dtype, device=DEV)
    v = buf[64:64 + P * Q].view(P, Q)
    v.copy_(t.to(dtype))
    return buf, v


@pytest.mark.parametrize("name", list(G.WGRAD_CASES))
def test_wgrad_edges(name):
    """Fresh bf16 output, bf16 and fp32 accumulation (the target a view between sentinels), the fused bias
    gradient, on every kernel the case has; repeated calls agree bitwise."""
    M, P, Q, S_, slice_rows, grid8 = G.WGRAD_CASES[name]
    inp = G.wgrad_inputs(name)
    dy, x = _padded(inp["dy"]), inp["x"].to(DEV)
    try:
        with gemm_config(reserve=ALL_CUS if grid8 else 0):
            for mf in (0, 16, 32):
                _ops().wgrad_set_mfma(mf)
                for of32 in (False, True):
                    for bias in (False, True):
                        plan = list(_ops().wgrad_plan(M, P, Q, of32, bias))
                        assert plan == G.expect_wgrad_plan(name, mf, of32, bias), (plan, mf, of32, bias)

                def run():
                    out = dict(fresh=_ops().wgrad(dy, x))
                    for nm, dt in (("f32", F32), ("bf16", BF16)):
                        buf, v = _sentinel_view(inp["acc0"], dt)
                        _ops().wgrad(dy, x, v)
                        assert (buf[:64] == SENT).all() and (buf[-64:] == SENT).all(), f"{nm}: sentinels overwritten"
                        out[f"acc_{nm}"] = v.clone()
                        buf, v = _sentinel_view(inp["acc0"], F32)
                        b = inp["b0"].to(dt).to(DEV)
                        _ops().wgrad(dy, x, v, b)
                        assert (buf[:64] == SENT).all() and (buf[-64:] == SENT).all(), f"bias {nm}: sentinels"
                        out[f"bias_{nm}"], out[f"acc_with_bias_{nm}"] = b, v.clone()
                    return out

                out, again = run(), run()
                for k in out:
                    assert torch.equal(out[k], again[k]), (mf, k)
                cpu = _cpu(out)
                G.check_all(G.wgrad_checks(name, cpu))
                G.check_all(G.wgrad_checks(name, dict(acc_f32=cpu["acc_with_bias_f32"])))
                G.check_all(G.wgrad_checks(name, dict(acc_f32=cpu["acc_with_bias_bf16"])))
    finally:
        _ops().wgrad_set_mfma(0)


# ------------------------------------------------------------------------------------------------ gemv
@pytest.mark.parametrize("M", G.GEMV_M)
def test_gemv_edges(M):
    """Plain calls over the dispatch seams in N (columns per workgroup 1 -> 2 -> 4, split-K form -> wide form, a
    ragged wave) and K (one chunk, a partly idle second wave, full), x a view in a NaN-padded buffer; below the
    wide form also GELU / ReLU from the kernel's own pre-activation."""
    for M_, N, K, bias in G.gemv_cases():
        if M_ != M:
            continue
        inp = G.gemv_inputs(M, N, K)
        x, w = _padded(inp["x"], 8), inp["w"].to(DEV)
        b = inp["bias"].to(DEV) if bias else None
        y, s = _ops().gemv(x, w, b)
        assert y.shape == (M, N) and s.numel() == 0
        G.check_all([("gemv_y", f"y {N}x{K}", y.cpu(), G.gemv_ref(inp, bias))])
        if N < 8192:  # (with an activation the wide sizes run the split-K form: another pre-activation)
            g = _ops().gemv(x, w, b, None, None, None, 1e-5, 0, 1)[0]
            r = _ops().gemv(x, w, b, None, None, None, 1e-5, 0, 2)[0]
            G.check_all([("gelu_fwd", f"gelu {N}x{K}", g.cpu(), S.gelu_ref(y.cpu())),
                         ("exact", f"relu {N}x{K}", r.cpu(), S.relu_ref(y.cpu()))])


@pytest.mark.parametrize("M,N,K,norm,with_res", G.gemv_norm_cases())
def test_gemv_norm_prologue_edges(M, N, K, norm, with_res):
    """LayerNorm / RMSNorm prologue (an all-equal row included), with and without the residual, then GELU / ReLU
    from the kernel's own pre-activation; N = 8197 keeps the split-K form with a ragged last workgroup."""
    inp = G.gemv_inputs(M, N, K, norm)
    ref = G.gemv_norm_ref(inp, norm == 2, with_res)
    x, w, b = _padded(inp["x"], 8), inp["w"].to(DEV), inp["bias"].to(DEV)
    res = _padded(inp["res"], 8) if with_res else None
    gamma, beta = inp["gamma"].to(DEV), None if norm == 2 else inp["beta"].to(DEV)
    args = (x, w, b, res, gamma, beta, G.GEMV_EPS, int(norm == 2))
    y, s = _ops().gemv(*args, 0)
    items = [("gemv_norm_y", "y", y.cpu(), ref["y"])]
    if with_res:
        items.append(("exact", "s", s.cpu(), ref["s"]))
    else:
        assert s.numel() == 0
    g, r = _ops().gemv(*args, 1)[0], _ops().gemv(*args, 2)[0]
    items += [("gelu_fwd", "gelu", g.cpu(), S.gelu_ref(y.cpu())), ("exact", "relu", r.cpu(), S.relu_ref(y.cpu()))]
    G.check_all(items)


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("slot", ["first", "last"])
def test_gemv_kv_append_edges(per_row, slot):
    """The KV-cache append at slot 0 and S_max - 1, ``pos`` as [1] and as [M]: the slot equals the K / V columns of
    y bitwise and every other cache slot keeps its sentinel."""
    M, K, q_cols, kv_cols, S_max = 3, 520, 520, 256, 4
    N = q_cols + 2 * kv_cols
    inp = G.gemv_inputs(M, N, K)
    x, w, b = _padded(inp["x"], 8), inp["w"].to(DEV), inp["bias"].to(DEV)
    kc = torch.full((M, S_max, 4, 64), SENT, dtype=BF16, device=DEV)
    vc = torch.full_like(kc, -SENT)
    p = 0 if slot == "first" else S_max - 1
    rows = [p, S_max - 1 - p, p] if per_row else [p] * M
    pos = torch.tensor(rows if per_row else [p], device=DEV)
    y = _ops().gemv(x, w, b, None, None, None, 1e-5, 0, 0, kc, vc, pos, q_cols)[0]
    G.check_all([("gemv_y", "y", y.cpu(), G.gemv_ref(inp))])
    for m in range(M):
        assert torch.equal(kc[m, rows[m]].reshape(-1), y[m, q_cols:q_cols + kv_cols])
        assert torch.equal(vc[m, rows[m]].reshape(-1), y[m, q_cols + kv_cols:])
        for sl in range(S_max):
            if sl != rows[m]:
                assert (kc[m, sl] == SENT).all() and (vc[m, sl] == -SENT).all(), (m, sl)
