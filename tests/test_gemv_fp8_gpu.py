"""Per-element checks of the weight-only FP8 decode kernels on the GPU: the FP8 arms of the skinny GEMM
(``gemv_fp8``, csrc/gemv.hip) and the per-row quantiser (``quantize_rows_fp8``, csrc/quant_fp8.hip).

References, units and budgets are those of ``tests/_fp8_refs.py`` (calibrated on the CPU by ``test_fp8_refs.py``);
the inputs are ``_gemm_refs.gemv_inputs`` with ``w`` quantised by ``quant_ref`` on the CPU.  x and res are views in
NaN-padded buffers, as in ``test_gemm_edges_gpu.py``."""
import pytest
import torch

import _fp8_refs as R
import _gemm_refs as G
import _streaming_refs as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SENT = 7.5


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _ops():
    return torch.ops.pllm


def _padded(t, pad=8):
    """``t`` [R, C] as a column slice of a NaN-filled [R + 2, C + 2 pad] buffer on the device."""
    Rr, C = t.shape
    big = torch.full((Rr + 2, C + 2 * pad), float("nan"), dtype=t.dtype, device=DEV)
    big[1:Rr + 1, pad:pad + C] = t.to(DEV)
    return big[1:Rr + 1, pad:pad + C]


def _wq(inp):
    return inp["q"].to(DEV), inp["scale"].to(DEV)


def test_decode_table_is_ocp_e4m3fn_bitwise():
    """Row n holds the n-th finite code 8 times, scale 1, x = ones: y[n] == 8 value(code) for all 254 codes (OCP
    e4m3fn, not fnuz; 8 value is exact in bf16)."""
    codes = torch.tensor(R.FINITE_CODES, dtype=torch.uint8)
    wq = codes[:, None].expand(-1, 8).contiguous().to(DEV)
    y = _ops().gemv_fp8(torch.ones(1, 8, dtype=BF16, device=DEV), wq, torch.ones(254, device=DEV), None)[0]
    want = (8.0 * R.code_values()[list(R.FINITE_CODES)] + 0.0).to(BF16)  # (+ 0: the sum of the -0 code's products is +0)
    assert torch.equal(y[0].cpu().view(torch.int16), want.view(torch.int16))


def test_decode_byte_order_within_the_chunk():
    """x = one-hot at element e: y == value(code at byte e), for every byte of two 8-byte chunks."""
    K = 16
    wq = (torch.arange(K, dtype=torch.int32) * 7 + 0x21).to(torch.uint8)[None].repeat(3, 1)
    wq[1] += 0x40
    wq[2] += 0x80
    y = _ops().gemv_fp8(torch.eye(8, K, dtype=BF16, device=DEV), wq.to(DEV), torch.ones(3, device=DEV), None)[0]
    y2 = _ops().gemv_fp8(torch.eye(K, dtype=BF16, device=DEV)[8:], wq.to(DEV), torch.ones(3, device=DEV), None)[0]
    want = R.values_of(wq).to(BF16)  # [3, K]
    assert torch.equal(torch.cat([y, y2]).cpu().t(), want)


@pytest.mark.parametrize("M", G.GEMV_M)
def test_gemv_fp8_edges(M):
    """Plain calls over the dispatch seams in N (columns per workgroup 1 -> 2 -> 4, split-K form -> wide form, a
    ragged wave) and K (one chunk, a partly idle second wave, full), the bias alternating; below the wide form
    also GELU / ReLU from the kernel's own pre-activation."""
    for M_, N, K, bias in G.gemv_cases():
        if M_ != M:
            continue
        inp = R.fp8_inputs(M, N, K)
        x, (q, sc) = _padded(inp["x"]), _wq(inp)
        b = inp["bias"].to(DEV) if bias else None
        y, s = _ops().gemv_fp8(x, q, sc, b)
        assert y.shape == (M, N) and y.dtype == BF16 and s.numel() == 0
        R.check_all([("gemv_fp8_y", f"y {N}x{K}", y.cpu(), R.gemv_fp8_ref(inp, bias))])
        if N < 8192:
            g = _ops().gemv_fp8(x, q, sc, b, None, None, None, 1e-5, 0, 1)[0]
            r = _ops().gemv_fp8(x, q, sc, b, None, None, None, 1e-5, 0, 2)[0]
            R.check_all([("gelu_fwd", f"gelu {N}x{K}", g.cpu(), S.gelu_ref(y.cpu())),
                         ("exact", f"relu {N}x{K}", r.cpu(), S.relu_ref(y.cpu()))])


@pytest.mark.parametrize("M,N,K,norm,with_res", G.gemv_norm_cases())
def test_gemv_fp8_norm_prologue_edges(M, N, K, norm, with_res):
    """LayerNorm / RMSNorm prologue with and without the residual; s must be bitwise the bf16 sum."""
    inp = R.fp8_inputs(M, N, K, norm)
    ref = R.gemv_fp8_norm_ref(inp, norm == 2, with_res)
    x, (q, sc), b = _padded(inp["x"]), _wq(inp), inp["bias"].to(DEV)
    res = _padded(inp["res"]) if with_res else None
    gamma, beta = inp["gamma"].to(DEV), None if norm == 2 else inp["beta"].to(DEV)
    args = (x, q, sc, b, res, gamma, beta, G.GEMV_EPS, int(norm == 2))
    y, s = _ops().gemv_fp8(*args, 0)
    items = [("gemv_fp8_norm_y", "y", y.cpu(), ref["y"])]
    if with_res:
        items.append(("exact", "s", s.cpu(), ref["s"]))
    else:
        assert s.numel() == 0
    g, r = _ops().gemv_fp8(*args, 1)[0], _ops().gemv_fp8(*args, 2)[0]
    items += [("gelu_fwd", "gelu", g.cpu(), S.gelu_ref(y.cpu())), ("exact", "relu", r.cpu(), S.relu_ref(y.cpu()))]
    R.check_all(items)


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("slot", ["first", "last", "outside"])
def test_gemv_fp8_kv_append_edges(per_row, slot):
    """The KV-cache append at slot 0 and S_max - 1, ``pos`` as [1] and as [M]: the slot equals the K / V columns of
    y bitwise and every other cache slot keeps its sentinel; a position outside [0, S_max) writes nothing."""
    M, K, q_cols, kv_cols, S_max = 3, 520, 520, 256, 4
    N = q_cols + 2 * kv_cols
    inp = R.fp8_inputs(M, N, K)
    x, (q, sc), b = _padded(inp["x"]), _wq(inp), inp["bias"].to(DEV)
    kc = torch.full((M, S_max, 4, 64), SENT, dtype=BF16, device=DEV)
    vc = torch.full_like(kc, -SENT)
    p = {"first": 0, "last": S_max - 1, "outside": S_max}[slot]
    rows = [p, S_max - 1 - p if slot != "outside" else -1, p] if per_row else [p] * M
    pos = torch.tensor(rows if per_row else [p], device=DEV)
    y = _ops().gemv_fp8(x, q, sc, b, None, None, None, 1e-5, 0, 0, kc, vc, pos, q_cols)[0]
    R.check_all([("gemv_fp8_y", "y", y.cpu(), R.gemv_fp8_ref(inp))])
    for m in range(M):
        inside = 0 <= rows[m] < S_max
        if inside:
            assert torch.equal(kc[m, rows[m]].reshape(-1), y[m, q_cols:q_cols + kv_cols])
            assert torch.equal(vc[m, rows[m]].reshape(-1), y[m, q_cols + kv_cols:])
        for sl in range(S_max):
            if not inside or sl != rows[m]:
                assert (kc[m, sl] == SENT).all() and (vc[m, sl] == -SENT).all(), (m, sl)


@pytest.mark.parametrize("N", [2056, 8200])
def test_gemv_fp8_scale_seam(N):
    """Neighbouring rows' scales 2^20 apart, across the columns of a workgroup and across workgroups (split-K form,
    4 columns each; wide form, a wave 4 columns): a scale indexed by workgroup or wave is far out of bound."""
    M, K = 3, 520
    inp = R.fp8_inputs(M, N, K, seam=True)
    y = _ops().gemv_fp8(_padded(inp["x"]), *_wq(inp), inp["bias"].to(DEV))[0]
    R.check_all([("gemv_fp8_y", f"y {N}", y.cpu(), R.gemv_fp8_ref(inp))])


def test_gemv_fp8_is_deterministic():
    for M, N, K in ((8, 2056, 768), (5, 8197, 520)):
        inp = R.fp8_inputs(M, N, K)
        args = (_padded(inp["x"]), *_wq(inp), inp["bias"].to(DEV))
        assert torch.equal(_ops().gemv_fp8(*args)[0], _ops().gemv_fp8(*args)[0])


def test_gemv_fp8_host_checks():
    inp = R.fp8_inputs(1, 1024, 8)
    x, (q, sc) = inp["x"].to(DEV), _wq(inp)
    with pytest.raises(RuntimeError):
        _ops().gemv_fp8(x, q.view(torch.int8), sc, None)          # not uint8
    with pytest.raises(RuntimeError):
        _ops().gemv_fp8(x, q, sc[:-1].contiguous(), None)         # scale [N]
    with pytest.raises(RuntimeError):
        _ops().gemv_fp8(x, q, sc.to(BF16), None)                  # scale fp32
    with pytest.raises(RuntimeError):
        _ops().gemv_fp8(x, q.t().contiguous().t(), sc, None)      # not contiguous
    with pytest.raises(RuntimeError):
        _ops().gemv_fp8(torch.zeros(9, 8, dtype=BF16, device=DEV), q, sc, None)  # more than gemv_max_rows()


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("N,K", R.QUANT_SHAPES)
def test_quantize_rows_fp8_matches_the_reference_bitwise(N, K):
    """Codes and scales equal ``quant_ref`` bitwise: random rows, an all-zero row, +-amax at a row's end, a row of
    planted exact ties (to even); w is a row-strided view."""
    w = R.quant_inputs(N, K)
    q_ref, s_ref = R.quant_ref(w)
    q, s = _ops().quantize_rows_fp8(_padded(w))
    assert q.dtype == torch.uint8 and q.shape == (N, K) and q.is_contiguous() and s.dtype == F32 and s.shape == (N,)
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32))
    bad = (q.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), q.cpu()[tuple(bad[0])], q_ref[tuple(bad[0])])
    q2, s2 = _ops().quantize_rows_fp8(w.to(DEV))  # contiguous, and again: deterministic
    assert torch.equal(q2, q) and torch.equal(s2, s)


def test_ops_quantize_weight_fp8_on_the_gpu():
    from pretraining_llm_amd import ops
    w = R.quant_inputs(300, 520).to(DEV)
    fw = ops.quantize_weight_fp8(w)
    q_ref, s_ref = R.quant_ref(w)
    assert fw.ref is w and fw.shape == w.shape and torch.equal(fw.q.cpu(), q_ref) and torch.equal(fw.scale.cpu(), s_ref)
    assert torch.equal(ops.dequantize_fp8(fw.q, fw.scale).cpu(), R.dq64(q_ref, s_ref).float())
    assert ops.quantize_weight_fp8(w[:, :516]) is None and ops.quantize_weight_fp8(w[:, :512]) is None  # K, strides
    assert ops.quantize_weight_fp8(w.float()) is None  # a GPU weight off the HIP path
    bad = w.clone()
    bad[7, 3] = float("inf")
    with pytest.raises(ValueError):
        ops.quantize_weight_fp8(bad)
    x = R.fp8_inputs(3, 1032, 520)["x"].to(DEV)
    with torch.no_grad():
        y = ops.linear(x, fw)
        y9 = ops.linear(torch.cat([x, x, x]), fw)
    assert torch.equal(y, _ops().gemv_fp8(x, fw.q, fw.scale, None)[0])
    assert torch.equal(y9, torch.nn.functional.linear(torch.cat([x, x, x]), w))  # 9 rows: the bf16 weight
