"""References, case builders and budgets for the weight-only FP8 decode path: the per-row e4m3fn quantiser
(csrc/quant_fp8.hip) and the FP8 arms of the skinny GEMM (``gemv_fp8``, csrc/gemv.hip).

Not collected by pytest.  ``test_fp8_refs.py`` (CPU) checks the references, calibrates the budgets below and shows
which defects the checks reject; ``test_gemv_fp8_gpu.py`` runs the HIP kernels on the same cases under the same
bounds; ``test_fp8_decode.py`` / ``test_fp8_decode_gpu.py`` use ``snap_to_fp8_grid`` for a model whose quantisation
is lossless.  The bound is the project's (``_streaming_refs.assert_close_ulps``):

    |out - ref| <= budget * (ulp_bf16(ref) + unit)

Quantiser (``quant_ref``): scale_n = max_k |w_nk| / 448 in fp32 (1 for an all-zero row), code = the e4m3fn value
nearest to fl32(w_nk / scale_n), ties to even -- PyTorch's CPU conversion to ``torch.float8_e4m3fn``.  The kernel
must match it bitwise, codes and scales.

gemv_fp8: ref = x . dq64^T + bias in fp64 with dq64 = value(code) * scale, unit = 2^-23 (scale_n sum_k |x||code|
+ |bias|): the kernel sums code * x products in fp32 (the code -> fp32 convert is exact), multiplies the sum by the
scale once and adds the bias.  With the norm prologue the reference is ``_gemm_refs.gemv_norm_ref`` fed the fp64
dequantised matrix as ``w``.  The inputs are ``_gemm_refs.gemv_inputs`` with ``w`` quantised by ``quant_ref``, the
dispatch seams are those of the bf16 kernel (the FP8 arms keep its lane <-> K mapping: ``_gemm_refs.GEMV_N`` /
``GEMV_K`` / ``gemv_form``).

Budgets, by the convention of ``_gemm_refs``: ``measured`` is the smallest integer budget at which a CPU fp32 model
passes on all cases -- the larger of a torch fp32 matmul on the codes and ``gemv_chain_f32`` on the codes, each
followed by * scale, + bias and rounding to bf16 --, ``budget`` twice that.  ``test_fp8_refs.py`` recomputes
``measured`` and fails when a row is stale; nothing was tuned against kernel output.

    op                measured  budget   outputs
    ----------------  --------  ------   ---------------------------------------------------
    gemv_fp8_y               1       2   gemv_fp8 y (bf16), no norm prologue
    gemv_fp8_norm_y          2       4   gemv_fp8 y (bf16) with the LayerNorm / RMSNorm prologue
"""
from __future__ import annotations

import functools

import torch

import _gemm_refs as G
import _streaming_refs as S
from _streaming_refs import BF16, E32, F32, F64, _gen

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0

BUDGET = {
    "gemv_fp8_y": (1, 2),
    "gemv_fp8_norm_y": (2, 4),
}


def budget(op):
    return BUDGET[op] if op in BUDGET else G.budget(op)


def check_all(items):
    """``_gemm_refs.check_all`` over this file's table too: (op, name, out, (ref64, unit)) tuples."""
    for it in items:
        (ref, unit), u = it[3], budget(it[0])[1]
        S.assert_close_ulps(it[2], ref, u, u * torch.as_tensor(unit, dtype=F64), f"{it[0]}/{it[1]}")


# ------------------------------------------------------------------------------------------------ codes
def code_values():
    """fp32 value of each of the 256 codes (0x7f / 0xff: NaN)."""
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).view(FP8).to(F32)


FINITE_CODES = tuple(c for c in range(256) if c & 0x7f != 0x7f)  # 254


def values_of(q):
    """fp32 values of a uint8 code tensor (the conversion is exact)."""
    return q.view(FP8).to(F32)


# ------------------------------------------------------------------------------------------------ quantiser
def quant_ref(w):
    """(codes uint8 [N, K], scale fp32 [N]) of a bf16 / fp32 matrix, on the CPU."""
    wf = w.detach().cpu().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / FP8_MAX)
    return (wf / scale[:, None]).to(FP8).view(torch.uint8), scale


def dq64(q, scale):
    return values_of(q.cpu()).to(F64) * scale.cpu().to(F64)[:, None]


def quotients(w, scale):
    """t = fl32(w / scale): what the quantiser rounds."""
    return w.detach().cpu().float() / scale[:, None]


def nearest_code_report(w, q, scale):
    """Checks of a quantisation against its definition -> dict(violations, ties, odd_ties, nan_codes, sign_flips,
    bad_scales).  A violation: |t - value(code)| exceeds the distance from t to its nearest finite code (t the fp32
    quotient); a tie: t exactly half way between two neighbouring codes; an odd tie: one that took the code with
    the odd mantissa."""
    wf = w.detach().cpu().float()
    amax = wf.abs().amax(dim=1)
    want = torch.where(amax == 0, torch.ones_like(amax), amax / FP8_MAX)
    t = quotients(w, want).to(F64)
    pos = torch.tensor(sorted(float(code_values()[c]) for c in FINITE_CODES if c < 0x80), dtype=F64)  # 0 .. 448
    ta = t.abs().clamp(max=FP8_MAX)
    hi = torch.searchsorted(pos, ta.contiguous()).clamp(1, pos.numel() - 1)
    lo = hi - 1
    best = torch.minimum((ta - pos[lo]).abs(), (ta - pos[hi]).abs()) + (t.abs() - ta)
    v = values_of(q).to(F64)
    tie = ((ta - pos[lo]) == (pos[hi] - ta)) & (pos[lo] != pos[hi])
    return dict(violations=int(((t - v).abs() > best).sum()), ties=int(tie.sum()),
                odd_ties=int((tie & (q.cpu() & 1).bool()).sum()), nan_codes=int(((q & 0x7f) == 0x7f).sum()),
                sign_flips=int(((v != 0) & ((v < 0) != (wf < 0))).sum()),
                bad_scales=int((scale.cpu() != want).sum()))


def quant_trunc(w):
    """The defect: quotients rounded toward zero instead of to nearest."""
    _, scale = quant_ref(w)
    t = quotients(w, scale)
    q, _ = quant_ref(w)
    v = values_of(q)
    over = v.abs() > t.abs()  # rounded away from zero: step one code back toward zero
    return torch.where(over, q - 1, q), scale


def quant_amax240(w):
    """The defect: the e4m3 fnuz range (240) as the divisor."""
    wf = w.detach().cpu().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 240.0)
    return (wf / scale[:, None]).to(FP8).view(torch.uint8), scale


QUANT_SHAPES = ((300, 520), (5, 8))


@functools.lru_cache(maxsize=None)
def quant_inputs(N, K):
    """randn / sqrt(K) bf16 weights; at N >= 4 row 1 is all zero, row 2 holds +-amax at its last two elements and
    row 3 is planted on exact ties: the mid-points of neighbouring codes (normal and subnormal) under the
    power-of-two scale that its +-448 * 2^-7 entries fix."""
    g = _gen(31, N, K)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16)
    if N >= 4:
        w[1] = 0.0
        w[2, -1], w[2, -2] = 3.0, -3.0
        pos = torch.tensor(sorted(float(code_values()[c]) for c in FINITE_CODES if c < 0x80))
        mid = (pos[:-1] + pos[1:]) / 2          # 126 mid-points, 5 significant bits each
        row = torch.cat([mid, -mid])[torch.arange(K) % (2 * mid.numel())] * 2.0 ** -7
        row[0], row[1] = FP8_MAX * 2.0 ** -7, -FP8_MAX * 2.0 ** -7
        w[3] = row.to(BF16)
        assert torch.equal(w[3].float(), row)
    return w


# ------------------------------------------------------------------------------------------------ gemv_fp8
@functools.lru_cache(maxsize=None)
def fp8_inputs(M, N, K, norm=0, seam=False):
    """``_gemm_refs.gemv_inputs`` plus q / scale = quant_ref(w).  ``seam``: the rows of w alternate between 2^10
    and 2^-10 times their values, so that neighbouring scales differ by 2^20."""
    inp = dict(G.gemv_inputs(M, N, K, norm))
    if seam:
        f = torch.where(torch.arange(N) % 2 == 0, 2.0 ** 10, 2.0 ** -10)[:, None]
        inp["w"] = (inp["w"].float() * f).to(BF16)
    inp["q"], inp["scale"] = quant_ref(inp["w"])
    return inp


def gemv_fp8_ref(inp, bias=True):
    xd, cd, sd = inp["x"].to(F64), values_of(inp["q"]).to(F64), inp["scale"].to(F64)
    bd = inp["bias"].to(F64) if bias else torch.zeros(1, dtype=F64)
    return (xd @ cd.t()) * sd + bd, E32 * ((xd.abs() @ cd.abs().t()) * sd + bd.abs())


def gemv_fp8_norm_ref(inp, rms, with_res, bias=True):
    return G.gemv_norm_ref(dict(inp, w=dq64(inp["q"], inp["scale"])), rms, with_res, bias)


def gemv_fp8_model(inp, N, K, norm=0, with_res=False, bias=True, chain=False):
    """fp32 CPU model -> dict(y bf16, s, acc fp32 [the sum before the scale]).  ``chain``: the kernel's order."""
    if not norm:
        xin, s = inp["x"], None
    else:  # the bf16 model's normalised input (its GEMM operand), from _gemm_refs.gemv_model_outputs
        s = (inp["x"].float() + inp["res"].float()).to(BF16) if with_res else inp["x"]
        sf = s.float()
        if chain:
            mean = torch.zeros(sf.shape[0], 1) if norm == 2 else sf.mean(-1, keepdim=True)
            var = ((sf * sf).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
            xin = ((sf - mean) * torch.rsqrt(var + G.GEMV_EPS) * inp["gamma"].float()
                   + (0.0 if norm == 2 else inp["beta"].float())).to(BF16)
        elif norm == 2:
            xin = (sf * torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + G.GEMV_EPS) * inp["gamma"].float()).to(BF16)
        else:
            xin = torch.nn.functional.layer_norm(sf, (K,), inp["gamma"].float(), inp["beta"].float(),
                                                 G.GEMV_EPS).to(BF16)
    codes = values_of(inp["q"])
    if chain:
        acc = G.gemv_chain_f32(xin, codes, None, G.gemv_form(N, K, split_only=bool(norm)))
    else:
        acc = xin.float() @ codes.t()
    y = acc * inp["scale"] + (inp["bias"].float() if bias else 0.0)
    return dict(y=y.to(BF16), s=s if with_res else None, acc=acc)


# ------------------------------------------------------------------------------------------------ lossless model
def snap_to_fp8_grid(model):
    """Move every weight that ``GPT.quantize_decode_weights`` quantises onto the e4m3fn grid: per row a power-of-two
    scale s >= amax / 448, every element replaced by s * (nearest code value of w / s), and +-448 s planted in the
    row's first two elements, so that the quantiser's scale is exactly s, its codes reproduce the row exactly, and
    the values (4 significant bits times a power of two) are exact in bf16.  The FP8 model and the bf16 model are
    then the same function.  Returns the number of matrices changed."""
    n = 0
    with torch.no_grad():
        for _, p in model._decode_weight_params():
            wf = p.detach().float().cpu()
            amax = wf.abs().amax(dim=1).clamp_min(2.0 ** -20)
            s = torch.exp2(torch.ceil(torch.log2(amax / FP8_MAX)))[:, None]
            snapped = (wf / s).to(FP8).to(F32) * s
            snapped[:, 0], snapped[:, 1] = FP8_MAX * s[:, 0], -FP8_MAX * s[:, 0]
            assert torch.equal(snapped.to(BF16).float(), snapped)
            p.copy_(snapped.to(device=p.device, dtype=p.dtype))
            n += 1
    return n
