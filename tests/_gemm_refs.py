"""fp64 references, case builders and the per-element bound for the GEMM family: ``gemm_tn`` (csrc/gemm_pp.hip and
its fallback csrc/gemm.hip), ``wgrad`` (csrc/gemm_wgrad.hip, csrc/wgrad_pp.hip, hybrid form included) and the
decode ``gemv`` (csrc/gemv.hip).

Not collected by pytest.  ``test_gemm_refs.py`` (CPU) checks the references against independent double-precision
paths, calibrates the budgets below and shows which defects the bound rejects; ``test_gemm_edges_gpu.py`` runs
the HIP kernels on the same cases against the same bounds.  The bound, ``assert_close_ulps``, ``ulps_needed`` and
``_gen`` are those of ``_streaming_refs``, ``check_all`` is its ``check_all`` over both budget tables:

    |out - ref| <= budget * (ulp_out(ref) + unit)

with ``unit`` = fp32's 2^-23 times the magnitudes of the terms that the kernel sums in fp32 (a sum of mixed signs
cancels), taken from the roundings that the kernel headers document, never from kernel output:

    C of epilogue 0 (+ bias), pre of epilogue 1,     ref = sum_k a b (+ bias), unit = 2^-23 (sum_k |a||b| + |bias|)
      [gate | up] of epilogue 7 (bf16)
    fused activations                                from the kernel's OWN bf16 pre-activation / data gradient under
                                                     the streaming budgets: epilogue 1 act = gelu(pre) (gelu_fwd),
                                                     2 y == relu(epilogue-0 + bias output) bitwise, 7 a = silu(g) u
                                                     (swiglu_fwd); 3 / 4 / 5 = act'(aux) d with d the kernel's own
                                                     epilogue-0 output of the same operands and config (gelu_bwd,
                                                     exact, swiglu_bwd)
    epilogue 6 delta (fp32)                          sum_d dO O per 64-wide head of the kernel's dO,
                                                     unit = 2^-23 sum_d |dO O|
    bias_acc of epilogues 3 / 4 (fp32 / bf16)        acc0 + column sums of the kernel's own bf16 out,
                                                     unit = 2^-23 (|acc0| + sum_rows |out|), budget ``colsum``
    wgrad fresh (bf16) / into fp32 / into bf16       (acc0 +) sum_m dy x, unit = 2^-23 (|acc0| + sum_m |dy||x|)
    wgrad fused bias gradient                        b0 + sum_m dy, unit = 2^-23 (|b0| + sum_m |dy|)
    gemv                                             as C; with the norm prologue the normalised input n is rounded
                                                     to bf16 before the product (gemv.hip header), and its statistics
                                                     are one fp32 pass, var = E[s^2] - E[s]^2: the unit gains
                                                     sum_k |w_k| (2^-9 |n_k| + unit_n_k), unit_n as ``gemv_norm_ref``

The epilogue 3 / 4 / 5 checks rest on the main loop being the same for every epilogue, i.e. on
``d == epilogue-0 output`` bitwise.  It holds on every arm the GPU file runs: epilogue 4 is checked with budget 0
(``out == d (aux > 0)`` bitwise wherever aux > 0), epilogue 6 by ``torch.equal(dO, epilogue-0 output)``, and
epilogues 3 / 5 pass under the streaming budgets of the unfused kernels with no allowance for a different d.

Data families (seeded by ``_gen``): ``randn`` -- A randn, B randn / sqrt(K), bias 0.5 randn; ``exact`` -- integer
operands, |a| <= 51 and |b| <= 4, so every fp32 partial sum in any order is an integer below 2^24 and exact (no
sparsity is needed for that at K <= 2112: K * 51 * 4 < 2^19): the reference is then the exact sum rounded ONCE to
nearest-even and budget 0 applies to C, which pins the rounding mode; rows 0 and M - 1 carry sums planted exactly
on bf16 ties (+-257, +-259: between 256 / 258 and 258 / 260).  Epilogue aux comes from randn, and on one shape
from the ``grid`` magnitude family of ``_streaming_refs``.

Budgets.  ``measured`` is the smallest integer budget at which a CPU fp32 model of the op passes on all of its
cases, the model being the larger of ``torch.float32`` matmul and an fp32 accumulation in the kernel's order
(sequential over 32-deep chunks -- which is also sequential over 64-deep tiles --, split-K slices and hybrid pieces
summed in slice order; gemv: per-thread chains over the thread's chunks, lanes, then waves in order), rounded to
the output type; ``budget`` is twice that (a different summation order inside the MFMA / the shuffles).  Filled
from ``pytest tests/test_gemm_refs.py``, which fails when a row is stale; nothing was tuned against kernel output.

    op            measured  budget   outputs
    ------------  --------  ------   ------------------------------------------------------------
    gemm_c               1       2   C of epi 0 (+ bias), pre of epi 1, [gate | up] of epi 7 (bf16)
    gemm_delta           1       2   epi 6 delta (fp32)
    wgrad_bf16           1       2   wgrad fresh / accumulated into bf16
    wgrad_f32            1       2   wgrad accumulated into fp32
    wgrad_bias           1       2   wgrad fused bias gradient (fp32 / bf16)
    gemv_y               1       2   gemv y (bf16), no norm prologue
    gemv_norm_y          2       4   gemv y (bf16) with the LayerNorm / RMSNorm prologue
    (colsum, gelu_fwd, gelu_bwd, swiglu_fwd, swiglu_bwd, exact: the rows of ``_streaming_refs``)
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

import _streaming_refs as S
from _streaming_refs import BF16, E32, F32, F64, _gen

# op -> (measured, budget); see the table above
BUDGET = {
    "gemm_c": (1, 2),
    "gemm_delta": (1, 2),
    "wgrad_bf16": (1, 2),
    "wgrad_f32": (1, 2),
    "wgrad_bias": (1, 2),
    "gemv_y": (1, 2),
    "gemv_norm_y": (2, 4),
}


def budget(op):
    """(measured, budget) of an op of this file's table or of ``_streaming_refs``'s."""
    return BUDGET[op] if op in BUDGET else S.BUDGET[op]


def check_all(items):
    """``_streaming_refs.check_all`` over both budget tables: (op, name, out, (ref64, unit)[, fmt]) tuples."""
    for it in items:
        (ref, unit), u = it[3], budget(it[0])[1]
        S.assert_close_ulps(it[2], ref, u, u * torch.as_tensor(unit, dtype=F64), f"{it[0]}/{it[1]}", *(it[4:5]))


def bf16_rne(v64):
    """fp64 values that fp32 holds exactly, rounded once to bf16 (nearest-even), as fp64."""
    return v64.to(F32).to(BF16).to(F64)


def bf16_trunc(v32):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero): the defect, not the kernel."""
    return (v32.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)


def rel_norm(a, b):
    """The criterion of the older tests: ||a - b|| / ||b|| (they assert < 5e-3)."""
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def mm64(a, b):
    """(a b^T, |a| |b|^T) in fp64 for a [M, K], b [N, K]."""
    ad, bd = a.to(F64), b.to(F64)
    return ad @ bd.t(), ad.abs() @ bd.abs().t()


def mm32_chunked(a, b, chunk=32):
    """fp32 a b^T accumulated sequentially over ``chunk``-deep pieces of K (the kernels' MFMA chain)."""
    af, bf = a.float(), b.float()
    acc = torch.zeros(af.shape[0], bf.shape[0])
    for k0 in range(0, af.shape[1], chunk):
        acc = acc + af[:, k0:k0 + chunk] @ bf[:, k0:k0 + chunk].t()
    return acc


# ------------------------------------------------------------------------------------------------ gemm_tn
# (M, N, K): what each reaches is listed in test_gemm_edges_gpu.py
GEMM_SHAPES = ((1, 8, 128), (17, 72, 128), (129, 264, 192), (257, 520, 128), (300, 264, 64), (257, 264, 2048),
               (520, 776, 2112), (520, 776, 192))
GEMM_TILED = ((520, 776, 2112), (520, 776, 192))  # 3 x 4 ragged tiles
GEMM_GRID_AUX = (129, 264, 192)                   # the shape whose aux is the magnitude grid
SWIGLU_F136 = (257, 136, 128)                     # epilogue 7 only: a 128-column tile plus 8
# epilogue 6 (B, T, N, K): T = 112 puts batch boundaries inside a tile; T = 200 (T % 16 != 0) is the fallback arm;
# (5, 112, 832, 2048): 3 x 4 ragged tiles with quadrant epilogues
DELTA_CASES = ((3, 112, 320, 128), (3, 112, 320, 2048), (2, 200, 320, 128), (5, 112, 832, 2048), (5, 112, 832, 192))


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K, data="randn", aux="randn"):
    """a [M, K], b [N, K], b7 [2N, K] (epilogue 7's [gate | up] rows), bias [N]; aux [M, N] (epilogues 3 / 4: the
    pre-activation; 4 takes relu(aux)), gu [M, 2N] (epilogue 5), fill [N] (bias_acc's start)."""
    g = _gen(11, M, N, K, data == "exact", aux == "grid")
    if data == "exact":
        ri = lambda *s, lo, hi: torch.randint(lo, hi + 1, s, generator=g).to(F32)  # noqa: E731
        # a = i + 16 j with |i|, |j| <= 3: sums of ~12 significant bits, so nearly every output is rounded
        a = ri(M, K, lo=-3, hi=3) + 16 * ri(M, K, lo=-3, hi=3)
        b, b7 = ri(N, K, lo=-4, hi=4), ri(2 * N, K, lo=-4, hi=4)
        bias = ri(N, lo=-4, hi=4)
        for r in {0, M - 1}:  # ties: row r = [4 x 16, 1, 1, ...], columns [+-4 x 16, t, 0, ...] -> +-256 + t
            a[r, :16], a[r, 16:] = 4.0, 1.0
            for j, (sg, t) in zip((0, 1, 2, 3, N - 4, N - 3, N - 2, N - 1), ((1, 1), (1, 3), (-1, -1), (-1, -3)) * 2):
                for w_ in (b, b7):
                    w_[j] = 0.0
                    w_[j, :16], w_[j, 16] = 4.0 * sg, float(t)
                bias[j] = 0.0
    else:
        a = torch.randn(M, K, generator=g)
        b = torch.randn(N, K, generator=g) / K ** 0.5
        b7 = torch.randn(2 * N, K, generator=g) / K ** 0.5
        bias = 0.5 * torch.randn(N, generator=g)
    if aux == "grid":
        ax = S.mag_grid(M * N, shift=3).reshape(M, N)
        gate, up = S.mag_grid(M * N).reshape(M, N), S.mag_grid(M * N, shift=7).reshape(M, N)
        gu = torch.cat([gate, torch.where(up == 0, torch.ones_like(up), up)], -1)
    else:
        ax = (2 * torch.randn(M, N, generator=g)).to(BF16)
        gu = torch.cat([2 * torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)], -1).to(BF16)
    fill = 1.5 + 0.01 * torch.arange(N, dtype=F32)
    return dict(a=a.to(BF16), b=b.to(BF16), b7=b7.to(BF16), bias=bias.to(BF16), aux=ax, gu=gu.contiguous(),
                fill=fill, data=data)


@functools.lru_cache(maxsize=None)
def gemm_refs(M, N, K, data="randn", aux="randn"):
    """(ref, unit) of a b^T, a b^T + bias and a b7^T."""
    inp = gemm_inputs(M, N, K, data, aux)
    c, ca = mm64(inp["a"], inp["b"])
    c7, c7a = mm64(inp["a"], inp["b7"])
    bd = inp["bias"].to(F64)
    if data == "exact":  # exact sums, rounded once; budget 0
        return dict(c=(bf16_rne(c), 0.0), cb=(bf16_rne(c + bd), 0.0), c7=(bf16_rne(c7), 0.0))
    return dict(c=(c, E32 * ca), cb=(c + bd, E32 * (ca + bd.abs())), c7=(c7, E32 * c7a))


def colsum_acc_ref(out, acc0):
    """acc0 + the fp64 column sums of ``out``; unit 2^-23 (|acc0| + sum_rows |out|)."""
    od, fd = out.detach().cpu().to(F64), acc0.detach().cpu().to(F64)
    return fd + od.sum(0), E32 * (fd.abs() + od.abs().sum(0))


def gemm_checks(inp, refs, out):
    """``out`` (the kernel's, or the model's): c0, c0b (epi 0 without / with bias), act1, pre1, y2, o3, o4, o5 and
    b3_f32, b3_bf16, b4_f32, b4_bf16 (bias_acc after the call, started from inp['fill']), a7, gu7.  Missing keys
    are skipped."""
    cop = "exact" if inp["data"] == "exact" else "gemm_c"
    has = lambda *k: all(x in out for x in k)  # noqa: E731
    items = []
    for key, r in (("c0", "c"), ("c0b", "cb"), ("pre1", "cb"), ("gu7", "c7")):
        if has(key):
            items.append((cop, key, out[key], refs[r]))
    if has("act1", "pre1"):
        items.append(("gelu_fwd", "act1", out["act1"], S.gelu_ref(out["pre1"].cpu())))
    if has("y2", "c0b"):
        items.append(("exact", "y2", out["y2"], (S.relu_of(out["c0b"].cpu()).to(F64), 0.0)))
    if has("a7", "gu7"):
        items.append(("swiglu_fwd", "a7", out["a7"], S.swiglu_ref(out["gu7"].cpu())))
    if has("o3"):
        items.append(("gelu_bwd", "o3", out["o3"], S.gelu_bwd_ref(out["c0"].cpu(), inp["aux"])))
    if has("o4"):
        items.append(("exact", "o4", out["o4"], S.relu_bwd_ref(out["c0"].cpu(), S.relu_of(inp["aux"]))))
    if has("o5"):
        items.append(("swiglu_bwd", "o5", out["o5"], S.swiglu_bwd_ref(out["c0"].cpu(), inp["gu"])))
    for e in (3, 4):
        for nm, dt in (("f32", F32), ("bf16", BF16)):
            if has(f"b{e}_{nm}"):
                items.append(("colsum", f"b{e}_{nm}", out[f"b{e}_{nm}"],
                              colsum_acc_ref(out[f"o{e}"], inp["fill"].to(dt))))
    return items


def colsum_groups_f32(out, acc0, group_rows=64):
    """The kernels' column sums: fp32 sums per row group, then the groups in order on top of acc0."""
    o = out.float()
    v = acc0.float().clone()
    tot = torch.zeros_like(v)
    for r0 in range(0, o.shape[0], group_rows):
        tot = tot + o[r0:r0 + group_rows].sum(0)
    return (v + tot).to(acc0.dtype)


def gemm_model_outputs(M, N, K, data="randn", aux="randn", chunked=False):
    """The fp32 CPU model of every gemm_tn output (``chunked``: in the kernel's K order)."""
    inp = gemm_inputs(M, N, K, data, aux)
    mm = mm32_chunked if chunked else (lambda a, b: a.float() @ b.float().t())
    c = mm(inp["a"], inp["b"])
    c0, c0b = c.to(BF16), (c + inp["bias"].float()).to(BF16)
    gu7 = mm(inp["a"], inp["b7"]).to(BF16)
    o3 = S.gelu_model_f32(inp["aux"], c0)["dx"]
    o4 = torch.where(inp["aux"] > 0, c0, torch.zeros_like(c0))
    out = dict(c0=c0, c0b=c0b, pre1=c0b, act1=F.gelu(c0b.float(), approximate="tanh").to(BF16),
               y2=S.relu_of(c0b), o3=o3, o4=o4, o5=S.swiglu_model_f32(inp["gu"], c0)["dgu"], gu7=gu7,
               a7=S.swiglu_model_f32(gu7, torch.ones(M, N).to(BF16))["y"])
    for e, o in ((3, o3), (4, o4)):
        for nm, dt in (("f32", F32), ("bf16", BF16)):
            out[f"b{e}_{nm}"] = colsum_groups_f32(o, inp["fill"].to(dt)) if chunked else \
                (inp["fill"].to(dt).float() + o.float().sum(0)).to(dt)
    return out


@functools.lru_cache(maxsize=None)
def delta_inputs(B, T, N, K):
    g = _gen(12, B, T, N, K)
    M = B * T
    return dict(a=(0.5 * torch.randn(M, K, generator=g)).to(BF16), b=(torch.randn(N, K, generator=g) / K ** 0.5).to(BF16),
                o=torch.randn(M, N, generator=g).to(BF16), data="randn")


def delta_ref(do, o, B, T):
    """delta[b, h, t] = sum_d dO O over the 64 columns of head h, from the given (the kernel's own) bf16 dO."""
    p = (do.detach().cpu().to(F64) * o.to(F64)).view(B, T, -1, 64)
    return p.sum(-1).permute(0, 2, 1), E32 * p.abs().sum(-1).permute(0, 2, 1)


def delta_checks(inp, B, T, out):
    """``out``: do6 (bf16 [M, N]) and delta6 (fp32 [B, N / 64, T])."""
    c, ca = mm64(inp["a"], inp["b"])
    return [("gemm_c", "do6", out["do6"], (c, E32 * ca)),
            ("gemm_delta", "delta6", out["delta6"], delta_ref(out["do6"], inp["o"], B, T))]


def delta_model_outputs(B, T, N, K, chunked=False):
    inp = delta_inputs(B, T, N, K)
    do = (mm32_chunked(inp["a"], inp["b"]) if chunked else inp["a"].float() @ inp["b"].float().t()).to(BF16)
    p = (do.float() * inp["o"].float()).view(B, T, -1, 64)
    if chunked:  # a lane's 8 columns in turn, then the 8 lanes of a head
        p8 = p.view(B, T, -1, 8, 8)
        s = torch.zeros(p8.shape[:-1])
        for e in range(8):
            s = s + p8[..., e]
        d = torch.zeros(s.shape[:-1])
        for l_ in range(8):
            d = d + s[..., l_]
    else:
        d = p.sum(-1)
    return dict(do6=do, delta6=d.permute(0, 2, 1).contiguous())


def expect_gemm_plan(M, N, K, epi, phased=4, T=0):
    """The arm a case was written for, as ``gemm_plan`` reports it (without the grid): ping-pong kernel at K >= 128
    (epilogue 6: and 16 | T), quadrant epilogues at K >= 2048 for epilogues 0, 2, 3, 4, 6; 4 (2) column-sum rows per
    tile row with (without) them.  -> ([pp, quad], [tile rows, tile columns, column-sum rows])"""
    pp = phased == 4 and K >= 128 and (epi != 6 or T % 16 == 0)
    quad = pp and K >= 2048 and epi in (0, 2, 3, 4, 6)
    tm, tn = -(-M // 256), -(-N // (128 if epi == 7 else 256))
    groups = (4 if phased == 4 and K >= 2048 else 2) * tm
    return [int(pp), int(quad)], [tm, tn, groups]


# ------------------------------------------------------------------------------------------------ wgrad
# name -> (M, P, Q, S, slice, grid8) and, for grid8 cases (persistent grid cut to 8 workgroups), the hybrid plan
# (full, rem, S, K-tiles per slice).  S / slice are what wgrad_plan's cost model gives today; the GPU tests assert
# them (and the kernel arm) through torch.ops.pllm.wgrad_plan, so a changed model fails there instead of moving a
# case onto another kernel.
WGRAD_CASES = {
    "m64": (64, 264, 136, 1, 64, False),            # one K-tile: the one-barrier kernel even for fp32 targets
    "m128": (128, 264, 136, 1, 128, False),         # two K-tiles: the ping-pong kernel's minimum
    "ragged1": (2048, 200, 136, 4, 512, False),     # ragged P and Q in a single tile
    "tiles2x3": (1024, 264, 520, 2, 512, False),    # 2 x 3 tiles with 8-row / 8-column remainders
    "short_last": (4672, 256, 256, 9, 576, False),  # 73 stages: 8 slices of 9 and a last one of a single stage
    "short_last2": (1216, 256, 264, 2, 640, False),  # 19 stages: slices of 10 and 9
    "hybrid": (1024, 520, 776, 2, 512, True),       # 12 tiles on 8 workgroups: 8 whole + 4 sliced, ragged edges
    "hybrid_rem0": (256, 776, 776, 1, 256, True),   # 16 tiles on 8 workgroups: two whole rounds, nothing sliced
}
WGRAD_HYBRID = {"hybrid": (8, 4, 2, 8), "hybrid_rem0": (16, 0, 0, 4)}


def wgrad_arm(name, mf, out_f32, bias):
    """0 / 1: the one-barrier kernel (16x16x32 / 32x32x16); 2: ping-pong (fp32 targets, >= 2 K-tiles per slice);
    3: hybrid (fp32 target, no bias, more tiles than workgroups)."""
    slice_rows, grid8 = WGRAD_CASES[name][4:]
    if mf:
        return 0 if mf == 16 else 1
    if not out_f32 or slice_rows < 128:
        return 0
    return 3 if grid8 and not bias else 2


def expect_wgrad_plan(name, mf, out_f32, bias):
    """What ``wgrad_plan`` reports for a WGRAD_CASES row under ``wgrad_set_mfma(mf)``."""
    arm = wgrad_arm(name, mf, out_f32, bias)
    return [arm, *WGRAD_CASES[name][3:5]] + (list(WGRAD_HYBRID[name]) if arm == 3 else [0, 0, 0, 0])


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name):
    M, P, Q = WGRAD_CASES[name][:3]
    g = _gen(13, M, P, Q)
    return dict(dy=(0.3 * torch.randn(M, P, generator=g)).to(BF16), x=torch.randn(M, Q, generator=g).to(BF16),
                acc0=torch.randn(P, Q, generator=g), b0=torch.randn(P, generator=g))


@functools.lru_cache(maxsize=None)
def wgrad_refs(name):
    inp = wgrad_inputs(name)
    w, wa = mm64(inp["dy"].t(), inp["x"].t())
    dyd = inp["dy"].to(F64)
    return dict(w=w, wa=wa, db=dyd.sum(0), dba=dyd.abs().sum(0))


def wgrad_checks(name, out):
    """``out``: fresh (bf16), acc_bf16 / acc_f32 (started from acc0 in that type), bias_f32 / bias_bf16 (from b0)."""
    inp, r = wgrad_inputs(name), wgrad_refs(name)
    items = []
    if "fresh" in out:
        items.append(("wgrad_bf16", "fresh", out["fresh"], (r["w"], E32 * r["wa"])))
    for nm, dt, op in (("acc_f32", F32, "wgrad_f32"), ("acc_bf16", BF16, "wgrad_bf16")):
        if nm in out:
            a0 = inp["acc0"].to(dt).to(F64)
            items.append((op, nm, out[nm], (a0 + r["w"], E32 * (a0.abs() + r["wa"]))))
    for nm, dt in (("bias_f32", F32), ("bias_bf16", BF16)):
        if nm in out:
            b0 = inp["b0"].to(dt).to(F64)
            items.append(("wgrad_bias", nm, out[nm], (b0 + r["db"], E32 * (b0.abs() + r["dba"]))))
    return items


def wgrad_pieces_f32(dy, x, slice_rows):
    """The fp32 split-K pieces: each slice of ``slice_rows`` tokens summed sequentially over 32-token chunks."""
    return [mm32_chunked(dy[m0:m0 + slice_rows].t(), x[m0:m0 + slice_rows].t())
            for m0 in range(0, dy.shape[0], slice_rows)]


def wgrad_model_outputs(name, order="torch"):
    """``order``: torch (fp32 matmul), plan (wgrad_plan's slices in slice order), whole (one sequential chain, the
    hybrid form's whole tiles), hybrid (the hybrid form's slices)."""
    inp = wgrad_inputs(name)
    M, P, Q, _, slice_rows, _ = WGRAD_CASES[name]
    dy, x = inp["dy"], inp["x"]
    if order == "torch":
        pieces = [dy.float().t() @ x.float()]
        bpieces = [dy.float().sum(0)]
    else:
        rows = {"plan": slice_rows, "whole": M, "hybrid": 64 * WGRAD_HYBRID.get(name, (0, 0, 0, M // 64))[3]}[order]
        pieces = wgrad_pieces_f32(dy, x, rows)
        bpieces = [mm32_chunked(dy[m0:m0 + rows].t(), torch.ones(1, min(rows, M - m0)))[:, 0] for m0 in range(0, M, rows)]

    def total(start, ps):  # the reduce kernels: the target (or zero), then the pieces in slice order
        v = start.float().clone()
        for p in ps:
            v = v + p
        return v

    zero = torch.zeros(P, Q)
    return dict(fresh=total(zero, pieces).to(BF16), acc_f32=total(inp["acc0"], pieces),
                acc_bf16=total(inp["acc0"].to(BF16), pieces).to(BF16), bias_f32=total(inp["b0"], bpieces),
                bias_bf16=total(inp["b0"].to(BF16), bpieces).to(BF16))


# ------------------------------------------------------------------------------------------------ gemv
GEMV_M = (1, 3, 5, 8)
# 1024 / 1032: C = 1 -> 2 columns per workgroup; 2048 / 2056: C = 2 -> 4; 8184 / 8192: split-K form -> wide form
# (one wave per 4 columns); 8197: the wide form with a ragged wave (1 of 4 columns) and workgroup
GEMV_N = (1024, 1032, 2048, 2056, 8184, 8192, 8197)
GEMV_K = (8, 520, 768)  # chunks of 8: 1 (one lane busy), 65 (128 threads, the second wave holds one chunk), 96
GEMV_EPS = 1e-5


def gemv_form(N, K, split_only=False):
    """(columns per workgroup, threads) of the launch gemv.hip picks: the wide form is (16, 256) -- for plain calls
    (no norm prologue, activation or KV append) at N >= 8192."""
    if N >= 8192 and not split_only:
        return 16, 256
    nch = K // 8
    return (1 if N <= 1024 else 2 if N <= 2048 else 4), (256 if nch > 128 else 128 if nch > 64 else 64)


@functools.lru_cache(maxsize=None)
def gemv_inputs(M, N, K, norm=0):
    """norm 0: none; 1 LayerNorm; 2 RMSNorm (x is then given a non-zero mean, and row 1 is all equal)."""
    g = _gen(14, M, N, K, norm)
    x = torch.randn(M, K, generator=g)
    res = torch.randn(M, K, generator=g).to(BF16)
    if norm:
        x = 2 * x + 0.5
        if M >= 3:
            x[1], res[1] = 2.0, 0.5
    return dict(x=x.to(BF16), res=res, w=(torch.randn(N, K, generator=g) / K ** 0.5).to(BF16),
                bias=torch.randn(N, generator=g).to(BF16), gamma=(1 + 0.1 * torch.randn(K, generator=g)).to(BF16),
                beta=(0.1 * torch.randn(K, generator=g)).to(BF16))


def gemv_ref(inp, bias=True):
    c, ca = mm64(inp["x"], inp["w"])
    bd = inp["bias"].to(F64) if bias else torch.zeros(1, dtype=F64)
    return c + bd, E32 * (ca + bd.abs())


def gemv_norm_ref(inp, rms, with_res, bias=True, eps=GEMV_EPS):
    """s = bf16(x + res); n = (s - mean) rstd gamma + beta (mean 0, no beta for RMS); y = sum_k n_k w_k + bias.

    The kernel rounds n to bf16 (2^-9 |n| each) and takes its statistics in one fp32 pass, var = E[s^2] - E[s]^2:
    the two terms cancel, so rstd carries 2^-23 E[s^2] / (2 (var + eps)) relative, and the mean's error 2^-23 mean|s|
    reaches n scaled by rstd |gamma|.  unit_n = 2^-23 (|x_hat gamma| (1 + E[s^2] / (var + eps)) + |beta| +
    rstd |gamma| mean|s|), and y's unit is 2^-23 (sum|n||w| + |bias|) + sum_k |w_k| (2^-9 |n_k| + unit_n_k)."""
    eps = S.f32r(eps)
    sx = inp["x"].to(F64) + (inp["res"].to(F64) if with_res else 0.0)
    s = sx.to(F32).to(BF16) if with_res else inp["x"]
    sq = s.to(F64)
    mean = torch.zeros(sq.shape[0], 1, dtype=F64) if rms else sq.mean(-1, keepdim=True)
    ms = (sq * sq).mean(-1, keepdim=True)
    var = ((sq - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    gd = inp["gamma"].to(F64)
    bt = torch.zeros_like(gd) if rms else inp["beta"].to(F64)
    xh = (sq - mean) * rstd
    n = xh * gd + bt
    unit_n = E32 * ((xh * gd).abs() * (1 + ms / (var + eps)) + bt.abs()
                    + (0.0 if rms else 1.0) * rstd * gd.abs() * sq.abs().mean(-1, keepdim=True))
    wd = inp["w"].to(F64)
    bd = inp["bias"].to(F64) if bias else torch.zeros(1, dtype=F64)
    unit = E32 * (n.abs() @ wd.abs().t() + bd.abs()) + (2.0 ** -9 * n.abs() + unit_n) @ wd.abs().t()
    return dict(s=(bf16_rne(sx) if with_res else sq, 0.0), y=(n @ wd.t() + bd, unit), n=n)


def gemv_chain_f32(xin, w, bias, cols_threads):
    """fp32 in gemv.hip's order: thread t chains the products of its chunks t, t + T, ... (8 elements each), the
    64 lanes of a wave are summed, then bias + the waves in order.  (Wide form: one wave per column, 64 lanes.)"""
    _, T = cols_threads
    T = 64 if cols_threads[0] == 16 else T
    M, K = xin.shape
    nch = K // 8
    xf, wf = xin.float().view(M, nch, 8), w.float().view(-1, nch, 8)
    out = torch.empty(M, w.shape[0])
    for n0 in range(0, w.shape[0], 512):
        wb = wf[n0:n0 + 512]
        acc = torch.zeros(M, wb.shape[0], T)
        for c0 in range(0, nch, T):
            nt = min(T, nch - c0)
            for e in range(8):
                acc[:, :, :nt] = acc[:, :, :nt] + xf[:, None, c0:c0 + nt, e] * wb[None, :, c0:c0 + nt, e]
        waves = acc.view(M, wb.shape[0], T // 64, 64).sum(-1)
        v = bias.float()[n0:n0 + 512].expand(M, -1).clone() if bias is not None else torch.zeros(M, wb.shape[0])
        for i in range(T // 64):
            v = v + waves[..., i]
        out[:, n0:n0 + 512] = v
    return out


def gemv_model_outputs(inp, N, K, norm=0, with_res=False, bias=True, chain=False):
    """fp32 CPU model: y (and s with a residual).  ``chain``: the kernel's order, and for the norm prologue its
    one-pass statistics."""
    b = inp["bias"] if bias else None
    if not norm:
        xin, s = inp["x"], None
    else:
        s = (inp["x"].float() + inp["res"].float()).to(BF16) if with_res else inp["x"]
        sf = s.float()
        if chain:
            mean = torch.zeros(sf.shape[0], 1) if norm == 2 else sf.mean(-1, keepdim=True)
            var = ((sf * sf).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
            xin = ((sf - mean) * torch.rsqrt(var + GEMV_EPS) * inp["gamma"].float()
                   + (0.0 if norm == 2 else inp["beta"].float())).to(BF16)
        elif norm == 2:
            xin = (sf * torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + GEMV_EPS) * inp["gamma"].float()).to(BF16)
        else:
            xin = F.layer_norm(sf, (K,), inp["gamma"].float(), inp["beta"].float(), GEMV_EPS).to(BF16)
    if chain:
        y = gemv_chain_f32(xin, inp["w"], b, gemv_form(N, K, split_only=bool(norm)))
    else:
        y = xin.float() @ inp["w"].float().t() + (b.float() if b is not None else 0.0)
    return dict(y=y.to(BF16), s=s if with_res else None)


def gemv_cases():
    """(M, N, K, bias) of the plain calls: every M x N x K, the bias alternating."""
    return [(M, N, K, (i + j + k) % 2 == 0) for i, M in enumerate(GEMV_M) for j, N in enumerate(GEMV_N)
            for k, K in enumerate(GEMV_K)]


def gemv_norm_cases():
    """(M, N, K, norm, with_res): the norm prologue at both sides of each split-K seam and over the wide form's
    threshold (the prologue keeps the split-K form there), K with a partly idle second wave and full."""
    return [(M, N, K, norm, wr) for (M, N, K) in ((1, 1024, 520), (3, 1032, 768), (5, 2056, 520), (8, 8197, 768),
                                                    (3, 2048, 8))
            for norm in (1, 2) for wr in (False, True)]
