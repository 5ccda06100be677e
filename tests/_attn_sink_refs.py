"""fp64 references, case builders and budgets for attention sinks: ``attn_fwd`` / ``attn_decode`` with ``sinks``,
``attn_bwd`` on a sink-inclusive lse, and ``attn_sink_bwd`` (csrc/attn_sink.hip), by the method of
``_attention_refs.py`` (whose inputs, bound helpers, backward reference and backward budgets are used here).

Not collected by pytest.  ``test_attn_sink_refs.py`` (CPU) checks the references against independent PyTorch
double-precision paths, calibrates the budgets below and shows that the checks catch a kernel that ignores or
misplaces the sink; ``test_attn_sinks_gpu.py`` runs the HIP kernels on the same cases against the same bounds.

Semantics.  ``sinks`` is bf16 [H], one logit per QUERY head.  Row i of head h has
Z_i = sum_visible exp(scale q_i.k_j) + exp(s_h), o_i = sum_j (exp(scale q_i.k_j) / Z_i) v_j, lse_i = log Z_i: the
sink is not multiplied by ``scale``, is visible whatever the mask, and has no value row.  The backward is the plain
one on the sink-inclusive lse (``_attention_refs.bwd_ref`` is a function of the lse it is handed) plus
dsinks[h] = -sum_{b,i} exp(s_h - lse[b,h,i]) delta[b,h,i] with delta = rowsum(dO o).

The bound is that file's: |out - ref| <= ulps * (ulp_out(ref) + unit), with the units carried over (P normalised
by the sink-inclusive Z):

    o           2^-9 sum_j P_ij |V_jd|
    lse (fp32)  2^-23 (scale sum_d |q_id| |k_jd| at the row's largest score j  +  |lse|  +  |s_h|)
                (the sink enters as s_h log2(e), one fp32 product of magnitude |s_h|)
    decode o    2^-23 sum_j P_j |V_jd|
    dsinks      2^-23 sum_{b,i} p (|delta| (2.5 + 1.25 |s_h - lse|) + dmag),  p = exp(s_h - lse)

The dsinks unit, term by term for one row's summand a = p delta: the fp32 difference d = s_h - lse (2^-24 |d|) times
the fp32 constant log2(e) (itself rounded: 2^-25; the product: 2^-24) shifts the exponent by 2.5 x 2^-24 |d|, i.e.
p by 1.25 x 2^-23 |d| relative; v_exp_f32 about one fp32 ulp (2^-23); the product with delta 2^-24; the fp32 sum over
the B T rows 2^-23 of the magnitudes summed (the convention of ``_streaming_refs.colsum_ref``): together
2^-23 |a| (2.5 + 1.25 |d|).  dmag is the error of delta itself where the kernels' pre-pass formed it, an fp32 sum
of the magnitudes sum_d |dO_id o_id| (0 where delta is an input of the op).

Budgets.  ``measured`` is the smallest integer budget at which a plain PyTorch CPU model of the op (``*_model``
below: exactly the roundings listed above and in ``_attention_refs.py``, nothing else) passes on all of that op's
cases; ``budget`` is twice that.  Filled from ``pytest tests/test_attn_sink_refs.py`` (which fails when a row is
stale); nothing here was tuned against kernel output.  dq / dk / dv run under the ``attn_dq`` / ``attn_dk`` /
``attn_dv`` budgets of ``_attention_refs.py`` unchanged.

    op             measured  budget   outputs
    -------------  --------  ------   ------------------------------------------------
    sink_o                2       4   attn_fwd o (bf16) with sinks, plain and with kv_start
    sink_lse              1       2   attn_fwd lse (fp32) with sinks
    sink_decode_o         1       2   attn_decode o (bf16) with sinks
    sink_ds               1       2   attn_sink_bwd (bf16 fresh / fp32 slot), delta an input or from attn_bwd's pre-pass
"""
from __future__ import annotations

import functools
import math

import torch

import _attention_refs as A
from _streaming_refs import BF16, E32, F32, F64, _gen, assert_close_ulps, ulps_needed  # noqa: F401

BUDGET = {
    "sink_o": (2, 4),
    "sink_lse": (1, 2),
    "sink_decode_o": (1, 2),
    "sink_ds": (1, 2),
}
EB = A.EB
B, H = A.B, A.H
LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=F32))
EXTREME = (-math.inf, -30.0, 0.0, 30.0)
DEFECTS_FWD = ("dropped", "scaled", "kvhead")
DEFECTS_DS = ("dropped", "scaled", "kvhead", "sign")
DEFECTS_DECODE = ("dropped", "scaled", "kvhead", "per_split")


def check(op, out, ref_unit, what):
    ref, unit = ref_unit
    u = (BUDGET.get(op) or A.BUDGET[op])[1]
    assert_close_ulps(out, ref, u, u * torch.as_tensor(unit, dtype=F64), what=f"{op}/{what}")


def check_all(items):
    for op, name, out, ref_unit in items:
        check(op, out, ref_unit, name)


def fails(op, out, ref_unit):
    try:
        check(op, out, ref_unit, "defect")
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ masks
def window_start(T, W):
    """kv_start [T] of a sliding window of W keys, the query included."""
    return (torch.arange(T) - (W - 1)).clamp_min(0)


def visible(T, S, causal, window=None):
    vis = A.visible(T, S, causal)
    if window is not None:  # (causal, S == T)
        vis = vis & (torch.arange(S)[None, :] >= window_start(T, window)[:, None])
    return vis


# ------------------------------------------------------------------------------------------------ references
def fwd_ref(q, k, v, causal, scale, sinks, window=None):
    """o, lse as (ref, unit), the key probabilities p [B, H, T, S] and the sink's p_sink [B, H, T], in fp64 from the
    bf16 inputs.  A sink of -inf is plain attention; a row without keys has o = 0, lse = s_h."""
    T, Hq, S, Hkv = q.shape[1], q.shape[2], k.shape[1], k.shape[2]
    hmap = A.head_map(Hq, Hkv)
    qd, kd, vd = A._bh(q), A._kvh(k, hmap), A._kvh(v, hmap)
    sk = sinks.detach().cpu().to(F64).view(1, Hq, 1, 1)
    s = (scale * (qd @ kd.transpose(-1, -2))).masked_fill(~visible(T, S, causal, window), -math.inf)
    smax = s.max(-1, keepdim=True).values if S else torch.full((q.shape[0], Hq, T, 1), -math.inf, dtype=F64)
    m = torch.maximum(smax, sk)
    e = torch.exp(s - m)
    es = torch.exp(sk - m).expand_as(m)
    l = e.sum(-1, keepdim=True) + es
    p = e / l
    lse = (m + l.log())[..., 0]
    amag = scale * (qd.abs() @ kd.abs().transpose(-1, -2))
    top = amag.gather(-1, s.argmax(-1, keepdim=True))[..., 0] if S else torch.zeros_like(lse)
    sabs = torch.where(torch.isinf(sk), torch.zeros_like(sk), sk.abs())[..., 0]  # (an infinite sink: no product)
    unit_lse = E32 * (top + lse.abs() + sabs)
    return dict(o=((p @ vd).permute(0, 2, 1, 3), (EB * (p @ vd.abs())).permute(0, 2, 1, 3)),
                lse=(lse, unit_lse), p=p, p_sink=(es / l)[..., 0])


def dsinks_ref(lse, delta, sinks, dmag=None):
    """(ref, unit) [H] of ds[h] = -sum_{b,i} exp(s_h - lse[b,h,i]) delta[b,h,i] from the fp32 lse / delta [B, H, T]
    the op is handed (``dmag``: see the module docstring)."""
    l, dl = lse.detach().cpu().to(F64), delta.detach().cpu().to(F64)
    sk = sinks.detach().cpu().to(F64).view(1, -1, 1)
    d = sk - l
    p = torch.exp(d)
    dabs = torch.where(torch.isinf(d), torch.zeros_like(d), d.abs())
    mag = p * (dl.abs() * (2.5 + 1.25 * dabs) + (0.0 if dmag is None else dmag.detach().cpu().to(F64)))
    return -(p * dl).sum((0, 2)), E32 * mag.sum((0, 2))


def decode_keys(n, window):
    return (max(0, n - window) if window else 0), n


def decode_ref(q, k, v, scale, counts, sinks, window=0):
    """One query per sequence over keys [max(0, count - window), count) plus the sink; a count of 0 gives zeros."""
    Bb, _, Hq, D = q.shape
    o = torch.zeros(Bb, 1, Hq, D, dtype=F64)
    unit = torch.zeros_like(o)
    for b, n in enumerate(counts):
        j0, j1 = decode_keys(n, window)
        if j1 > j0:
            r = fwd_ref(q[b:b + 1], k[b:b + 1, j0:j1], v[b:b + 1, j0:j1], False, scale, sinks)["o"]
            o[b], unit[b] = r[0][0], r[1][0] * (E32 / EB)
    return o, unit


# ------------------------------------------------------------------------------------------------ fp32 / bf16 models
def _sink32(sinks, hmap, scale, defect):
    """The sink as the (possibly defective) kernel uses it: fp32 [1, H, 1, 1]."""
    s = sinks.detach().cpu().to(F32)
    if defect == "dropped":
        s = torch.full_like(s, -math.inf)
    elif defect == "scaled":
        s = s * torch.tensor(scale, dtype=F32)
    elif defect == "kvhead":
        s = s[hmap]
    return s.view(1, -1, 1, 1)


def fwd_model(q, k, v, causal, scale, sinks, window=None, defect=None, p_bf16=True, copies=1):
    """The forward with the documented roundings (``_attention_refs.fwd_model``) and the sink folded into the row
    maximum and the row sum in fp32.  ``defect``: see DEFECTS_FWD; ``copies``: the sink added that many times."""
    T, Hq, S, Hkv = q.shape[1], q.shape[2], k.shape[1], k.shape[2]
    hmap = A.head_map(Hq, Hkv)
    sk = _sink32(sinks, hmap, scale, defect)
    s = A._scores32(q, k, hmap, scale).masked_fill(~visible(T, S, causal, window), -math.inf)
    m = torch.maximum(s.max(-1, keepdim=True).values, sk)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True) + copies * torch.exp(sk - m)
    pv = (p.to(BF16).to(F32) if p_bf16 else p) @ A._kvh(v, hmap, F32)
    return dict(o=(pv / l).permute(0, 2, 1, 3).to(BF16), lse=(m + l.log())[..., 0])


def dsinks_model(lse, delta, sinks, out_dtype=BF16, defect=None, scale=1.0, hmap=None):
    """attn_sink_bwd in plain fp32: p = exp2((s - lse) log2 e), p delta, an fp32 sum, one output rounding."""
    Hq = sinks.numel()
    sk = _sink32(sinks, torch.arange(Hq) if hmap is None else hmap, scale, defect).view(1, Hq, 1)
    p = torch.exp2((sk - lse.to(F32)) * torch.tensor(LOG2E32, dtype=F32))
    ds = -(p * delta.to(F32)).sum((0, 2))
    return (-ds if defect == "sign" else ds).to(out_dtype)


def decode_model(q, k, v, scale, counts, sinks, window=0, defect=None):
    o = torch.zeros(q.shape, dtype=BF16)
    Bb, Hkv = q.shape[0], k.shape[2]
    span = min(window, k.shape[1]) if window and window < k.shape[1] else k.shape[1]
    copies = A.decode_splits(Bb, Hkv, span) if defect == "per_split" else 1
    for b, n in enumerate(counts):
        j0, j1 = decode_keys(n, window)
        if j1 > j0:
            o[b] = fwd_model(q[b:b + 1], k[b:b + 1, j0:j1], v[b:b + 1, j0:j1], False, scale, sinks, defect=defect,
                             p_bf16=False, copies=copies)["o"][0]
    return o


# ------------------------------------------------------------------------------------------------ inputs and cases
FAMILIES = ("randn", "extreme")


def draw_sinks(family, lse_plain, *key):
    """bf16 [H], distinct per head.  randn: each head's sink sits near the median of that head's sink-free lse, so
    the sink takes a real share of most rows (the CPU file asserts a probability in [0.05, 0.95] on at least half the
    rows); extreme: -inf, -30, 0, +30 cycling over the heads."""
    Hq = lse_plain.shape[1]
    if family == "extreme":
        return torch.tensor([EXTREME[h % 4] for h in range(Hq)], dtype=F32).to(BF16)
    g = _gen(21, *key)
    med = lse_plain.permute(1, 0, 2).reshape(Hq, -1).median(-1).values
    s = med + torch.linspace(-0.6, 0.6, Hq, dtype=F64) + 0.2 * torch.randn(Hq, generator=g, dtype=F64)
    return s.to(F32).to(BF16)


# (T, S): causal, queries aligned to the end of the keys
FWD_GEOMS = ((1, 1), (31, 31), (33, 33), (1, 65), (129, 129), (257, 257), (40, 600), (300, 340))
WINDOW_GEOMS = ((200, 17), (257, 64))  # (T, W): the SEG forward
BWD_GEOMS = ((33, 33), (200, 200), (257, 257), (513, 513))


def _spread(geoms, families):
    """(family, T, S, D, Hkv): (H, Hkv) rotating over (4, 4), (4, 2), (4, 1) along the cases."""
    return [(fam, T, S, D, (4, 2, 1)[(gi + di) % 3]) for fam in families for gi, (T, S) in enumerate(geoms)
            for di, D in enumerate((32, 64, 128))]


def fwd_cases():
    return _spread(FWD_GEOMS, FAMILIES)


def window_cases():
    """(family, T, W, D, Hkv)."""
    return _spread(WINDOW_GEOMS, FAMILIES)


def bwd_cases():
    return _spread(BWD_GEOMS, FAMILIES)


def _inputs(fam, T, S, D, Hkv, window=None):
    inp = dict(A.attn_inputs("randn", T, S, 1, D, Hkv))
    plain = A.fwd_ref(inp["q"], inp["k"], inp["v"], True, inp["scale"])["lse"][0] if window is None else \
        fwd_ref(inp["q"], inp["k"], inp["v"], True, inp["scale"], torch.full((H,), -math.inf), window)["lse"][0]
    inp["sinks"] = draw_sinks(fam, plain, T, S, D, Hkv, window or 0)
    inp["window"] = window
    return inp


@functools.lru_cache(maxsize=None)
def fwd_case(case, windowed=False):
    """(inputs, reference) of a forward case (``windowed``: the case's third entry is the window, S = T); computed
    once and shared: treat both as read-only."""
    fam, T, S, D, Hkv = case
    inp = _inputs(fam, T, T if windowed else S, D, Hkv, S if windowed else None)
    if windowed:
        inp["kv_start"] = window_start(T, S).to(torch.int32).expand(B, T).contiguous()
    return inp, fwd_ref(inp["q"], inp["k"], inp["v"], True, inp["scale"], inp["sinks"], inp["window"])


def fwd_checks(case, out, windowed=False):
    _, ref = fwd_case(case, windowed)
    return [("sink_o", "o", out["o"], ref["o"]), ("sink_lse", "lse", out["lse"], ref["lse"])]


@functools.lru_cache(maxsize=None)
def bwd_case(case):
    """(inputs, reference): the forward inputs plus ``o`` (the sink forward reference rounded to bf16), ``lse``
    (sink-inclusive, rounded to fp32) and ``delta`` = rowsum(dO o) rounded to fp32 (the ready delta of the second
    run); the reference holds dq / dk / dv (``_attention_refs.bwd_ref`` on that lse) and ``ds``."""
    fam, T, S, D, Hkv = case
    inp, fw = fwd_case(case)
    inp = dict(inp)
    inp.update(o=fw["o"][0].to(F32).to(BF16), lse=fw["lse"][0].to(F32))
    prod = A._bh(inp["do"]) * A._bh(inp["o"])
    inp["delta"] = prod.sum(-1).to(F32)
    ref = A.bwd_ref(inp["do"], inp["q"], inp["k"], inp["v"], inp["o"], inp["lse"], True, inp["scale"])
    # delta as the kernels' pre-pass forms it: the fp64 row sum is the reference, its fp32 summation error in the unit
    ref["ds"] = dsinks_ref(inp["lse"], prod.sum(-1), inp["sinks"], dmag=prod.abs().sum(-1))
    return inp, ref


def bwd_checks(case, out):
    _, ref = bwd_case(case)
    return [("attn_dq", "dq", out["dq"], ref["dq"]), ("attn_dk", "dk", out["dk"], ref["dk"]),
            ("attn_dv", "dv", out["dv"], ref["dv"])]


# attn_sink_bwd on its own: (B, H, T, family).  32 workgroups of 256 threads per head, one 16-byte group of four
# rows per thread and pass: (3, 2, 40003) is 3 x 10002 groups per head, 3.7 ragged passes of every workgroup, and
# with T odd the rows start at every misalignment
DS_CASES = ((2, 4, 1, "randn"), (2, 4, 257, "randn"), (2, 4, 257, "extreme"), (1, 3, 1000, "randn"),
            (3, 2, 40003, "randn"))


@functools.lru_cache(maxsize=None)
def ds_case(case):
    Bb, Hq, T, fam = case
    g = _gen(22, Bb, Hq, T, FAMILIES.index(fam))
    lse = (3.0 + 1.5 * torch.randn(Bb, Hq, T, generator=g)).to(F32)
    delta = torch.randn(Bb, Hq, T, generator=g).to(F32)
    sinks = draw_sinks(fam, lse.to(F64), Bb, Hq, T)
    inp = dict(lse=lse, delta=delta, sinks=sinks)
    return inp, dsinks_ref(lse, delta, sinks)


# ------------------------------------------------------------------------------------------------ decode
DECODE_HEADS, DECODE_S = A.DECODE_HEADS, A.DECODE_S
DECODE_WINDOW = 64


def decode_cases():
    """(D, H, Hkv, B, S buffer rows, counts, window, family); counts as in ``_attention_refs.decode_cases`` (None:
    the host shape; an int: a device scalar; a tuple: one count per sequence).  Split counts at B = 2: 1 up to
    S = 64, 2 at 65, 5 at 257, 16 at 1000; with the window of 64 the split count is 1 whatever S (the splits cover
    the window), so the windowed cases take the in-kernel fold and the others with S > 64 the combine kernel."""
    out = [(D, Hq, Hkv, 2, S, None, 0, "randn") for S in DECODE_S for (D, Hq, Hkv) in DECODE_HEADS]
    out += [(D, Hq, Hkv, 2, 1000, None, 0, "extreme") for (D, Hq, Hkv) in DECODE_HEADS]
    out += [(D, Hq, Hkv, 2, 1000, n, 0, "randn") for (D, Hq, Hkv), n in zip(DECODE_HEADS, (1, 63, 257, 700))]
    out += [(D, Hq, Hkv, 5, 1000, (0, 1, 1000, 65, 300), 0, "randn") for (D, Hq, Hkv) in DECODE_HEADS]
    W = DECODE_WINDOW
    out += [(D, Hq, Hkv, 2, S, None, W, "randn") for S in (63, 65, 1000) for (D, Hq, Hkv) in DECODE_HEADS]
    out += [(D, Hq, Hkv, 2, 1000, n, W, "randn") for (D, Hq, Hkv), n in zip(DECODE_HEADS, (1, 64, 257, 700))]
    out += [(D, Hq, Hkv, 5, 1000, (0, 1, 1000, 65, 300), W, fam) for (D, Hq, Hkv) in DECODE_HEADS for fam in FAMILIES]
    out += [(64, 8, 4, 2, 300, (0, 0), 0, "randn")]
    return out


def decode_splits(case):
    D, Hq, Hkv, Bb, S, counts, W, fam = case
    return A.decode_splits(Bb, Hkv, W if W and W < S else S)


@functools.lru_cache(maxsize=None)
def decode_case(case):
    D, Hq, Hkv, Bb, S, counts, W, fam = case
    base, _ = A.decode_case((D, Hq, Hkv, Bb, S, counts))
    inp = dict(base)
    # the sink-free lse of every sequence with keys, for the draw
    rows = []
    for b, n in enumerate(inp["counts"]):
        j0, j1 = decode_keys(n, W)
        if j1 > j0:
            rows.append(A.fwd_ref(inp["q"][b:b + 1], inp["k"][b:b + 1, j0:j1], inp["v"][b:b + 1, j0:j1], False,
                                  inp["scale"])["lse"][0])
    plain = torch.cat(rows, 0) if rows else torch.zeros(1, Hq, 1, dtype=F64)
    inp["sinks"] = draw_sinks(fam, plain, D, Hq, Hkv, Bb, S, W)
    inp["window"] = W
    return inp, decode_ref(inp["q"], inp["k"], inp["v"], inp["scale"], inp["counts"], inp["sinks"], W)
