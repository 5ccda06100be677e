"""fp64 references and case builders for the attention kernels' per-row key bounds (``attn_fwd(..., kv_start)``,
``attn_bwd(..., kv_start, q_last)``): document and window masks.

Not collected by pytest.  ``test_attention_seg_refs.py`` (CPU) checks the references against torch double-precision
autograd, re-measures the budgets of ``_attention_refs.BUDGET`` on these cases and shows that the checks catch
one key admitted before ``kv_start`` or one query past ``q_last``; ``test_attention_seg_gpu.py`` runs the HIP kernels
on the same cases under the same budgets.

Conventions, units and the bound are those of ``_attention_refs`` (see its docstring); the only difference is the mask:
S = T, and query i of batch row b sees key j iff kv_start[b, i] <= j <= i, equivalently j <= i <= q_last[b, j].  The
references take the mask as a [B, T, T] visibility tensor, so they know nothing of either bound form.

A case is (family, T, D, Hkv, pattern of batch row 0, pattern of batch row 1): the two rows of a batch carry different
patterns, so a kernel that read row 0's bounds for both fails.

Budgets.  o / lse / dq / dk / dv use ``_attention_refs.BUDGET`` unchanged: the CPU model of the op needs the same
measured budgets on these cases (2 / 1 / 2 / 2 / 2).  The rotated-back dq needs 2 on the bounded RoPE case where the
table's unbounded cases need 1 (rows of a 40-key window or a short document sum few terms, so the rotation's own fp32
rounding of the partner element is a larger share of the unit); by the table's rule (budget = twice the model's
need) the rotated outputs are judged here with ``ROT_BUDGET``.  Nothing was tuned against kernel output."""
from __future__ import annotations

import functools
import math

import torch

import _attention_refs as A
from _attention_refs import B, BF16, E32, EB, F32, F64, H, KEY_BLOCK  # noqa: F401

DOC_STARTS = (1, 31, 32, 33, 64, 65, 127, 128, 200, 255, 256, 257, 300, 511, 512)
PATTERNS = ("docs", "window40", "single", "late", "halves", "one_doc")
# every pattern once, two per case
PAIRS = (("docs", "window40"), ("single", "late"), ("halves", "one_doc"))
GEOMS = (33, 200, 257, 513)
ROPE_T = 300
# op -> (measured on the CPU model, budget = 2 x measured) for the rotated-back gradients of the bounded RoPE case
ROT_BUDGET = {"attn_dq_rot": (2, 4), "attn_dk_rot": (2, 4)}


def budget(op):
    return ROT_BUDGET[op] if op in ROT_BUDGET else A.BUDGET[op]


def check_all(items):
    for op, name, out, (ref, unit) in items:
        u = budget(op)[1]
        A.assert_close_ulps(out, ref, u, u * torch.as_tensor(unit, dtype=F64), what=f"{op}/{name}")


# ------------------------------------------------------------------------------------------------ bounds
def kv_start_of(pattern, T):
    """int32 [T]: the first key of each query (non-decreasing, 0 <= kv_start[i] <= i)."""
    i = torch.arange(T)
    if pattern == "docs":        # boundaries on and beside every sub-block (32), key-tile (64) and key-block (256) edge
        starts = torch.tensor([0] + [s for s in DOC_STARTS if s < T])
        ks = starts[torch.searchsorted(starts, i, right=True) - 1]
    elif pattern == "window40":  # a sliding window of 40 keys: both limits inside most tiles, aligned to nothing
        ks = (i - 39).clamp_min(0)
    elif pattern == "single":    # every row sees one key
        ks = i
    elif pattern == "late":      # one document starting at T - 1
        ks = torch.where(i >= T - 1, T - 1, 0)
    elif pattern == "halves":    # one boundary at 256 (T <= 256: one document)
        ks = torch.where(i >= 256, 256, 0)
    elif pattern == "one_doc":
        ks = torch.zeros(T, dtype=torch.long)
    else:
        raise ValueError(pattern)
    return ks.to(torch.int32)


def q_last_of(kv_start):
    """int32 [T]: the last query that sees key j = the last i with kv_start[i] <= j (written as a plain loop, apart
    from ``ops.bounds_from_start``)."""
    ks = kv_start.tolist()
    T = len(ks)
    out, i = [], 0
    for j in range(T):
        while i + 1 < T and ks[i + 1] <= j:
            i += 1
        out.append(i)
    return torch.tensor(out, dtype=torch.int32)


def vis_from_start(kv_start):
    """[T, T] bool (query i, key j): kv_start[i] <= j <= i."""
    T = kv_start.numel()
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    return (j >= kv_start.long()[:, None]) & (j <= i)


def vis_from_last(q_last):
    """[T, T] bool (query i, key j): j <= i <= q_last[j]."""
    T = q_last.numel()
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    return (j <= i) & (i <= q_last.long()[None, :])


def bounds(case):
    """(kv_start, q_last) int32 [B, T] and the visibility [B, T, T] of a case."""
    fam, T, D, Hkv, pa, pb = case
    ks = torch.stack([kv_start_of(pa, T), kv_start_of(pb, T)])
    ql = torch.stack([q_last_of(r) for r in ks])
    return ks, ql, torch.stack([vis_from_start(r) for r in ks])


# ------------------------------------------------------------------------------------------------ references
def fwd_ref(q, k, v, vis, scale):
    """``_attention_refs.fwd_ref`` with the mask given as vis [B, T, S]."""
    Hq, Hkv = q.shape[2], k.shape[2]
    hmap = A.head_map(Hq, Hkv)
    qd, kd, vd = A._bh(q), A._kvh(k, hmap), A._kvh(v, hmap)
    s = (scale * (qd @ kd.transpose(-1, -2))).masked_fill(~vis[:, None], -math.inf)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    lse = (m + l.log())[..., 0]
    amag = scale * (qd.abs() @ kd.abs().transpose(-1, -2))
    unit_lse = E32 * (amag.gather(-1, s.argmax(-1, keepdim=True))[..., 0] + lse.abs())
    return dict(o=((p @ vd).permute(0, 2, 1, 3), (EB * (p @ vd.abs())).permute(0, 2, 1, 3)),
                lse=(lse, unit_lse), p=p)


def bwd_ref(do, q, k, v, o, lse, vis, scale, cos=None, sin=None):
    """``_attention_refs.bwd_ref`` with the mask given as vis [B, T, S] (S = T: the rotation offset is 0)."""
    Hq, S, Hkv = q.shape[2], k.shape[1], k.shape[2]
    hmap = A.head_map(Hq, Hkv)
    qd, dod, od = A._bh(q), A._bh(do), A._bh(o)
    kd, vd = A._kvh(k, hmap), A._kvh(v, hmap)
    s = scale * (qd @ kd.transpose(-1, -2))
    p = torch.where(vis[:, None], torch.exp(s - lse.detach().cpu().to(F64)[..., None]), torch.zeros_like(s))
    dp = dod @ vd.transpose(-1, -2)
    delta = (dod * od).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    canc = E32 * p * (dod.abs() @ vd.abs().transpose(-1, -2) + delta.abs() + (dod * od).abs().sum(-1, keepdim=True))
    dv = p.transpose(-1, -2) @ dod
    unit_dv = EB * (p.transpose(-1, -2) @ dod.abs())
    dk = scale * (ds.transpose(-1, -2) @ qd)
    unit_dk = scale * (EB * (ds.abs().transpose(-1, -2) @ qd.abs()) + canc.transpose(-1, -2) @ qd.abs())
    dq = scale * (ds @ kd)
    part = torch.zeros_like(dq)
    for j0 in range(0, S, KEY_BLOCK):
        part += (ds[..., j0:j0 + KEY_BLOCK] @ kd[..., j0:j0 + KEY_BLOCK, :]).abs()
    unit_dq = scale * (EB * (ds.abs() @ kd.abs() + part) + canc @ kd.abs())
    dq, unit_dq = dq.permute(0, 2, 1, 3), unit_dq.permute(0, 2, 1, 3)
    dk, unit_dk = A._group_sum(dk, Hkv), A._group_sum(unit_dk, Hkv)
    dv, unit_dv = A._group_sum(dv, Hkv), A._group_sum(unit_dv, Hkv)
    if cos is not None:
        dq, unit_dq = A.rotate_back(dq, cos.to(F64), sin.to(F64), 0), A.rotate_back_unit(unit_dq, cos, sin, 0)
        dk, unit_dk = A.rotate_back(dk, cos.to(F64), sin.to(F64), 0), A.rotate_back_unit(unit_dk, cos, sin, 0)
    return dict(dq=(dq, unit_dq), dk=(dk, unit_dk), dv=(dv, unit_dv))


# ------------------------------------------------------------------------------------------------ cases
def _spread(Ts, families, pairs=PAIRS):
    """(T, pattern pair) x D x family, with Hkv in {4, 2, 1} spread over the cases as ``_attention_refs._spread``."""
    out = []
    for fam in families:
        gi = 0
        for T in Ts:
            for pa, pb in pairs:
                for di, D in enumerate((32, 64, 128)):
                    out.append((fam, T, D, (4, 2, 1)[(gi + di) % 3], pa, pb))
                gi += 1
    return out


def cases():
    """randn everywhere; count at T = 257 and 513 (lse = ln(visible keys) shows one key admitted or dropped); wide
    (row maxima that jump far past the forward's lazy-max threshold) at T = 513."""
    return _spread(GEOMS, ("randn",)) + _spread((257, 513), ("count",)) + _spread((513,), ("wide",))


def rope_cases():
    return _spread((ROPE_T,), ("randn",), (("docs", "window40"),))


def inputs(case):
    fam, T, D, Hkv, pa, pb = case
    return A.attn_inputs(fam, T, T, 1, D, Hkv)


@functools.lru_cache(maxsize=None)
def fwd_case(case):
    """(inputs with kv_start / q_last / vis, reference); computed once and shared: read-only."""
    inp = dict(inputs(case))
    inp["kv_start"], inp["q_last"], inp["vis"] = bounds(case)
    return inp, fwd_ref(inp["q"], inp["k"], inp["v"], inp["vis"], inp["scale"])


@functools.lru_cache(maxsize=None)
def bwd_case(case, mode="plain"):
    """The forward inputs plus o (the forward reference rounded to bf16) and lse (rounded to fp32); mode rope: RoPE
    tables, q / k taken as the rotated heads."""
    finp, fw = fwd_case(case)
    inp = dict(finp)
    inp.update(o=fw["o"][0].to(F32).to(BF16), lse=fw["lse"][0].to(F32), cos=None, sin=None)
    if mode == "rope":
        inp["cos"], inp["sin"] = A.rope_tables(case[1] + 3, case[2])
    ref = bwd_ref(inp["do"], inp["q"], inp["k"], inp["v"], inp["o"], inp["lse"], inp["vis"], inp["scale"],
                  inp["cos"], inp["sin"])
    return inp, ref


def fwd_checks(case, out):
    _, ref = fwd_case(case)
    return [("attn_o", "o", out["o"], ref["o"]), ("attn_lse", "lse", out["lse"], ref["lse"])]


def bwd_checks(case, out, mode="plain"):
    _, ref = bwd_case(case, mode)
    rot = "_rot" if mode == "rope" else ""
    return [("attn_dq" + rot, "dq", out["dq"], ref["dq"]), ("attn_dk" + rot, "dk", out["dk"], ref["dk"]),
            ("attn_dv", "dv", out["dv"], ref["dv"])]


def count_facts(case, out):
    """``_attention_refs.count_facts`` under the case's mask: lse[b, h, i] = ln(visible keys of row i of batch b) and
    o = the plain mean of the visible v rows."""
    fam, T, D, Hkv, pa, pb = case
    assert fam == "count"
    inp, _ = fwd_case(case)
    vis = inp["vis"]
    n = vis.sum(-1).to(F64)                                   # [B, T]
    lse = n.log()[:, None, :].expand(B, H, T)
    A.assert_close_ulps(out["lse"], lse, A.BUDGET["attn_lse"][1], A.BUDGET["attn_lse"][1] * E32 * lse,
                        what="count/lse = ln(visible keys)")
    vd = A._kvh(inp["v"], A.head_map(H, Hkv))                  # [B, H, T, D]
    mean = (vis.to(F64)[:, None] @ vd / n[:, None, :, None]).permute(0, 2, 1, 3)
    A.assert_close_ulps(out["o"], mean, 1, 2 * E32 * mean.abs(), what="count/o = mean of the visible v rows")
