"""fp64 references, case builders and the per-element bound for the attention kernels (``attn_fwd``,
``attn_bwd`` with and without RoPE rotate-back / a ready ``delta``, ``attention_block_bwd``, ``attn_decode``).

Not collected by pytest.  ``test_attention_refs.py`` (CPU) checks the references against independent PyTorch
double-precision paths, calibrates the budgets below and shows that the checks catch single-tile defects;
``test_attention_edges_gpu.py`` runs the HIP kernels on the same cases against the same bounds.

Conventions.  q, do, o, dq are [B, T, H, D]; k, v, dk, dv [B, S, Hkv, D]; lse is [B, H, T] in natural log.
Queries are aligned to the END of the keys: under the causal mask key j is visible to query i iff
j <= i + S - T.  Query head h reads kv head h // (H / Hkv).  The backward is a function of all six inputs
(do, q, k, v, o, lse), as the op is: P = exp(s - lse) with the lse it is handed, delta = rowsum(dO o) with the
bf16 o it is handed, dS = P (dO V^T - delta), dV = P^T dO, dK = scale dS^T Q, dQ = scale dS K.  The GPU file feeds
the kernel the reference's o rounded to bf16 and its lse rounded to fp32, so the backward is judged on its own, and
the same form covers the context-parallel use, where the lse of the whole row comes with a partial key block.

The bound.  Every element must satisfy

    |out - ref| <= ulps * (ulp_out(ref) + unit)

(``assert_close_ulps`` of ``_streaming_refs`` with ``abs_floor = ulps * unit``).  ``unit`` is the rounding
granularity times the magnitudes of the terms being summed; it follows from the roundings the kernel headers
document (fp32 scores from bf16 inputs; P and dS rounded to bf16, relative error 2^-9, before the MFMA that
consumes them; fp32 accumulation; dQ rounded to bf16 once per 256-key block, the blocks summed in fp32) and the
kernel output plays no part in it:

    o           2^-9 sum_j P_ij |V_jd|
    lse (fp32)  2^-23 (scale sum_d |q_id| |k_jd| at the row's largest score j  +  |lse|)
    dv          2^-9 sum_i P_ij |dO_id|
    dk          scale (2^-9 sum_i |dS_ij| |Q_id|  +  sum_i c_ij |Q_id|)
    dq          scale (2^-9 (sum_j |dS_ij| |K_jd| + sum_blocks |partial of that 256-key block|)  +  sum_j c_ij |K_jd|)
    rotated-back dq / dk    |cos| unit[d] + |sin| unit[partner(d)]
    decode o    2^-23 sum_j P_j |V_jd|   (all fp32; one rounding to bf16 at the end)

c_ij = 2^-23 P_ij (sum_d |dO_id| |V_jd| + |delta_i| + sum_d |dO_id o_id|) is the fp32 error of dS where dP - delta
cancels: dP is an fp32 sum of the magnitudes sum_d |dO| |V|, delta is subtracted from it at |delta|, and delta is
itself an fp32 sum of the magnitudes sum_d |dO o| (attn_bwd_pre_kernel, or the caller's fp32 delta).  dS feeds dK and
dQ alike, so the term stands in both (a causal row that sees one key has dS = 0 exactly in the reference while the
kernel's two fp32 sums of the same products may differ in their last bit).  Sums over the query heads of a GQA group
add their units.  Where a reference element is exactly 0 and its unit is 0, only an exact 0 passes; there is no
absolute floor.

Budgets.  ``measured`` is the smallest integer budget at which a plain PyTorch CPU model of the op (``*_model``
below: exactly the roundings listed above, nothing else) passes on all of that op's cases; ``budget`` is twice that
(a different summation order; v_exp / v_rcp / v_log at about 1 fp32 ulp).  Filled from
``pytest tests/test_attention_refs.py`` (which fails when a row is stale); nothing here was tuned against kernel
output.

    op            measured  budget   outputs
    ------------  --------  ------   ------------------------------------------------
    attn_o               2       4   attn_fwd o (bf16)
    attn_lse             1       2   attn_fwd lse (fp32)
    attn_dq              2       4   attn_bwd / attention_block_bwd dq (bf16)
    attn_dk              2       4   dk (bf16)
    attn_dv              2       4   dv (bf16)
    attn_dq_rot          1       2   dq rotated back (RoPE tables)
    attn_dk_rot          2       4   dk rotated back
    decode_o             1       2   attn_decode o (bf16)
"""
from __future__ import annotations

import functools
import math

import torch

from _streaming_refs import BF16, E32, F32, F64, _err_and_ulp, _gen, assert_close_ulps, ulps_needed  # noqa: F401

# op -> (measured, budget); see the table above
BUDGET = {
    "attn_o": (2, 4),
    "attn_lse": (1, 2),
    "attn_dq": (2, 4),
    "attn_dk": (2, 4),
    "attn_dv": (2, 4),
    "attn_dq_rot": (1, 2),
    "attn_dk_rot": (2, 4),
    "decode_o": (1, 2),
}

EB = 2.0 ** -9   # relative error of one rounding to bf16
KEY_BLOCK = 256  # keys per backward workgroup = per bf16 dQ slab
B, H = 2, 4


def check(op, out, ref_unit, what):
    """``out`` against a reference ``(ref64, unit)`` under the op's budget."""
    ref, unit = ref_unit
    u = BUDGET[op][1]
    assert_close_ulps(out, ref, u, u * torch.as_tensor(unit, dtype=F64), what=f"{op}/{what}")


def worst_ratio(op, out, ref_unit):
    """max over the elements of |out - ref| / (budget (ulp_out(ref) + unit)): 1 is the bound.  Information only."""
    ref, unit = ref_unit
    _, r, err, ulp = _err_and_ulp(out, ref)
    q = torch.where(err == 0, torch.zeros_like(err), err / (ulp + torch.as_tensor(unit, dtype=F64).expand_as(r)))
    return float(q.max()) / BUDGET[op][1] if q.numel() else 0.0


# ------------------------------------------------------------------------------------------------ helpers
def visible(T, S, causal):
    """[T, S] bool: key j is visible to query i."""
    if not causal:
        return torch.ones(T, S, dtype=torch.bool)
    return torch.arange(S)[None, :] <= torch.arange(T)[:, None] + (S - T)


def head_map(Hq, Hkv):
    return torch.arange(Hq) // (Hq // Hkv)


def _bh(x, dt=F64):
    """[B, L, H, D] -> [B, H, L, D] in ``dt`` on the CPU."""
    return x.detach().cpu().to(dt).permute(0, 2, 1, 3)


def _kvh(x, hmap, dt=F64):
    return _bh(x, dt)[:, hmap]


def _group_sum(x, Hkv):
    """[B, H, S, D] -> [B, S, Hkv, D]: the query heads of a group summed."""
    Bb, Hq, S, D = x.shape
    return x.reshape(Bb, Hkv, Hq // Hkv, S, D).sum(2).permute(0, 2, 1, 3)


def rotate_back(g, cos, sin, pos0):
    """R^T of the rotate-half convention on g [B, L, H, D]: (x, y) at dims (d, d + D/2) of the row at position
    pos0 + l -> (x c + y s, y c - x s); cos / sin [positions, D/2]."""
    L, D = g.shape[1], g.shape[3]
    c = cos[pos0:pos0 + L].to(g.dtype)[None, :, None, :]
    s = sin[pos0:pos0 + L].to(g.dtype)[None, :, None, :]
    x, y = g[..., : D // 2], g[..., D // 2:]
    return torch.cat([x * c + y * s, y * c - x * s], -1)


def rotate_back_unit(unit, cos, sin, pos0):
    """|cos| unit[d] + |sin| unit[partner(d)]."""
    L, D = unit.shape[1], unit.shape[3]
    c = cos[pos0:pos0 + L].to(F64).abs()[None, :, None, :]
    s = sin[pos0:pos0 + L].to(F64).abs()[None, :, None, :]
    x, y = unit[..., : D // 2], unit[..., D // 2:]
    return torch.cat([x * c + y * s, y * c + x * s], -1)


def rope_tables(n, D, theta=10000.0):
    """fp32 cos / sin [n, D/2], as the model builds them."""
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=F64) / D))
    fr = torch.outer(torch.arange(n, dtype=F64), inv)
    return fr.cos().to(F32), fr.sin().to(F32)


# ------------------------------------------------------------------------------------------------ references
def fwd_ref(q, k, v, causal, scale):
    """o = softmax(scale q k^T + mask) v and lse = logsumexp of the masked scores, in fp64 from the bf16 inputs.
    Returns o / lse as (ref, unit) and the probabilities p [B, H, T, S]."""
    T, Hq, S, Hkv = q.shape[1], q.shape[2], k.shape[1], k.shape[2]
    hmap = head_map(Hq, Hkv)
    qd, kd, vd = _bh(q), _kvh(k, hmap), _kvh(v, hmap)
    vis = visible(T, S, causal)
    s = (scale * (qd @ kd.transpose(-1, -2))).masked_fill(~vis, -math.inf)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    lse = (m + l.log())[..., 0]
    amag = scale * (qd.abs() @ kd.abs().transpose(-1, -2))
    unit_lse = E32 * (amag.gather(-1, s.argmax(-1, keepdim=True))[..., 0] + lse.abs())
    return dict(o=((p @ vd).permute(0, 2, 1, 3), (EB * (p @ vd.abs())).permute(0, 2, 1, 3)),
                lse=(lse, unit_lse), p=p)


def bwd_ref(do, q, k, v, o, lse, causal, scale, cos=None, sin=None):
    """dq, dk, dv as (ref, unit) from all six inputs (see the module docstring).  With RoPE tables q / k are the
    rotated heads and dq / dk are rotated back (query t at position t + S - T, key j at position j)."""
    T, Hq, S, Hkv = q.shape[1], q.shape[2], k.shape[1], k.shape[2]
    hmap = head_map(Hq, Hkv)
    qd, dod, od = _bh(q), _bh(do), _bh(o)
    kd, vd = _kvh(k, hmap), _kvh(v, hmap)
    vis = visible(T, S, causal)
    s = scale * (qd @ kd.transpose(-1, -2))
    p = torch.where(vis, torch.exp(s - lse.detach().cpu().to(F64)[..., None]), torch.zeros_like(s))
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
    dk, unit_dk = _group_sum(dk, Hkv), _group_sum(unit_dk, Hkv)
    dv, unit_dv = _group_sum(dv, Hkv), _group_sum(unit_dv, Hkv)
    if cos is not None:
        dq, unit_dq = rotate_back(dq, cos.to(F64), sin.to(F64), S - T), rotate_back_unit(unit_dq, cos, sin, S - T)
        dk, unit_dk = rotate_back(dk, cos.to(F64), sin.to(F64), 0), rotate_back_unit(unit_dk, cos, sin, 0)
    return dict(dq=(dq, unit_dq), dk=(dk, unit_dk), dv=(dv, unit_dv))


def decode_ref(q, k, v, scale, counts):
    """One query per sequence over the first counts[b] keys of k / v [B, S, Hkv, D]; a count of 0 gives zeros."""
    Bb, _, Hq, D = q.shape
    o = torch.zeros(Bb, 1, Hq, D, dtype=F64)
    unit = torch.zeros_like(o)
    for b, n in enumerate(counts):
        if n > 0:
            r = fwd_ref(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], False, scale)["o"]
            o[b], unit[b] = r[0][0], r[1][0] * (E32 / EB)
    return o, unit


# ------------------------------------------------------------------------------------------------ fp32 / bf16 models
def _scores32(q, k, hmap, scale):
    return (_bh(q, F32) @ _kvh(k, hmap, F32).transpose(-1, -2)) * torch.tensor(scale, dtype=F32)


def fwd_model(q, k, v, causal, scale, vis=None, hmap=None, p_bf16=True):
    """The forward in plain PyTorch with the documented roundings: fp32 scores from the bf16 inputs, P rounded to
    bf16 before the PV product (not for the decode kernel, which is all fp32), fp32 accumulation, the row sum from
    the unrounded P.  ``vis`` / ``hmap`` replace the mask / the head map (the defect tests)."""
    T, Hq, S, Hkv = q.shape[1], q.shape[2], k.shape[1], k.shape[2]
    hmap = head_map(Hq, Hkv) if hmap is None else hmap
    vis = visible(T, S, causal) if vis is None else vis
    s = _scores32(q, k, hmap, scale).masked_fill(~vis, -math.inf)
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    pv = (p.to(BF16).to(F32) if p_bf16 else p) @ _kvh(v, hmap, F32)
    return dict(o=(pv / l).permute(0, 2, 1, 3).to(BF16), lse=(m + l.log())[..., 0])


def bwd_model(do, q, k, v, o, lse, causal, scale, cos=None, sin=None, vis=None, hmap=None):
    """The backward with the documented roundings: fp32 scores, P = exp(s - lse) and dS = P (dP - delta) rounded to
    bf16 (dS from the fp32 P), fp32 accumulation of dV / dK over all queries and the heads of a group, dQ rounded to
    bf16 once per 256-key block and the blocks summed in fp32, the rotation in fp32 before the one output rounding."""
    T, Hq, S, Hkv = q.shape[1], q.shape[2], k.shape[1], k.shape[2]
    hmap = head_map(Hq, Hkv) if hmap is None else hmap
    vis = visible(T, S, causal) if vis is None else vis
    sc = torch.tensor(scale, dtype=F32)
    qf, dof, of = _bh(q, F32), _bh(do, F32), _bh(o, F32)
    kf, vf = _kvh(k, hmap, F32), _kvh(v, hmap, F32)
    p = torch.where(vis, torch.exp(_scores32(q, k, hmap, scale) - lse.to(F32)[..., None]), torch.zeros(()))
    delta = (dof * of).sum(-1, keepdim=True)
    ds = (p * (dof @ vf.transpose(-1, -2) - delta)).to(BF16).to(F32)
    dv = p.to(BF16).to(F32).transpose(-1, -2) @ dof
    dk = (ds.transpose(-1, -2) @ qf) * sc
    dq = torch.zeros_like(qf)
    for j0 in range(0, S, KEY_BLOCK):
        dq += (ds[..., j0:j0 + KEY_BLOCK] @ kf[..., j0:j0 + KEY_BLOCK, :]).to(BF16).to(F32)
    dq = (dq * sc).permute(0, 2, 1, 3)
    # a defective head map still sums into the true groups' slots: only the shapes matter to the callers
    dk, dv = _group_sum(dk, Hkv), _group_sum(dv, Hkv)
    if cos is not None:
        dq, dk = rotate_back(dq, cos, sin, S - T), rotate_back(dk, cos, sin, 0)
    return dict(dq=dq.to(BF16), dk=dk.to(BF16), dv=dv.to(BF16))


def decode_model(q, k, v, scale, counts):
    o = torch.zeros(q.shape, dtype=BF16)
    for b, n in enumerate(counts):
        if n > 0:
            o[b] = fwd_model(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], False, scale, p_bf16=False)["o"][0]
    return o


# ------------------------------------------------------------------------------------------------ inputs
FAMILIES = ("randn", "wide", "count")


def attn_inputs(family, T, S, causal, D, Hkv):
    """bf16 q [B, T, H, D], k / v [B, S, Hkv, D], do like q; scale = D^-1/2.

    randn: q, k ~ N(0, 0.8^2), v, do ~ N(0, 1).  wide: q, k ~ N(0, 2.5^2), and keys in late tiles aligned (x 3) with
    late queries, so that row maxima jump by far more than the forward's lazy-max threshold (2^8) after many tiles
    were accumulated.  count: q = 0, so every visible key has p = 1 before normalisation: lse = ln(visible keys) and
    o is the plain mean of the visible v rows; v and do are small integers (sums exact in fp32)."""
    g = _gen(11, FAMILIES.index(family), T, S, causal, D, Hkv)
    rn = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    q, k = rn(B, T, H, D), rn(B, S, Hkv, D)
    v, do = rn(B, S, Hkv, D), rn(B, T, H, D)
    if family == "randn":
        q, k = 0.8 * q, 0.8 * k
    elif family == "wide":
        q, k = 2.5 * q, 2.5 * k
        off = S - T
        for h, (i, j) in enumerate(((T - 1, T - 1 + off), (T - 1 - T // 8, max(0, off + T // 3)),
                                    (T // 2, min(S - 1, T // 2 + off)), (T - 2, S // 2 if not causal else off))):
            j = max(0, min(j, S - 1))  # visible to query i under the causal mask: j <= i + off
            k[:, j, h // (H // Hkv)] = q[:, i, h] * 3.0
    else:
        q = torch.zeros_like(q)
        v = torch.randint(-4, 5, v.shape, generator=g).to(F32)
        do = torch.randint(-4, 5, do.shape, generator=g).to(F32)
    return dict(q=q.to(BF16), k=k.to(BF16), v=v.to(BF16), do=do.to(BF16), causal=bool(causal),
                scale=1.0 / math.sqrt(D))


def _spread(geoms, families=("randn",)):
    """geometry x D x family, with Hkv in {4, 2, 1} spread over the cases, not crossed with them."""
    out = []
    for fam in families:
        for gi, (T, S, causal) in enumerate(geoms):
            for di, D in enumerate((32, 64, 128)):
                out.append((fam, T, S, causal, D, (4, 2, 1)[(gi + di) % 3]))
    return out


# (T, S, causal).  The forward's tile is 256 queries at D <= 64 (wave w owns the 32-query sub-blocks w and 7 - w) and
# 128 at D = 128; key tiles are 64; a tile runs the code path MASK 3 (both of a wave's sub-blocks see it), 1 or 2.
FWD_GEOMS = (
    (1, 1, 1),       # one query, one key: a sub-block with one live row, lse = 0
    (1, 65, 1),      # one query through attn_fwd, two key tiles, the second holding one key
    (31, 31, 1),     # a partly filled sub-block
    (33, 33, 1),     # a second sub-block of one row (D <= 64: wave 1's block; MASK 1 throughout)
    (64, 64, 1),     # exactly one key tile
    (65, 65, 1),     # a second key tile of one key
    (129, 129, 1),   # the second workgroup at D = 128; at D <= 64 only wave 3's second block (row 128) sees the third
                     # key tile: MASK 2
    (257, 257, 1),   # the second workgroup at D <= 64: a wave's blocks w and 7 - w partly or wholly past T
    (200, 264, 1),   # offset 64: the diagonal one key tile to the right
    (300, 340, 1),   # offset 40, no multiple of 32: the diagonal is aligned with neither the sub-blocks nor the key
                     # tiles, so every diagonal tile takes the per-element masked path
    (96, 700, 0),    # non-causal, a ragged last key tile (700 = 10 x 64 + 60)
    (130, 70, 0),    # T > S, non-causal
    (513, 513, 1),   # three workgroups (five at D = 128): MASK 3 then 2 along a wave's sweep, MASK 1 in the last
                     # workgroup, whose blocks past row 512 are dead
)
WIDE_GEOMS = ((257, 257, 1), (300, 340, 1), (96, 700, 0), (513, 513, 1))


def fwd_cases():
    return _spread(FWD_GEOMS, ("randn", "count")) + _spread(WIDE_GEOMS, ("wide",))


# The backward: a workgroup owns 256 keys (eight waves of 32 at D <= 64, the fused-role kernel; four waves of 64 at
# D = 128, the key-stationary kernel) and sweeps the queries in slices of 128 / 32 rows.
BWD_GEOMS = (
    (33, 33, 1),     # one key block, a second 32-query sub-block of one row
    (200, 200, 1),   # one ragged key block, two query slices at D <= 64
    (257, 257, 1),   # a second key block of one key
    (513, 513, 1),   # three key blocks
    (300, 340, 1),   # offset 40: the first visible query of a key block (qb_start) inside a sub-block
    (200, 264, 1),   # offset 64
    (40, 600, 1),    # offset 560: two key blocks wholly visible to every query, the third ragged
    (96, 700, 0),    # non-causal, ragged third key block
    (130, 70, 0),    # T > S, non-causal
)
BWD_WIDE_GEOMS = ((300, 340, 1), (513, 513, 1))
BWD_COUNT_GEOMS = ((257, 257, 1), (40, 600, 1), (130, 70, 0))
ROPE_GEOMS = ((200, 264, 1), (300, 340, 1))
PARTIAL_GEOMS = ((200, 264, 1), (96, 700, 0))


def bwd_cases():
    return _spread(BWD_GEOMS) + _spread(BWD_WIDE_GEOMS, ("wide",)) + _spread(BWD_COUNT_GEOMS, ("count",))


def rope_cases():
    return _spread(ROPE_GEOMS)


def partial_cases():
    return _spread(PARTIAL_GEOMS)


@functools.lru_cache(maxsize=None)
def fwd_case(case):
    """(inputs, reference) of a forward case; computed once and shared: treat both as read-only."""
    inp = attn_inputs(*case)
    return inp, fwd_ref(inp["q"], inp["k"], inp["v"], inp["causal"], inp["scale"])


@functools.lru_cache(maxsize=None)
def bwd_case(case, mode="plain"):
    """(inputs, reference) of a backward case: the forward inputs plus ``o`` (the forward reference rounded to bf16)
    and ``lse`` (rounded to fp32).  mode rope: RoPE tables, q / k taken as the rotated heads.  mode partial: the
    context-parallel case -- the key block is part of a longer row, so the lse handed in is
    logaddexp(lse_block, lse_rest) with lse_rest larger by 0.5 .. 2.5, and o is the whole row's output, the matching
    mix of the block's o and another block's; P = exp(s - lse) then sums to less than 1 / 2."""
    inp = dict(attn_inputs(*case))
    fam, T, S, causal, D, Hkv = case
    fw = fwd_ref(inp["q"], inp["k"], inp["v"], inp["causal"], inp["scale"])
    o, lse = fw["o"][0], fw["lse"][0]
    if mode == "partial":
        g = _gen(12, T, S, D)
        rest = lse + 0.5 + 2 * torch.rand(lse.shape, generator=g, dtype=F64)
        tot = torch.logaddexp(lse, rest)
        w = torch.exp(lse - tot).permute(0, 2, 1)[..., None]
        o = w * o + (1 - w) * torch.randn(o.shape, generator=g, dtype=F64)
        lse = tot
    inp.update(o=o.to(F32).to(BF16), lse=lse.to(F32), cos=None, sin=None)
    if mode == "rope":
        inp["cos"], inp["sin"] = rope_tables(S + 3, D)  # a table longer than S
    ref = bwd_ref(inp["do"], inp["q"], inp["k"], inp["v"], inp["o"], inp["lse"], inp["causal"], inp["scale"],
                  inp["cos"], inp["sin"])
    return inp, ref


def bwd_args(inp):
    return (inp["do"], inp["q"], inp["k"], inp["v"], inp["o"], inp["lse"], inp["causal"], inp["scale"],
            inp["cos"], inp["sin"])


def fwd_checks(case, out):
    _, ref = fwd_case(case)
    return [("attn_o", "o", out["o"], ref["o"]), ("attn_lse", "lse", out["lse"], ref["lse"])]


def bwd_checks(case, out, mode="plain"):
    _, ref = bwd_case(case, mode)
    rot = "_rot" if mode == "rope" else ""
    return [("attn_dq" + rot, "dq", out["dq"], ref["dq"]), ("attn_dk" + rot, "dk", out["dk"], ref["dk"]),
            ("attn_dv", "dv", out["dv"], ref["dv"])]


def check_all(items):
    for op, name, out, ref_unit in items:
        check(op, out, ref_unit, name)


def count_facts(case, out):
    """The count family's own facts, apart from the generic bound: lse[i] = ln(number of visible keys of row i)
    within the fp32 budget, so that one key admitted or dropped shows on its row for any T and S (the nearest
    wrong count changes lse by 1 / n >= 1 / S, far over 2^-23 ln n); and o = the plain mean of the visible v rows
    (p is exactly 1 and every sum of at most S small integers is exact in fp32, so what remains is the output
    rounding, at most 1 bf16 ulp in this file's convention, and the fp32 reciprocal of n and the product with it,
    2 x 2^-23 relative)."""
    fam, T, S, causal, D, Hkv = case
    assert fam == "count"
    inp, _ = fwd_case(case)
    vis = visible(T, S, causal)
    n = vis.sum(-1).to(F64)
    lse = n.log()[None, None, :].expand(B, H, T)
    assert_close_ulps(out["lse"], lse, BUDGET["attn_lse"][1], BUDGET["attn_lse"][1] * E32 * lse,
                      what="count/lse = ln(visible keys)")
    vd = _kvh(inp["v"], head_map(H, Hkv))
    mean = (vis.to(F64) @ vd / n[:, None]).permute(0, 2, 1, 3)
    assert_close_ulps(out["o"], mean, 1, 2 * E32 * mean.abs(), what="count/o = mean of the visible v rows")


# ------------------------------------------------------------------------------------------------ decode
# (D, H, Hkv): group sizes 1, 2, 4, 8
DECODE_HEADS = ((32, 8, 8), (64, 8, 4), (128, 8, 2), (64, 8, 1))
DECODE_S = (1, 2, 63, 64, 65, 257, 1000)


def decode_splits(Bb, Hkv, S):
    """attn_decode_splits of attn_decode.hip, restated to document which split count a case reaches."""
    want, cap = -(-512 // (Bb * Hkv)), -(-S // 64)
    return max(1, min(want, cap, 64))


def decode_cases():
    """(D, H, Hkv, B, S buffer rows, counts).  counts None: the key count is the host shape; an int: a device scalar
    smaller than the buffer; a tuple: one count per sequence.  Rows of the buffer past a sequence's count are NaN.

    With B = 2 the split count is min(ceil(512 / (B Hkv)), ceil(S / 64)): 1 up to S = 64, 2 at 65, 5 at 257, 16 at
    1000 (capped by S).  B = 64, Hkv = 8: 1 split with S = 130 > 64 (B Hkv >= 512).  B = 8, Hkv = 8, S = 1000: 8
    splits, capped by the grid (want < cap).  B = 1, Hkv = 2, S = 4100: capped at 64 splits.  Per-sequence counts
    with B = 5, S = 1000 (n = 13 splits at Hkv = 8, else 16, each of ceil(count / n) keys): count 1 leaves all splits
    but one empty, 65 at n = 16 -> chunks of 5 with 3 empty splits, 0 -> every split empty, the kernel writes zeros."""
    out = [(D, Hq, Hkv, 2, S, None) for S in DECODE_S for (D, Hq, Hkv) in DECODE_HEADS]
    out += [(32, 8, 8, 64, 130, None), (64, 8, 8, 8, 1000, None), (32, 4, 2, 1, 4100, None)]
    out += [(D, Hq, Hkv, 2, 1000, n) for (D, Hq, Hkv), n in zip(DECODE_HEADS, (1, 63, 257, 700))]
    out += [(D, Hq, Hkv, 5, 1000, (0, 1, 1000, 65, 300)) for (D, Hq, Hkv) in DECODE_HEADS]
    out += [(64, 8, 4, 2, 300, (0, 0))]
    return out


def decode_counts(case):
    D, Hq, Hkv, Bb, S, counts = case
    return [S] * Bb if counts is None else ([counts] * Bb if isinstance(counts, int) else list(counts))


@functools.lru_cache(maxsize=None)
def decode_case(case):
    D, Hq, Hkv, Bb, S, counts = case
    g = _gen(13, D, Hq, Hkv, Bb, S, *decode_counts(case))
    q = (0.8 * torch.randn(Bb, 1, Hq, D, generator=g)).to(BF16)
    k = (0.8 * torch.randn(Bb, S, Hkv, D, generator=g)).to(BF16)
    v = torch.randn(Bb, S, Hkv, D, generator=g).to(BF16)
    for b, n in enumerate(decode_counts(case)):
        k[b, n:], v[b, n:] = math.nan, math.nan
    inp = dict(q=q, k=k, v=v, scale=1.0 / math.sqrt(D), counts=decode_counts(case))
    return inp, decode_ref(q, k, v, inp["scale"], inp["counts"])
