"""fp64 reference, cases and per-element bound for the fused cross-entropy with z-loss and final-logit soft-capping
(op ``cross_entropy_aux``, csrc/cross_entropy.hip).

Not collected by pytest.  ``test_ce_aux_refs.py`` (CPU) checks the reference against fp64 autograd and calibrates the
budgets below; ``test_ce_aux_gpu.py`` runs the HIP kernel on the same cases against the same bounds.  Inputs, the
bound ``|out - ref| <= ulps * (ulp(ref) + unit)`` and the way budgets are set are those of ``_streaming_refs``
(``ce_inputs``, ``assert_close_ulps``, ``ulps_needed``): ``measured`` is the smallest integer budget at which a plain
fp32 torch evaluation on the CPU (``ce_aux_model_f32``), rounded to the kernel's output types, passes on all cases;
``budget`` is twice that.  Filled from ``pytest tests/test_ce_aux_refs.py -s`` (which fails when a row is stale);
nothing here was tuned against kernel output.

    op               measured  budget   outputs
    ---------------  --------  ------   ------------------------------------
    ce_aux_loss             1       2   per-row loss incl. the z term (fp32)
    ce_aux_lse              1       2   per-row log-sum-exp (fp32)
    ce_aux_dlogits          1       2   dlogits (bf16)

The fp32 model evaluates tanh as ``1 - 2 / (exp2(2 u log2 e) + 1)``, the form the kernel uses: NaN-free at
u = +-inf, absolute error about one fp32 ulp of 1 whatever |tanh| is.  That is why ``y`` carries an absolute unit.
"""
from __future__ import annotations

import math

import torch

import _streaming_refs as R
from _streaming_refs import BF16, E32, F32, F64, FLUSH, IGNORE

# op -> (measured, budget); see the table above
BUDGET = {
    "ce_aux_loss": (1, 2),
    "ce_aux_lse": (1, 2),
    "ce_aux_dlogits": (1, 2),
}

# (z_loss, softcap; 0: off).  z = 1e-4 is the recipes' value, but 1 + 2 z lse is then about 1.002, under one bf16 ulp
# of the gradient: a kernel that dropped the factor would pass.  At z = 0.5 it is about 10.  With inputs of 4 randn a
# cap of 30 leaves the derivative factor 1 - tanh^2 near 1; at 2 it spans (0, 1].
PAIRS = ((0.5, 0.0), (1e-4, 0.0), (0.0, 2.0), (0.0, 30.0), (0.5, 2.0))
AUX_V = (8, 4104, 16392, 53256, 131072)  # ragged and full; arms CH = 1, 2, 8, 16, 32 (R.ce_inputs)
FULL_PAIR = (0.5, 2.0)                    # this pair runs all of R.CE_V: every arm once


def cases():
    out = []
    for z, c in PAIRS:
        for V in (R.CE_V if (z, c) == FULL_PAIR else AUX_V):
            out.append((z, c, V))
    return out


def case_id(case):
    z, c, V = case
    return f"z{z:g}-c{c:g}-V{V}"


def ce_aux_ref(logits, targets, z, c, inv_n=None, ignore_index=IGNORE):
    """y = c tanh(x / c) (c = 0: x); lse = logsumexp(y); loss = lse - y_t + z lse^2;
    dx = (p (1 + 2 z lse) - onehot) inv_n (1 - (y / c)^2); ignored rows give loss 0, lse 0, gradient 0.
    x = -inf under a cap is y = -c: finite, and part of the softmax.

    Units (``ce_ref``'s, extended; g = 1 + 2 z lse, fac = 1 - (y / c)^2, th = y / c):
      unit_y   = 2^-23 (c + |y|): the tanh form's absolute error c 2^-23 plus the product's rounding (0 without cap).
      unit_lse = 2^-23 (|m| + |log sum| + sum_i p_i (1 + |y_i - m| log2 e))            ce_ref's terms without x_t
                 + unit_y(m) + sum_i p_i unit_y(i)                                     y's error through m and the sum
      unit_loss = unit_lse + 2^-23 |y_t| + unit_y(t)                                   the target logit
                 + 2 z |lse| unit_lse + 2^-23 z lse^2                                  the z term and its own rounding
      unit_dx  = inv_n { fac [ (2^-23 (p g (2 + |y - m| log2 e) + onehot) + 2^-126)    ce_ref's terms, p scaled by g
                               + p g (unit_y(i) + unit_y(m) + sum_j p_j unit_y(j))     y's error through p_i
                               + 2 z p unit_lse + 2^-23 p g ]                          g's error and rounding
                         + |p g - onehot| (2 |th| unit_y / c + 2^-23 (1 + th^2)) }     fac: y's error, its own rounding
    """
    x = logits.to(F64)
    N, V = x.shape
    valid = targets != ignore_index
    if inv_n is None:
        inv_n = 1.0 / max(int(valid.sum()), 1)
    if c:
        y = c * torch.tanh(x / c)
        unit_y = E32 * (c + y.abs())
        th = y / c
        fac = 1 - th * th
        dfac = 2 * th.abs() * unit_y / c + E32 * (1 + th * th)
    else:
        y = x
        unit_y = torch.zeros_like(x)
        fac = torch.ones_like(x)
        dfac = torch.zeros_like(x)
    m, mi = y.max(-1, keepdim=True)
    e = torch.exp(y - m)
    ssum = e.sum(-1, keepdim=True)
    p = e / ssum
    lse = m + ssum.log()
    tc = torch.where(valid, targets, torch.zeros_like(targets))
    yt = y.gather(1, tc[:, None])
    vd = valid[:, None].to(F64)
    g = 1 + 2 * z * lse
    loss = ((lse - yt + z * lse * lse) * vd)[:, 0]
    onehot = torch.zeros_like(x).scatter_(1, tc[:, None], 1.0)
    dl = (p * g - onehot) * inv_n * fac * vd
    dist = torch.where(p > 0, (y - m).abs() * math.log2(math.e), torch.zeros_like(x))
    uy_m = unit_y.gather(1, mi)
    uy_sum = (p * unit_y).sum(-1, keepdim=True)
    unit_lse = E32 * (m.abs() + ssum.log().abs() + (p * (1 + dist)).sum(-1, keepdim=True)) + uy_m + uy_sum
    unit_loss = unit_lse + E32 * yt.abs() + unit_y.gather(1, tc[:, None]) + 2 * z * lse.abs() * unit_lse \
        + E32 * z * lse * lse
    unit_dl = (fac * ((E32 * (p * g * (2 + dist) + onehot) + FLUSH) + p * g * (unit_y + uy_m + uy_sum)
                      + 2 * z * p * unit_lse + E32 * p * g)
               + (p * g - onehot).abs() * dfac) * inv_n * vd
    return dict(loss=(loss, (unit_loss * vd)[:, 0]), lse=((lse * vd)[:, 0], (unit_lse * vd)[:, 0]),
                dlogits=(dl, unit_dl))


def ce_aux_model_f32(logits, targets, z, c, inv_n=None):
    """The same in plain fp32 torch ops on the CPU, outputs rounded to the kernel's types."""
    x = logits.float()
    valid = targets != IGNORE
    if inv_n is None:
        inv_n = 1.0 / max(int(valid.sum()), 1)
    if c:
        q = 2.0 / (torch.exp2(x * torch.tensor(2 * math.log2(math.e) / c, dtype=F32)) + 1.0)
        y = torch.tensor(c, dtype=F32) * (1.0 - q)
        fac = q * (2.0 - q)
    else:
        y, fac = x, torch.ones_like(x)
    lse = torch.logsumexp(y, -1, keepdim=True)
    tc = torch.where(valid, targets, torch.zeros_like(targets))
    vf = valid[:, None].float()
    zf = torch.tensor(z, dtype=F32)
    loss = (lse - y.gather(1, tc[:, None]) + zf * lse * lse) * vf
    onehot = torch.zeros_like(x).scatter_(1, tc[:, None], 1.0)
    dl = ((y - lse).exp() * (1 + 2 * zf * lse) - onehot) * torch.tensor(inv_n, dtype=F32) * fac * vf
    return dict(loss=loss[:, 0], lse=(lse * vf)[:, 0], dlogits=dl.to(BF16))


def checks(inp, out, z, c, inv_n=None):
    """(op, name, out, (ref64, unit)) tuples for the outputs present in ``out`` (loss, lse, dlogits)."""
    ref = ce_aux_ref(inp["logits"], inp["targets"], z, c, inv_n)
    return [(f"ce_aux_{k}", k, out[k], ref[k]) for k in ("loss", "lse", "dlogits") if out.get(k) is not None]


def check_all(items, budget=None):
    """Every item within its op's budget (or ``budget[op]``, for the calibration)."""
    for op, name, o, (ref, unit) in items:
        u = BUDGET[op][1] if budget is None else budget[op]
        R.assert_close_ulps(o, ref, u, u * torch.as_tensor(unit, dtype=F64), what=f"{op}/{name}")


def needed(items):
    """op -> smallest integer budget at which these items pass."""
    need = {}
    for op, _, o, (ref, unit) in items:
        need[op] = max(need.get(op, 0), R.ulps_needed(o, ref, unit))
    return need
