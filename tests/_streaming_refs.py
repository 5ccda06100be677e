"""fp64 references, case builders and the per-element bound for the streaming kernels
(norms, activations, SwiGLU, cross-entropy, AdamW, gradient norm).

Not collected by pytest.  ``test_streaming_refs.py`` (CPU) checks the references against
independent PyTorch double-precision paths and calibrates the budgets below;
``test_streaming_edges_gpu.py`` runs the HIP kernels on the same cases against the same bounds.

The bound.  Every element must satisfy

    |out - ref| <= ulps * ulp(ref) + abs_floor,        ulp(ref) = 2^-8 |ref|  (bf16 outputs)
                                                                  2^-23 |ref| (fp32 outputs)

(ulp(ref) is clamped from below at the format's denormal spacing, 2^-133 / 2^-149).  Where the op
cancels, ``abs_floor = ulps * unit`` and ``unit`` is fp32's 2^-23 times the magnitudes of the terms
being cancelled (documented at each reference), plus 2^-126 times the gain where an intermediate
below fp32's smallest normal may be flushed by the hardware exp / rcp.  The floor scales with the
budget so that a zero budget demands exact results.

Budgets.  ``measured`` is the smallest integer budget at which a plain PyTorch fp32 (CPU) evaluation
of the op, rounded to the kernel's output type, passes on all of that op's cases; ``budget`` is
twice that (a different summation order; v_exp / v_rcp at about 1 fp32 ulp instead of correctly
rounded functions).  Ops that only select or copy values (ReLU, the bf16 residual sum) are exact:
budget 0.  Filled from ``pytest tests/test_streaming_refs.py`` (which fails when a row is stale);
nothing here was tuned against kernel output.

    op            measured  budget   outputs
    ------------  --------  ------   ------------------------------------------------
    norm_y               2       4   y (bf16)
    norm_stats           2       4   mean, rstd (fp32)
    norm_dx              1       2   dx (bf16)
    norm_dwdb            1       2   dw, db (bf16 / fp32), column sums of dx
    gelu_fwd             1       2   act_fwd op 1
    gelu_bwd             1       2   act_bwd / act_bwd_bias op 1 (dx)
    swiglu_fwd           1       2   swiglu_fwd
    swiglu_bwd           1       2   swiglu_bwd
    colsum               1       2   act_bwd_bias bias_acc (bf16 / fp32)
    ce_loss              2       4   per-row loss (fp32)
    ce_dlogits           1       2   dlogits (bf16)
    adamw                2       4   update, m, v (fp32)
    sumsq                1       2   sumsq, grad_norm_clip (fp32)
    exact                0       0   relu fwd / bwd, residual sum s
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

# op -> (measured, budget); see the table above
BUDGET = {
    "norm_y": (2, 4),
    "norm_stats": (2, 4),
    "norm_dx": (1, 2),
    "norm_dwdb": (1, 2),
    "gelu_fwd": (1, 2),
    "gelu_bwd": (1, 2),
    "swiglu_fwd": (1, 2),
    "swiglu_bwd": (1, 2),
    "colsum": (1, 2),
    "ce_loss": (2, 4),
    "ce_dlogits": (1, 2),
    "adamw": (2, 4),
    "sumsq": (1, 2),
    "exact": (0, 0),
}

EPS_OUT = {BF16: 2.0 ** -8, F32: 2.0 ** -23}
DENORM = {BF16: 2.0 ** -133, F32: 2.0 ** -149}
E32 = 2.0 ** -23     # fp32 ulp of 1
FLUSH = 2.0 ** -126  # fp32 smallest normal: smaller intermediates may be flushed to zero


# ------------------------------------------------------------------------------------------------ the bound
def _err_and_ulp(out, ref64, fmt=None):
    fmt = fmt or out.dtype  # fmt: the output format of a value held in fp64 (a difference of two fp32 outputs)
    assert fmt in EPS_OUT, f"output dtype {fmt}"
    o = out.detach().cpu().to(F64)
    r = ref64.detach().cpu().to(F64)
    assert o.shape == r.shape, f"shape {tuple(o.shape)} vs reference {tuple(r.shape)}"
    err = (o - r).abs()
    err = torch.where(torch.isinf(o) & (o == r), torch.zeros_like(err), err)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)  # NaN, or a wrong infinity
    ulp = (r.abs() * EPS_OUT[fmt]).clamp_min(DENORM[fmt])
    ulp = torch.where(torch.isfinite(ulp), ulp, torch.zeros_like(ulp))
    return o, r, err, ulp


def assert_close_ulps(out, ref64, ulps, abs_floor=0.0, what="output", fmt=None):
    """Every element of ``out`` (bf16 or fp32) within ``ulps * ulp(ref) + abs_floor`` of ``ref64``."""
    o, r, err, ulp = _err_and_ulp(out, ref64, fmt)
    floor = torch.as_tensor(abs_floor, dtype=F64).cpu().expand_as(r)
    bound = ulps * ulp + floor
    bad = ~(err <= bound)
    if bad.any():
        excess = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        flat = int(excess.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), r.shape)) if r.dim() else ()
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {r.numel()} elements out of bound (ulps={ulps}); worst at {idx}: "
            f"out={o.reshape(-1)[flat].item():.9g} ref={r.reshape(-1)[flat].item():.9g} "
            f"err={err.reshape(-1)[flat].item():.3g} bound={bound.reshape(-1)[flat].item():.3g}")


def ulps_needed(out, ref64, unit=0.0, fmt=None):
    """Smallest integer u with |out - ref| <= u * (ulp(ref) + unit) on every element."""
    _, r, err, ulp = _err_and_ulp(out, ref64, fmt)
    unit = torch.as_tensor(unit, dtype=F64).cpu().expand_as(r)
    q = torch.where(err == 0, torch.zeros_like(err), err / (ulp + unit))
    m = float(q.max()) if q.numel() else 0.0
    return math.inf if not math.isfinite(m) else int(math.ceil(m))


def check(op, out, ref_unit, what, fmt=None):
    """``out`` against a reference ``(ref64, unit)`` under the op's budget."""
    ref, unit = ref_unit
    u = BUDGET[op][1]
    assert_close_ulps(out, ref, u, u * torch.as_tensor(unit, dtype=F64), what=f"{op}/{what}", fmt=fmt)


def check_all(items):
    """``items``: (op, name, out, (ref64, unit)[, fmt]) tuples as the ``*_checks`` functions below return."""
    for it in items:
        check(it[0], it[2], it[3], it[1], *(it[4:5]))


def _gen(*key):
    g = torch.Generator()
    seed = 0
    for k in key:  # an explicit polynomial of the case's parameters: the same data on every interpreter
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    g.manual_seed(seed)
    return g


def f32r(v):
    """A Python scalar as the fp32 value the op receives."""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------------------------------------ norms
NORM_EPS = 1e-5
NORM_C = (8, 200, 520, 1032, 2056, 4096)
NORM_N = (1, 3, 6, 1030)


def norm_cases():
    """(rms, res, C, N).  K = ceil(C/512): 8, 200 -> K=1 (lanes partly idle; 8: one lane); 520 -> K=2 and
    1032 -> K=4 by one ragged vector; 2056 -> K=8 by one ragged vector; 4096 -> K=8 full (64 KiB of LDS in the
    backward).  N = 1, 3: one partly empty block; 6: a partly empty last block; 1030: 258 blocks of rows, over
    the backward grid's cap of 256 for C > 1024, so its blocks loop with a ragged last pass; 2054: 514 blocks, over
    the cap of 512 for C <= 1024 (run at C = 8 and 520 only)."""
    out = []
    for rms in (0, 1):
        for res in (0, 1):
            for C in NORM_C:
                for N in ((3, 1030) if C == 4096 else NORM_N + ((2054,) if C in (8, 520) else ())):
                    out.append((rms, res, C, N))
    return out


def norm_inputs(rms, res, C, N):
    g = _gen(1, rms, res, C, N)
    x = (3 + torch.randn(N, C, generator=g)).to(BF16)  # non-zero row mean
    r = torch.randn(N, C, generator=g).to(BF16) if res else None
    if N >= 3:  # one row of all-equal values: variance 0
        x[1] = 2.5
        if res:
            r[1] = 0.5
    w = (1 + 0.2 * torch.randn(C, generator=g)).to(BF16)
    b = None if rms else (0.3 * torch.randn(C, generator=g)).to(BF16)
    dy = torch.randn(N, C, generator=g).to(BF16)
    ds = torch.randn(N, C, generator=g).to(BF16) if res else None
    fill = (1.5 + 0.01 * torch.arange(3 * C, dtype=F32)).reshape(3, C)  # non-zero accumulation targets
    return dict(x=x, r=r, w=w, b=b, dy=dy, ds=ds, fill=fill, rms=rms, eps=NORM_EPS)


def norm_fwd_ref(x, r, w, b, eps, rms):
    """s = bf16(x + r); mean, rstd of s (mean 0 for RMS); y = (s - mean) rstd w + b.

    Units: mean is a sum of mixed signs, 2^-23 mean|s|.  y cancels x_hat w against b, and x_hat carries the
    error of the mean scaled by rstd: 2^-23 (|x_hat w| + |b| + rstd |w| mean|s|)."""
    eps = f32r(eps)
    sx = x.to(F64) + (r.to(F64) if r is not None else 0.0)
    s = sx.to(F32).to(BF16) if r is not None else x
    sq = s.to(F64)
    C = sq.shape[-1]
    mean = torch.zeros(sq.shape[0], dtype=F64) if rms else sq.sum(-1) / C
    d = sq - mean[:, None]
    rstd = ((d * d).sum(-1) / C + eps) ** -0.5
    xh = d * rstd[:, None]
    wd = w.to(F64)
    y = xh * wd + (b.to(F64) if b is not None else 0.0)
    mabs = sq.abs().mean(-1)
    unit_y = E32 * ((xh * wd).abs() + (b.to(F64).abs() if b is not None else 0.0)
                    + (0.0 if rms else 1.0) * (rstd * mabs)[:, None] * wd.abs())
    return dict(s=(sx, 0.0), s_bf16=s, mean=(mean, E32 * mabs), rstd=(rstd, 0.0), y=(y, unit_y))


def norm_bwd_ref(dy, s, w, mean, rstd, ds, rms):
    """dx = rstd (g - mean(g) - x_hat mean(g x_hat)) + ds with g = dy w; dw = sum dy x_hat; db = sum dy.

    ``mean`` / ``rstd`` are the fp32 values the kernel is given.  Units: dx cancels its three terms and the two
    row means are sums of mixed signs, 2^-23 (rstd (|g| + mean|g| + |x_hat| mean|g x_hat|) + |ds|); the column
    sums are sums of mixed signs, 2^-23 sum|term|."""
    sq, g0 = s.to(F64), dy.to(F64)
    C = sq.shape[-1]
    mu = torch.zeros_like(mean, dtype=F64) if rms else mean.to(F64)
    rs = rstd.to(F64)[:, None]
    xh = (sq - mu[:, None]) * rs
    g = g0 * w.to(F64)
    mg = torch.zeros(sq.shape[0], 1, dtype=F64) if rms else g.sum(-1, keepdim=True) / C
    mgx = (g * xh).sum(-1, keepdim=True) / C
    dsd = ds.to(F64) if ds is not None else torch.zeros_like(g)
    dx = rs * (g - mg - xh * mgx) + dsd
    unit_dx = E32 * (rs * (g.abs() + (0.0 if rms else 1.0) * g.abs().mean(-1, keepdim=True)
                           + xh.abs() * (g * xh).abs().mean(-1, keepdim=True)) + dsd.abs())
    return dict(dx=(dx, unit_dx), dw=((g0 * xh).sum(0), E32 * (g0 * xh).abs().sum(0)),
                db=(g0.sum(0), E32 * g0.abs().sum(0)))


def colsum_ref(t, fill=None, out_dtype=F32):
    """fill + column sums of t: 2^-23 sum|t|, plus the output format's ulp of |fill| + |sum| where a fill and
    the sum may cancel."""
    td = t.detach().cpu().to(F64).reshape(-1, t.shape[-1])
    sm = td.sum(0)
    unit = E32 * td.abs().sum(0)
    if fill is None:
        return sm, unit
    fd = fill.to(F64)
    return fd + sm, unit + EPS_OUT[out_dtype] * (fd.abs() + sm.abs())


def norm_model_f32(x, r, w, b, dy, ds, rms, eps, **_):
    """The same ops in plain PyTorch fp32, rounded to the kernel's output types."""
    C = x.shape[-1]
    s = (x.float() + r.float()).to(BF16) if r is not None else x
    sq = s.float()
    if rms:
        mean = torch.zeros(sq.shape[0])
        rstd = torch.rsqrt(sq.pow(2).mean(-1) + eps)
        y = sq * rstd[:, None] * w.float()
    else:
        mean = sq.mean(-1)
        rstd = torch.rsqrt(sq.var(-1, unbiased=False) + eps)
        y = F.layer_norm(sq, (C,), w.float(), b.float(), eps)
    # backward from the reference's fp32 statistics, as the GPU test feeds the kernel
    ref = norm_fwd_ref(x, r, w, b, eps, rms)
    mu, rs = ref["mean"][0].float(), ref["rstd"][0].float()
    xh = (sq - mu[:, None]) * rs[:, None]
    g = dy.float() * w.float()
    mg = 0.0 if rms else g.mean(-1, keepdim=True)
    dx = rs[:, None] * (g - mg - xh * (g * xh).mean(-1, keepdim=True))
    if ds is not None:
        dx = dx + ds.float()
    dx = dx.to(BF16)
    dw, db = (dy.float() * xh).sum(0), dy.float().sum(0)
    return dict(s=s, mean=mean, rstd=rstd, y=y.to(BF16), dx=dx, dw=dw, db=db, xb=dx.float().sum(0))


# ------------------------------------------------------------------------------------------------ activations
GELU_K, GELU_C = math.sqrt(2.0 / math.pi), 0.044715
MAG = (0.0, 2.0 ** -20, 0.5, 1.0, 3.0, 6.0, 10.0, 30.0, 100.0, 1000.0)
BF16_MAX = 3.3895313892515355e38
ACT_NUMEL = (8, 8 * 257, 8 * (256 * 3 + 1))  # one vector; one block + one vector; the `two` pairing with a tail
SWIGLU_SHAPES = tuple((rows, Fd) for rows in (1, 5) for Fd in (8, 136, 688))
ACT_BIAS_SHAPES = ((1, 8), (5, 520), (13, 1032), (300, 3080), (600, 24))
ACT_BIAS_GRID_SHAPES = ((13, 1032), (600, 24))  # these also on the magnitude grid


def mag_grid(numel, with_max=False, shift=0):
    """+-MAG (and +-largest finite bf16) tiled to ``numel`` elements, starting ``shift`` values in."""
    mags = list(MAG) + ([BF16_MAX] if with_max else [])
    vals = torch.tensor([s * m for m in mags for s in (1.0, -1.0)], dtype=F64)
    idx = (torch.arange(numel) + shift) % vals.numel()
    return vals[idx].to(BF16)


def act_inputs(kind, numel, data):
    """``kind`` relu / gelu; ``data`` randn or grid (then dy = 1 so the limits of the derivative show)."""
    g = _gen(2, kind == "gelu", numel, data == "grid")
    if data == "grid":
        x = mag_grid(numel, with_max=kind == "relu")
        dy = torch.ones(numel).to(BF16)
    else:
        x = (2 * torch.randn(numel, generator=g)).to(BF16)
        dy = torch.randn(numel, generator=g).to(BF16)
    return dict(x=x, dy=dy)


def gelu_ref(x):
    """0.5 x (1 + tanh(k (x + c x^3))).  1 + tanh cancels for x < 0: unit 2^-23 0.5 |x| (1 + |tanh|)."""
    xd = x.to(F64)
    t = torch.tanh(GELU_K * (xd + GELU_C * xd ** 3))
    return 0.5 * xd * (1 + t), E32 * 0.5 * xd.abs() * (1 + t.abs())


def gelu_bwd_ref(dy, x):
    """dy (0.5 (1 + t) + 0.25 q (1 - t^2)), t = tanh u, q = x 2k (1 + 3 c x^2) (= s + q s (1 - s) with
    s = sigmoid(2u)).  1 + t cancels for x < 0 and 1 - t^2 on both sides: unit |dy| 2^-23 (0.5 (1 + |t|) +
    0.25 |q| (1 + t^2)), plus a flushed exponential: |dy| 2^-126 (1 + |q|)."""
    xd, d = x.to(F64), dy.to(F64)
    s = torch.sigmoid(2 * GELU_K * (xd + GELU_C * xd ** 3))
    t = torch.tanh(GELU_K * (xd + GELU_C * xd ** 3))
    q = xd * 2 * GELU_K * (1 + 3 * GELU_C * xd * xd)
    unit = d.abs() * (E32 * (0.5 * (1 + t.abs()) + 0.25 * q.abs() * (1 + t * t)) + FLUSH * (1 + q.abs()))
    return d * (s + q * s * (1 - s)), unit


def relu_ref(x):
    xd = x.to(F64)
    return torch.where(xd > 0, xd, torch.zeros_like(xd)), 0.0


def relu_bwd_ref(dy, y):
    """ReLU backward takes the OUTPUT y: dy where y > 0, else 0."""
    return torch.where(y.to(F64) > 0, dy.to(F64), torch.zeros(y.shape, dtype=F64)), 0.0


def swiglu_inputs(rows, Fd, data):
    g = _gen(3, rows, Fd, data == "grid")
    if data == "grid":
        gate = mag_grid(rows * Fd).reshape(rows, Fd)
        up = mag_grid(rows * Fd, shift=7).reshape(rows, Fd)
        up = torch.where(up == 0, torch.ones_like(up), up)
        dy = torch.ones(rows, Fd).to(BF16)
    else:
        gate = (2 * torch.randn(rows, Fd, generator=g)).to(BF16)
        up = torch.randn(rows, Fd, generator=g).to(BF16)
        dy = torch.randn(rows, Fd, generator=g).to(BF16)
    return dict(gu=torch.cat([gate, up], -1).contiguous(), dy=dy)


def swiglu_ref(gu):
    """silu(gate) up.  No cancellation; a flushed sigmoid: unit 2^-126 |gate up|."""
    Fd = gu.shape[-1] // 2
    g, u = gu[..., :Fd].to(F64), gu[..., Fd:].to(F64)
    return g * torch.sigmoid(g) * u, FLUSH * (g * u).abs()


def swiglu_bwd_ref(dy, gu):
    """dgate = dy up s (1 + g (1 - s)), dup = dy g s, s = sigmoid(g).  1 + g (1 - s) cancels for g < 0 and 1 - s
    for g > 0: unit |dy up| (2^-23 s + 2^-126) (1 + |g|); dup: 2^-126 |dy g|."""
    Fd = gu.shape[-1] // 2
    g, u, d = gu[..., :Fd].to(F64), gu[..., Fd:].to(F64), dy.to(F64)
    s = torch.sigmoid(g)
    ref = torch.cat([d * u * s * (1 + g * (1 - s)), d * g * s], -1)
    unit = torch.cat([(d * u).abs() * (E32 * s + FLUSH) * (1 + g.abs()), FLUSH * (d * g).abs()], -1)
    return ref, unit


def act_bias_inputs(kind, N, C, data="randn"):
    """``data`` grid: the magnitude grid over the whole [N, C] matrix with dy = 1, so that each column sums
    saturated derivatives (0 or 1) beside the ones in between."""
    g = _gen(4, kind == "gelu", N, C, data == "grid")
    if data == "grid":
        x = mag_grid(N * C, with_max=kind == "relu", shift=3).reshape(N, C)
        dy = torch.ones(N, C).to(BF16)
    else:
        x = (2 * torch.randn(N, C, generator=g)).to(BF16)
        dy = torch.randn(N, C, generator=g).to(BF16)
    if kind == "relu":
        x = torch.where(x > 0, x, torch.zeros_like(x))  # the forward's output
    fill = 1.5 + 0.01 * torch.arange(C, dtype=F32)
    return dict(x=x, dy=dy, fill=fill)


# ------------------------------------------------------------------------------------------------ cross-entropy
CE_V = (8, 4096, 4104, 8200, 16392, 32776, 53256, 65544, 131072)
CE_N = 6
IGNORE = -100


def ce_inputs(V, all_ignored=False):
    """CH = ceil(V/8/512): 8, 4096 -> 1 (4096 full); 4104 -> 2, 8200 -> 4, 16392 -> 8, 32776 -> 13, 53256 -> 16,
    65544 -> 32, each by one ragged vector; 131072 -> 32 full: the largest vocabulary the op accepts
    (cross_entropy_max_vocab(); the GPU file asserts that they agree)."""
    g = _gen(5, V)
    x = 4 * torch.randn(CE_N, V, generator=g)
    sweep = 4096 if V > 4096 else (4095 if V == 4096 else V // 2)  # just across / at the end of the first sweep
    t = torch.tensor([0, 7, 8 if V > 8 else 3, V - 1, sweep, IGNORE])
    x[1] = -80.0
    x[1, 7] = 80.0            # one spike at the target: softmax - onehot cancels to ~0 (any error of the row's
                              # sum or of the maximum's own exponent, 2^0, shows here in full)
    x[2] = 1.5                # all equal
    x[3, V - 3] = 30.0        # the row maximum in the last vector
    inf_mask = (torch.arange(V) % 5 == 1) & (torch.arange(V) != sweep)
    x[4, inf_mask] = -math.inf  # masked vocabulary entries, never the whole row
    if all_ignored:
        t = torch.full((CE_N,), IGNORE)
    return dict(logits=x.to(BF16), targets=t)


def ce_ref(logits, targets, inv_n=None, ignore_index=IGNORE):
    """loss = logsumexp(x) - x_t; dlogits = (softmax(x) - onehot(t)) inv_n; ignored rows give 0.

    Units: the loss cancels m + log(sum) against x_t, and the sum carries each exponent's rounding:
    2^-23 (|m| + |log sum| + |x_t| + sum_i p_i (1 + |x_i - m| log2 e)).  dlogits cancels p_t against 1 at the
    target and carries the exponent's rounding elsewhere: 2^-23 inv_n (p (2 + |x - m| log2 e) + onehot), plus a
    flushed exponential, 2^-126 inv_n."""
    x = logits.to(F64)
    N, V = x.shape
    valid = targets != ignore_index
    if inv_n is None:
        inv_n = 1.0 / max(int(valid.sum()), 1)
    m = x.max(-1, keepdim=True).values
    e = torch.exp(x - m)
    ssum = e.sum(-1, keepdim=True)
    p = e / ssum
    tc = torch.where(valid, targets, torch.zeros_like(targets))
    xt = x.gather(1, tc[:, None])
    vd = valid[:, None].to(F64)
    loss = ((m + ssum.log() - xt) * vd)[:, 0]
    onehot = torch.zeros_like(x).scatter_(1, tc[:, None], 1.0)
    dl = (p - onehot) * inv_n * vd
    dist = torch.where(p > 0, (x - m).abs() * math.log2(math.e), torch.zeros_like(x))
    unit_loss = E32 * (m.abs() + ssum.log().abs() + xt.abs() + (p * (1 + dist)).sum(-1, keepdim=True))[:, 0] \
        * vd[:, 0]
    unit_dl = (E32 * (p * (2 + dist) + onehot) + FLUSH) * inv_n * vd
    return dict(loss=(loss, unit_loss), dlogits=(dl, unit_dl))


def ce_model_f32(logits, targets, inv_n=None):
    x = logits.float()
    valid = targets != IGNORE
    if inv_n is None:
        inv_n = 1.0 / max(int(valid.sum()), 1)
    lp = torch.log_softmax(x, -1)
    tc = torch.where(valid, targets, torch.zeros_like(targets))
    loss = -lp.gather(1, tc[:, None])[:, 0] * valid.float()
    onehot = torch.zeros_like(x).scatter_(1, tc[:, None], 1.0)
    dl = (lp.exp() - onehot) * torch.tensor(inv_n, dtype=F32) * valid[:, None].float()
    return dict(loss=loss, dlogits=dl.to(BF16))


# ------------------------------------------------------------------------------------------------ AdamW
ADAMW_N = (8, 64, 8 * 257, 64 * 100 + 8 * 3)
ADAMW_HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)
ADAMW_MASKS = ("none", "ones", "pattern", "long")
ADAMW_VARIANTS = ("base", "noparam", "hyper", "step1", "step1000")


def adamw_cases():
    """(n, grad dtype, mask, variant).  n = 8: one vector; 64: one decay block; 8*257: a second workgroup and a
    partly covered last decay block; 64*100 + 24: 101 blocks, the last partial.  Variants: ``base`` is step 2 with
    grad_scale 0.5 and a scale tensor of 0.25; ``noparam`` passes an empty param; ``hyper`` device scalars that
    differ from the arguments; ``step1`` / ``step1000`` without a scale tensor."""
    out = [(n, gd, mk, "base") for n in ADAMW_N for gd in ("bf16", "f32") for mk in ADAMW_MASKS]
    out += [(ADAMW_N[3], gd, "pattern", v) for gd in ("bf16", "f32")
            for v in ADAMW_VARIANTS[1:]]
    return out


def adamw_inputs(n, gd, mask, variant):
    g = _gen(6, n, gd == "f32", ADAMW_MASKS.index(mask), ADAMW_VARIANTS.index(variant))
    master = torch.randn(n, generator=g)
    m = 0.1 * torch.randn(n, generator=g)
    v = (0.1 * torch.randn(n, generator=g)) ** 2
    grad = torch.randn(n, generator=g)
    grad = grad if gd == "f32" else grad.to(BF16)
    nb = (n + 63) // 64
    if mask == "none":
        wd_mask = None
    elif mask == "ones":
        wd_mask = torch.ones(nb, dtype=torch.uint8)
    else:  # alternating, then irregular, non-zero bytes of several values; "long": more bytes than blocks
        k = torch.arange(nb + (37 if mask == "long" else 0))
        wd_mask = (((k % 2 == 0) ^ (k % 7 == 3)).to(torch.uint8) * (1 + (k % 3) * 100).to(torch.uint8))
    step = {"step1": 1, "step1000": 1000, "hyper": 5}.get(variant, 2)
    scale = None if variant in ("step1", "step1000") else 0.25
    hyper = torch.tensor([3e-3, 1.7, 1.3, 99.0], dtype=F32) if variant == "hyper" else None
    return dict(master=master, m=m, v=v, grad=grad, wd_mask=wd_mask, step=step, grad_scale=0.5, scale=scale,
                hyper=hyper, with_param=variant != "noparam", **ADAMW_HP)


def adamw_ref(master, m, v, grad, lr, b1, b2, eps, wd, step, grad_scale=1.0, scale=None, wd_mask=None,
              hyper=None, **_):
    """The header of adamw.hip: g' = g grad_scale scale; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2;
    p = p (1 - lr wd [block mask]) - lr / bc1 m / (sqrt(v) / sqrt(bc2) + eps), the mask one byte per 64 elements.
    ``hyper`` = [lr, 1/bc1, 1/sqrt(bc2)] replaces the scalars.  All scalars are the fp32 values the op receives.

    Units: m cancels its two terms, 2^-23 (|b1 m| + |(1 - b1) g'|).  The update p_new - p_old cancels the rounded
    p_new against p: 2^-23 |p|; it carries m's unit through step / denom, and the fp32 bias corrections cancel
    1 - b^t: |adam term| 2^-23 (b1^t / bc1 + b2^t / (2 bc2)) (not with ``hyper``)."""
    lr, b1, b2, eps, wd, gs = (f32r(a) for a in (lr, b1, b2, eps, wd, grad_scale))
    if hyper is not None:
        lr, inv_bc1, inv_sqrt_bc2 = (float(h) for h in hyper[:3])
        bc_unit = 0.0
    else:
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        inv_bc1, inv_sqrt_bc2 = 1 / bc1, 1 / math.sqrt(bc2)
        bc_unit = E32 * (b1 ** step / bc1 + 0.5 * b2 ** step / bc2)
    n = master.numel()
    gg = grad.to(F64) * (gs * (f32r(scale) if scale is not None else 1.0))
    p, m0, v0 = master.to(F64), m.to(F64), v.to(F64)
    m1 = b1 * m0 + (1 - b1) * gg
    v1 = b2 * v0 + (1 - b2) * gg * gg
    on = torch.ones(n, dtype=F64) if wd_mask is None else \
        (wd_mask[torch.arange(n) // 64] != 0).to(F64)
    denom = v1.sqrt() * inv_sqrt_bc2 + eps
    adam = lr * inv_bc1 * m1 / denom
    upd = p * (-(lr * wd) * on) - adam
    unit_m = E32 * ((b1 * m0).abs() + ((1 - b1) * gg).abs())
    unit_upd = E32 * p.abs() + lr * inv_bc1 * unit_m / denom + adam.abs() * bc_unit
    return dict(update=(upd, unit_upd), m=(m1, unit_m), v=(v1, 0.0), master=p + upd)


def adamw_model_f32(master, m, v, grad, lr, b1, b2, eps, wd, step, grad_scale=1.0, scale=None, wd_mask=None,
                    hyper=None, **_):
    t = lambda a: torch.tensor(a, dtype=F32)  # noqa: E731
    lr_, b1_, b2_, eps_, wd_ = t(lr), t(b1), t(b2), t(eps), t(wd)
    if hyper is not None:
        lr_, inv_bc1, inv_sqrt_bc2 = hyper[0], hyper[1], hyper[2]
    else:
        inv_bc1 = 1 / (1 - b1_ ** step)
        inv_sqrt_bc2 = 1 / torch.sqrt(1 - b2_ ** step)
    n = master.numel()
    gg = grad.float() * (t(grad_scale) * (t(scale) if scale is not None else t(1.0)))
    m1 = b1_ * m + (1 - b1_) * gg
    v1 = b2_ * v + (1 - b2_) * gg * gg
    on = torch.ones(n, dtype=torch.bool) if wd_mask is None else wd_mask[torch.arange(n) // 64] != 0
    decay = torch.where(on, 1 - lr_ * wd_, t(1.0))
    p1 = master * decay - lr_ * inv_bc1 * m1 / (v1.sqrt() * inv_sqrt_bc2 + eps_)
    return dict(master=p1, m=m1, v=v1)


# ------------------------------------------------------------------------------------------------ gradient norm
SUMSQ_N = (8, 8 * 255, 8 * (256 * 1024 * 2 + 3))  # one vector; a partly idle block; the capped grid loops 2x + 3
SWEEP = 8 * 256 * 1024  # elements one pass of the capped grid (1024 blocks of 256 threads, 8 each) covers


def sumsq_inputs(n, dtype):
    """Small values in the first sweep of the capped grid, large ones after it: a dropped sweep changes the
    result by orders of magnitude."""
    g = _gen(7, n, dtype == F32)
    x = 1e-2 * torch.randn(n, generator=g)
    if n > SWEEP:
        x[SWEEP:] = 50 * torch.randn(n - SWEEP, generator=g)
    return x.to(dtype)


def sumsq_ref(x):
    """Sum of squares: positive terms, no cancellation."""
    return (x.to(F64) ** 2).sum(), 0.0


def grad_norm_clip_ref(x, grad_scale, max_norm):
    """[norm grad_scale, min(max_norm / (norm grad_scale + 1e-6), 1)]; no cancellation."""
    nrm = math.sqrt(float((x.to(F64) ** 2).sum())) * f32r(grad_scale)
    return torch.tensor([nrm, min(f32r(max_norm) / (nrm + f32r(1e-6)), 1.0)], dtype=F64), 0.0


# ------------------------------------------------------------------------------------------------ what is compared
# Each ``*_checks`` takes a case's inputs and an op's outputs (the HIP kernel's, or the fp32 model's) and returns
# the (op, name, out, (ref64, unit)[, fmt]) comparisons, so that the CPU calibration and the GPU tests apply the
# same references and units.
def with_fill(ref_unit, fill, dtype):
    """An accumulated output: fill + ref; the fill and the sum may cancel at the output format's precision."""
    ref, unit = ref_unit
    fd = fill.to(F64)
    return fd + ref, unit + EPS_OUT[dtype] * (fd.abs() + ref.abs())


def norm_stats32(inp):
    """The reference forward, and the fp32 mean / rstd and bf16 s that the backward is given."""
    fw = norm_fwd_ref(inp["x"], inp["r"], inp["w"], inp["b"], inp["eps"], inp["rms"])
    return fw, fw["mean"][0].to(F32), fw["rstd"][0].to(F32)


def norm_checks(inp, out):
    """``out``: s (with a residual), mean, rstd, y; dx, dw, db (pure backward, bf16); dx_acc, dw_acc, db_acc,
    xb_acc (fp32 targets pre-filled with inp['fill'] rows 0, 1, 2)."""
    fw, mean32, rstd32 = norm_stats32(inp)
    bw = norm_bwd_ref(inp["dy"], fw["s_bf16"], inp["w"], mean32, rstd32, inp["ds"], inp["rms"])
    fill = inp["fill"]
    items = [("norm_stats", "rstd", out["rstd"], fw["rstd"]), ("norm_y", "y", out["y"], fw["y"]),
             ("norm_dx", "dx", out["dx"], bw["dx"]), ("norm_dx", "dx_acc", out["dx_acc"], bw["dx"]),
             ("norm_dwdb", "dw", out["dw"], bw["dw"]),
             ("norm_dwdb", "dw_acc", out["dw_acc"], with_fill(bw["dw"], fill[0], F32)),
             ("norm_dwdb", "xb_acc", out["xb_acc"], with_fill(colsum_ref(out["dx_acc"]), fill[2], F32))]
    if inp["r"] is not None:
        items.append(("exact", "s", out["s"], (fw["s_bf16"].to(F64), 0.0)))
    if not inp["rms"]:
        items += [("norm_stats", "mean", out["mean"], fw["mean"]), ("norm_dwdb", "db", out["db"], bw["db"]),
                  ("norm_dwdb", "db_acc", out["db_acc"], with_fill(bw["db"], fill[1], F32))]
    return items


def norm_model_outputs(inp):
    m = norm_model_f32(**inp)
    fill = inp["fill"]
    return dict(s=m["s"], mean=m["mean"], rstd=m["rstd"], y=m["y"], dx=m["dx"], dx_acc=m["dx"],
                dw=m["dw"].to(BF16), db=m["db"].to(BF16), dw_acc=fill[0] + m["dw"], db_acc=fill[1] + m["db"],
                xb_acc=fill[2] + m["xb"])


def act_checks(kind, inp, out):
    """``out``: y = act_fwd(x); dx = act_bwd(dy, x) (GELU) or act_bwd(dy, relu(x)) (ReLU takes the output)."""
    if kind == "relu":
        return [("exact", "y", out["y"], relu_ref(inp["x"])),
                ("exact", "dx", out["dx"], relu_bwd_ref(inp["dy"], relu_of(inp["x"])))]
    return [("gelu_fwd", "y", out["y"], gelu_ref(inp["x"])),
            ("gelu_bwd", "dx", out["dx"], gelu_bwd_ref(inp["dy"], inp["x"]))]


def relu_of(x):
    return torch.where(x > 0, x, torch.zeros_like(x))


def gelu_model_f32(x, dy):
    xf = x.float().requires_grad_()
    y = F.gelu(xf, approximate="tanh")
    (dx,) = torch.autograd.grad(y, xf, dy.float())
    return dict(y=y.detach().to(BF16), dx=dx.to(BF16))


def relu_model_f32(x, dy):
    y = relu_of(x)
    return dict(y=y, dx=torch.where(y > 0, dy, torch.zeros_like(dy)))


def swiglu_checks(inp, out):
    return [("swiglu_fwd", "y", out["y"], swiglu_ref(inp["gu"])),
            ("swiglu_bwd", "dgu", out["dgu"], swiglu_bwd_ref(inp["dy"], inp["gu"]))]


def swiglu_model_f32(gu, dy):
    Fd = gu.shape[-1] // 2
    gf = gu.float().requires_grad_()
    y = F.silu(gf[..., :Fd]) * gf[..., Fd:]
    (dgu,) = torch.autograd.grad(y, gf, dy.float())
    return dict(y=y.detach().to(BF16), dgu=dgu.to(BF16))


def act_bias_checks(kind, inp, out, acc_dtype):
    """``out``: dx and bias (the accumulation target, pre-filled with inp['fill'] in ``acc_dtype``).  The bias is
    compared with fill + the fp64 column sums of the op's own bf16 dx (returned here), and by the caller with the
    reference's sums under the bf16 bound of dx (``act_bias_ref_sums``)."""
    dx_ref = relu_bwd_ref(inp["dy"], inp["x"]) if kind == "relu" else gelu_bwd_ref(inp["dy"], inp["x"])
    fill = inp["fill"].to(acc_dtype)
    return [("exact" if kind == "relu" else "gelu_bwd", "dx", out["dx"], dx_ref),
            ("colsum", "bias", out["bias"], colsum_ref(out["dx"], fill, acc_dtype))]


def act_bias_ref_sums(kind, inp, acc_dtype):
    """fill + column sums of the reference dx, and the floor that dx's own per-element bound adds to them."""
    ref, unit = relu_bwd_ref(inp["dy"], inp["x"]) if kind == "relu" else gelu_bwd_ref(inp["dy"], inp["x"])
    u_dx = BUDGET["exact" if kind == "relu" else "gelu_bwd"][1]
    slack = u_dx * ((ref.abs() * EPS_OUT[BF16]).clamp_min(DENORM[BF16]) + unit).sum(0)
    fill = inp["fill"].to(acc_dtype)
    sm, sunit = colsum_ref(ref, fill, acc_dtype)
    return sm, BUDGET["colsum"][1] * sunit + slack


def act_bias_model_f32(kind, inp, acc_dtype):
    m = (relu_model_f32 if kind == "relu" else gelu_model_f32)(inp["x"], inp["dy"])
    fill = inp["fill"].to(acc_dtype)
    return dict(dx=m["dx"], bias=(fill.float() + m["dx"].float().sum(0)).to(acc_dtype))


def ce_checks(inp, out, inv_n=None):
    ref = ce_ref(inp["logits"], inp["targets"], inv_n)
    return [("ce_loss", "loss", out["loss"], ref["loss"]), ("ce_dlogits", "dlogits", out["dlogits"], ref["dlogits"])]


def adamw_checks(inp, out):
    """``out``: master, m, v after the step (fp32).  The update is master_after - master_before, in fp64."""
    ref = adamw_ref(**inp)
    upd = out["master"].detach().cpu().to(F64) - inp["master"].to(F64)
    return [("adamw", "update", upd, ref["update"], F32), ("adamw", "m", out["m"], ref["m"]),
            ("adamw", "v", out["v"], ref["v"])]


def adamw_model_outputs(inp):
    return adamw_model_f32(**inp)
