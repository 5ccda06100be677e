"""fp64 references, case builders and budgets for the QK-norm kernels (csrc/qk_norm.hip: ``qk_norm_rope`` and
``qk_norm_bwd_``), by the method of ``_streaming_refs.py`` (whose bound helpers are used here).

Not collected by pytest.  ``test_qk_norm_refs.py`` (CPU) checks the references against autograd in double
precision and calibrates the budgets below; ``test_qk_norm_gpu.py`` runs the HIP kernels on the same cases
against the same bounds.

The bound.  Every element must satisfy ``|out - ref| <= ulps * ulp(ref) + abs_floor`` with ``abs_floor = ulps *
unit`` (``_streaming_refs.assert_close_ulps``); the units are documented at each reference.

Budgets.  ``measured`` is the smallest integer budget at which a plain PyTorch fp32 (CPU) evaluation of the op,
rounded to the kernel's output type, passes on all cases; ``budget`` is twice that (a different summation order;
a hardware rsqrt at about 1 fp32 ulp).  Filled from ``pytest tests/test_qk_norm_refs.py`` (which fails when a row
is stale); nothing here was tuned against kernel output.

    op          measured  budget   outputs
    ----------  --------  ------   ---------------------------------------------------
    qkn_y              1       2   qk (bf16): normalised (and rotated) q / k heads
    qkn_rstd           2       4   rstd (fp32)
    qkn_dx             1       2   dx (bf16), in place on the q / k columns of dqkv
    qkn_dw             1       2   dwq, dwk (bf16 fresh / fp32 accumulated)

Cases (``cases()``): D in {32, 64, 128} x (H, Hkv) in {(4, 4), (4, 2), (8, 1)} x (B, T) in {(2, 5), (1, 67),
(3, 128)} x {no RoPE, RoPE at pos_offset 0, RoPE at pos_offset 9}; every case has two all-zero heads (r =
rsqrt(eps)) and gains with a zero and negative entries; inputs scaled by 2^-40 and by 2^20 at (1, 67) with RoPE
at offset 9 for every D and head layout.  ``BIG`` is the backward case of ``BIG_ROWS`` >= 8 x the rows one pass
of the backward's capped grid covers at (H, Hkv, D) = (2, 1, 32), so that every workgroup accumulates its gain
partials over 8-9 iterations.
"""
from __future__ import annotations

import torch

from _streaming_refs import BF16, E32, F32, F64, _gen, f32r, with_fill  # noqa: F401

# op -> (measured, budget); see the table above
BUDGET = {
    "qkn_y": (1, 2),
    "qkn_rstd": (2, 4),
    "qkn_dx": (1, 2),
    "qkn_dw": (1, 2),
}

EPS = 1e-5
THETA = 10000.0
HEAD_DIMS = (32, 64, 128)
HEAD_LAYOUTS = ((4, 4), (4, 2), (8, 1))
BATCH_SEQ = ((2, 5), (1, 67), (3, 128))
ROPE_MODES = ((0, 0), (1, 0), (1, 9))  # (rope, pos_offset)
SCALES = (1.0, 2.0 ** -40, 2.0 ** 20)

# the backward's grid is capped at 512 workgroups of 256 threads, D/16 threads per head (csrc/qk_norm.hip)
BWD_PASS_THREADS = 512 * 256
BIG = dict(D=32, H=2, Hkv=1, B=1, rope=0, pos=0, scale=1.0)
BIG_ROWS = 8 * (BWD_PASS_THREADS // (2 * 3) + 1)  # 2 threads per head, 3 normalised heads per row
BIG["T"] = BIG_ROWS


def cases():
    """dicts of D, H, Hkv, B, T, rope, pos, scale (without the big backward case)."""
    out = []
    for D in HEAD_DIMS:
        for H, Hkv in HEAD_LAYOUTS:
            for B, T in BATCH_SEQ:
                for rope, pos in ROPE_MODES:
                    out.append(dict(D=D, H=H, Hkv=Hkv, B=B, T=T, rope=rope, pos=pos, scale=1.0))
            for scale in SCALES[1:]:
                out.append(dict(D=D, H=H, Hkv=Hkv, B=1, T=67, rope=1, pos=9, scale=scale))
    return out


def case_id(c):
    s = {1.0: "", 2.0 ** -40: "-tiny", 2.0 ** 20: "-huge"}[c["scale"]]
    return f"D{c['D']}-h{c['H']}x{c['Hkv']}-{c['B']}x{c['T']}-" + (f"rope{c['pos']}" if c["rope"] else "norope") + s


def rope_tables(n_pos, D):
    """fp32 cos / sin [n_pos, D/2] (rotate-half convention, as ops.rope_cache)."""
    inv = THETA ** (-torch.arange(0, D, 2, dtype=F64) / D)
    ang = torch.arange(n_pos, dtype=F64)[:, None] * inv[None, :]
    return ang.cos().to(F32), ang.sin().to(F32)


def inputs(D, H, Hkv, B, T, rope, pos, scale):
    g = _gen(11, D, H, Hkv, B, T, rope, pos, int(torch.tensor(scale).log2()))
    rows, W = B * T, (H + 2 * Hkv) * D
    qkv = (scale * torch.randn(rows, W, generator=g)).to(BF16)
    r1 = min(1, rows - 1)
    qkv[r1, D:2 * D] = 0                       # an all-zero q head
    qkv[0, (H + Hkv - 1) * D:(H + Hkv) * D] = 0  # an all-zero k head
    wq = (1 + 0.2 * torch.randn(D, generator=g)).to(BF16)
    wk = (1 + 0.2 * torch.randn(D, generator=g)).to(BF16)
    for w in (wq, wk):  # zeros and negative entries, in both halves of the head
        w[0], w[3], w[D // 2 + 1], w[D - 1] = 0.0, -1.5, 0.0, -0.25
    dqkv = torch.randn(rows, W, generator=g).to(BF16)
    cos, sin = rope_tables(T + pos, D) if rope else (None, None)
    fill = (1.5 + 0.01 * torch.arange(2 * D, dtype=F32)).reshape(2, D)  # non-zero accumulation targets
    return dict(qkv=qkv, wq=wq, wk=wk, dqkv=dqkv, cos=cos, sin=sin, fill=fill, D=D, H=H, Hkv=Hkv, T=T, pos=pos,
                eps=EPS)


def _heads(t, H, Hkv, D, dtype):
    """The q and k heads of packed rows [rows, (H + 2 Hkv) D] -> [rows, H + Hkv, D]."""
    return t[:, : (H + Hkv) * D].to(dtype).reshape(t.shape[0], H + Hkv, D)


def _gains(wq, wk, H, Hkv, dtype):
    return torch.cat([wq.to(dtype).expand(H, -1), wk.to(dtype).expand(Hkv, -1)], 0)  # [H + Hkv, D]


def _rot(y, cos, sin, T, pos):
    """Rotate-half of y [rows, NH, D]: row r at position r % T + pos.  Returns the rotated heads and |terms|."""
    half = y.shape[-1] // 2
    t = torch.arange(y.shape[0]) % T + pos
    c, s = cos[t].to(y.dtype)[:, None, :], sin[t].to(y.dtype)[:, None, :]
    a, b = y[..., :half], y[..., half:]
    out = torch.cat([a * c - b * s, b * c + a * s], -1)
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
    return out, mag


def fwd_ref(qkv, wq, wk, cos, sin, D, H, Hkv, T, pos, eps, **_):
    """r = (mean(x^2) + eps)^-1/2; y = x r gamma, then rotated.

    Units: the mean of squares sums positive terms (none for rstd); the rotation cancels its two products:
    2^-23 (|a c| + |b s|); without tables 2^-23 |y|."""
    x = _heads(qkv, H, Hkv, D, F64)
    rstd = ((x * x).sum(-1) / D + f32r(eps)) ** -0.5
    y = x * rstd[..., None] * _gains(wq, wk, H, Hkv, F64)
    mag = y.abs()
    if cos is not None:
        y, mag = _rot(y, cos, sin, T, pos)
    return dict(y=(y.reshape(x.shape[0], -1), E32 * mag.reshape(x.shape[0], -1)), rstd=(rstd, 0.0))


def bwd_ref(dqkv, qkv, rstd, wq, wk, D, H, Hkv, **_):
    """x_hat = x r, g = dy gamma, c = mean(g x_hat), dx = r (g - x_hat c); dgamma = sum over rows and heads of
    dy x_hat.  ``rstd`` is the fp32 tensor the kernel is given.

    Units (as norm_bwd_ref): dx cancels its two terms and the row mean sums mixed signs, 2^-23 r (|g| + |x_hat|
    mean|g x_hat|); the gain gradients are sums of mixed signs, 2^-23 sum|dy x_hat|."""
    x, dy = _heads(qkv, H, Hkv, D, F64), _heads(dqkv, H, Hkv, D, F64)
    rs = rstd.to(F64).reshape(x.shape[0], H + Hkv, 1)
    xh = x * rs
    g = dy * _gains(wq, wk, H, Hkv, F64)
    gx = g * xh
    dx = rs * (g - xh * gx.mean(-1, keepdim=True))
    unit_dx = E32 * rs * (g.abs() + xh.abs() * gx.abs().mean(-1, keepdim=True))
    t = dy * xh
    n = x.shape[0]
    return dict(dx=(dx.reshape(n, -1), unit_dx.reshape(n, -1)),
                dwq=(t[:, :H].sum((0, 1)), E32 * t[:, :H].abs().sum((0, 1))),
                dwk=(t[:, H:].sum((0, 1)), E32 * t[:, H:].abs().sum((0, 1))))


def rstd32(inp):
    """The fp32 rstd [rows, H + Hkv] the backward is given: the reference's, rounded."""
    return fwd_ref(**inp)["rstd"][0].to(F32)


def model_f32(inp, backward=True, forward=True):
    """The same ops in plain PyTorch fp32, rounded to the kernels' output types."""
    D, H, Hkv = inp["D"], inp["H"], inp["Hkv"]
    x = _heads(inp["qkv"], H, Hkv, D, F32)
    gam = _gains(inp["wq"], inp["wk"], H, Hkv, F32)
    n = x.shape[0]
    out = {}
    if forward:
        r = torch.rsqrt(x.pow(2).mean(-1) + inp["eps"])
        y = x * r[..., None] * gam
        if inp["cos"] is not None:
            y = _rot(y, inp["cos"], inp["sin"], inp["T"], inp["pos"])[0]
        out.update(y=y.reshape(n, -1).to(BF16), rstd=r)
    if backward:
        rs = rstd32(inp)[..., None]
        dy = _heads(inp["dqkv"], H, Hkv, D, F32)
        xh = x * rs
        g = dy * gam
        dx = rs * (g - xh * (g * xh).mean(-1, keepdim=True))
        t = dy * xh
        dwq, dwk = t[:, :H].sum((0, 1)), t[:, H:].sum((0, 1))
        fill = inp["fill"]
        out.update(dx=dx.reshape(n, -1).to(BF16), dwq=dwq.to(BF16), dwk=dwk.to(BF16), dwq_acc=fill[0] + dwq,
                   dwk_acc=fill[1] + dwk)
    return out


def fwd_checks(inp, out):
    """``out``: y (bf16 [rows, (H + Hkv) D]) and rstd (fp32 [rows, H + Hkv])."""
    ref = fwd_ref(**inp)
    return [("qkn_y", "y", out["y"], ref["y"]), ("qkn_rstd", "rstd", out["rstd"], ref["rstd"])]


def bwd_checks(inp, out):
    """``out``: dx (bf16, the q / k columns of dqkv after the op), dwq / dwk (bf16, fresh) and dwq_acc / dwk_acc
    (fp32 targets pre-filled with inp['fill'] rows 0, 1)."""
    ref = bwd_ref(inp["dqkv"], inp["qkv"], rstd32(inp), inp["wq"], inp["wk"], inp["D"], inp["H"], inp["Hkv"])
    fill = inp["fill"]
    return [("qkn_dx", "dx", out["dx"], ref["dx"]),
            ("qkn_dw", "dwq", out["dwq"], ref["dwq"]), ("qkn_dw", "dwk", out["dwk"], ref["dwk"]),
            ("qkn_dw", "dwq_acc", out["dwq_acc"], with_fill(ref["dwq"], fill[0], F32)),
            ("qkn_dw", "dwk_acc", out["dwk_acc"], with_fill(ref["dwk"], fill[1], F32))]


def check_all(items):
    """(op, name, out, (ref64, unit)) comparisons under the ops' budgets."""
    from _streaming_refs import assert_close_ulps
    for op, name, out, (ref, unit) in items:
        u = BUDGET[op][1]
        assert_close_ulps(out, ref, u, u * torch.as_tensor(unit, dtype=F64), what=f"{op}/{name}")
