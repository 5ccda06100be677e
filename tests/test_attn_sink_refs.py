"""CPU checks of ``_attn_sink_refs``: the fp64 references against independent PyTorch double-precision paths (autograd
through ``softmax`` over the scores with the sink as one more column, ``gradcheck``, the extra-zero-key identity), the
choice of the sink values, the calibration of the budgets against the fp32 / bf16 model of the documented roundings on
the cases ``test_attn_sinks_gpu.py`` runs, and the proof that a kernel which drops, scales or misplaces the sink fails
the per-element checks in every family of cases."""
import math

import pytest
import torch

import _attention_refs as A
import _attn_sink_refs as K
from pretraining_llm_amd.ops import reference as ref

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32


def _same(a, b, what, tol=1e-12):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert float((a - b).abs().max()) <= tol * scale, f"{what}: {float((a - b).abs().max())} vs scale {scale}"


def _torch_sink_attention(q, k, v, sinks, scale, vis):
    """softmax over [scores | sink] on fp64 leaves [B, L, H, D] / [H], the sink's column dropped before the PV
    product; PyTorch's own ops throughout."""
    Hq, Hkv = q.shape[2], k.shape[2]
    kk, vv = k.repeat_interleave(Hq // Hkv, dim=2), v.repeat_interleave(Hq // Hkv, dim=2)
    s = (torch.einsum("bthd,bshd->bhts", q, kk) * scale).masked_fill(~vis, -math.inf)
    full = torch.cat([s, sinks.view(1, Hq, 1, 1).expand(*s.shape[:3], 1)], -1)
    o = torch.einsum("bhts,bshd->bthd", torch.softmax(full, -1)[..., :-1], vv)
    return o, torch.logsumexp(full, -1)


REF_CASES = [("randn", 33, 33, 32, 2), ("randn", 40, 600, 64, 1), ("extreme", 129, 129, 128, 4),
             ("randn", 1, 65, 32, 1)]


# ------------------------------------------------------------------------------------ references vs PyTorch fp64
@pytest.mark.parametrize("case", REF_CASES, ids=str)
def test_refs_match_torch_double(case):
    inp, fw = K.fwd_case(case)
    T, S = case[1], case[2]
    q, k, v = (inp[n].to(F64).requires_grad_() for n in ("q", "k", "v"))
    sk = inp["sinks"].to(F64).requires_grad_()
    o, lse = _torch_sink_attention(q, k, v, sk, inp["scale"], K.visible(T, S, True))
    _same(fw["o"][0], o.detach(), "o")
    _same(fw["lse"][0], lse.detach(), "lse")
    _same(fw["p"].sum(-1) + fw["p_sink"], torch.ones_like(lse), "rows of p and the sink sum to 1")
    dq, dk, dv, ds = torch.autograd.grad(o, (q, k, v, sk), inp["do"].to(F64))
    # the backward references from the exact o and lse
    bw = A.bwd_ref(inp["do"], inp["q"], inp["k"], inp["v"], o.detach(), lse.detach(), True, inp["scale"])
    for name, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        _same(bw[name][0], g, name + " (the plain backward on the sink-inclusive lse)")
    delta = (A._bh(inp["do"]) * A._bh(o.detach())).sum(-1)
    dsr, unit = K.dsinks_ref(lse.detach(), delta, inp["sinks"])
    finite = torch.isfinite(inp["sinks"].to(F64))
    _same(dsr[finite], ds[finite], "dsinks = -sum exp(s - lse) delta")
    assert not dsr[~finite].any() and (unit >= 0).all()  # a sink of -inf has no share and no gradient
    # ops.reference (fp32, the CPU path) computes the same
    o32, lse32 = ref.attention(inp["q"], inp["k"], inp["v"], causal=True, scale=inp["scale"], sinks=inp["sinks"])
    _same(o32.float(), fw["o"][0], "ops.reference.attention o", tol=1e-2)
    _same(lse32, fw["lse"][0], "ops.reference.attention lse", tol=1e-5)
    g32 = ref.attention_bwd(inp["do"], inp["q"], inp["k"], inp["v"], o.detach().float(), lse.detach().float(),
                            causal=True, scale=inp["scale"], sinks=inp["sinks"])
    assert len(g32) == 4
    _same(g32[3][finite], ds[finite], "ops.reference.attention_bwd dsinks", tol=1e-4)
    _same(g32[0], dq, "ops.reference.attention_bwd dq", tol=1e-4)


def test_windowed_ref_matches_torch_double():
    case = ("randn", 200, 17, 64, 2)
    inp, fw = K.fwd_case(case, True)
    vis = K.visible(200, 200, True, 17)
    assert vis[100].nonzero().flatten().tolist() == list(range(84, 101))  # W = 17 keys, the query included
    assert inp["kv_start"][1, 100] == 84 and inp["kv_start"][0, 3] == 0
    o, lse = _torch_sink_attention(inp["q"].to(F64), inp["k"].to(F64), inp["v"].to(F64), inp["sinks"].to(F64),
                                   inp["scale"], vis)
    _same(fw["o"][0], o, "windowed o")
    _same(fw["lse"][0], lse, "windowed lse")
    o32, _ = ref.attention(inp["q"], inp["k"], inp["v"], causal=True, scale=inp["scale"],
                           bounds=(inp["kv_start"], None), sinks=inp["sinks"])
    _same(o32.float(), fw["o"][0], "ops.reference.attention with bounds and sinks", tol=1e-2)


def test_gradcheck_of_the_sink_attention():
    g = torch.Generator().manual_seed(5)
    q = torch.randn(1, 5, 4, 4, generator=g, dtype=F64, requires_grad=True)
    k = torch.randn(1, 7, 2, 4, generator=g, dtype=F64, requires_grad=True)
    v = torch.randn(1, 7, 2, 4, generator=g, dtype=F64, requires_grad=True)
    sk = torch.randn(4, generator=g, dtype=F64, requires_grad=True)
    vis = K.visible(5, 7, True)
    assert torch.autograd.gradcheck(lambda *a: _torch_sink_attention(*a, 0.5, vis), (q, k, v, sk))
    # and ops.reference (fp32 inside) on its own autograd agrees with the closed-form dsinks it returns
    q32, k32, v32, s32 = (t.detach().float().requires_grad_() for t in (q, k, v, sk))
    o, lse = ref.attention(q32, k32, v32, causal=True, scale=0.5, sinks=s32)
    do = torch.randn(o.shape, generator=g)
    grads = torch.autograd.grad(o, (q32, k32, v32, s32), do)
    closed = ref.attention_bwd(do, q32.detach(), k32.detach(), v32.detach(), o.detach(), lse.detach(), causal=True,
                               scale=0.5, sinks=s32.detach())
    for a, b, name in zip(closed, grads, ("dq", "dk", "dv", "dsinks")):
        _same(a, b, "ops.reference " + name, tol=1e-5)


@pytest.mark.parametrize("case", [("randn", 33, 33, 32, 2), ("randn", 40, 600, 64, 4)], ids=str)
def test_zero_sink_is_an_extra_zero_key_and_minus_inf_is_plain(case):
    fam, T, S, D, Hkv = case
    inp, _ = K.fwd_case(case)
    zero = K.fwd_ref(inp["q"], inp["k"], inp["v"], True, inp["scale"], torch.zeros(K.H))
    # one more key in front, all zeros with a zero value: visible to every row (queries are aligned to the end)
    k1 = torch.cat([torch.zeros_like(inp["k"][:, :1]), inp["k"]], 1)
    v1 = torch.cat([torch.zeros_like(inp["v"][:, :1]), inp["v"]], 1)
    extra = A.fwd_ref(inp["q"], k1, v1, True, inp["scale"])
    _same(zero["o"][0], extra["o"][0], "o: sinks = 0 against an extra zero key")
    _same(zero["lse"][0], extra["lse"][0], "lse: sinks = 0 against an extra zero key")
    _same(zero["p_sink"], extra["p"][..., 0], "the sink's share is that key's")
    off = K.fwd_ref(inp["q"], inp["k"], inp["v"], True, inp["scale"], torch.full((K.H,), -math.inf))
    plain = A.fwd_ref(inp["q"], inp["k"], inp["v"], True, inp["scale"])
    assert torch.equal(off["o"][0], plain["o"][0]) and torch.equal(off["lse"][0], plain["lse"][0])
    assert not off["p_sink"].any()


def test_decode_ref_and_cases():
    case = (64, 8, 4, 5, 1000, (0, 1, 1000, 65, 300), K.DECODE_WINDOW, "randn")
    inp, (o, unit) = K.decode_case(case)
    assert torch.isfinite(o).all() and torch.isfinite(unit).all()
    assert not o[0].any() and not unit[0].any()  # a count of 0: the sink takes the whole row, o = 0
    for b, n in enumerate(inp["counts"]):
        j0, j1 = K.decode_keys(n, K.DECODE_WINDOW)
        assert (j0, j1) == (max(0, n - 64), n)
        if n:
            oo, _ = _torch_sink_attention(inp["q"][b:b + 1].to(F64), inp["k"][b:b + 1, j0:j1].to(F64),
                                          inp["v"][b:b + 1, j0:j1].to(F64), inp["sinks"].to(F64), inp["scale"],
                                          torch.ones(1, j1 - j0, dtype=torch.bool))
            _same(o[b:b + 1], oo, f"decode row {b}")
    cases = K.decode_cases()
    assert len(set(cases)) == len(cases)
    splits = {K.decode_splits(c) for c in cases}
    assert 1 in splits and max(splits) > 1  # the in-kernel fold and the combine kernel's
    assert all(K.decode_splits(c) == 1 for c in cases if c[6])  # a window of 64 keys is one split
    kinds = {(type(c[5]).__name__, bool(c[6])) for c in cases}
    assert kinds == {(t, w) for t in ("NoneType", "int", "tuple") for w in (False, True)}


# ------------------------------------------------------------------------------------ the choice of the sinks
def _share_ok(p_sink):
    ok = ((p_sink >= 0.05) & (p_sink <= 0.95)).to(F64).mean()
    return float(ok) >= 0.5


def test_sinks_take_a_real_share_of_the_rows():
    """In every randn case the reference's own sink probability lies in [0.05, 0.95] on at least half of the rows, so
    a kernel that ignores the sink is wrong by a large factor on most rows; sinks are distinct per head."""
    for case in K.fwd_cases():
        if case[0] == "randn":
            inp, fw = K.fwd_case(case)
            assert _share_ok(fw["p_sink"]), case
            assert len(set(inp["sinks"].tolist())) == K.H, case
    for case in K.window_cases():
        if case[0] == "randn":
            assert _share_ok(K.fwd_case(case, True)[1]["p_sink"]), case
    for case in K.decode_cases():
        if case[7] == "randn" and any(K.decode_case(case)[0]["counts"]):
            inp, _ = K.decode_case(case)
            ps = []
            for b, n in enumerate(inp["counts"]):
                j0, j1 = K.decode_keys(n, case[6])
                if j1 > j0:
                    ps.append(K.fwd_ref(inp["q"][b:b + 1], inp["k"][b:b + 1, j0:j1], inp["v"][b:b + 1, j0:j1], False,
                                        inp["scale"], inp["sinks"])["p_sink"].flatten())
            assert _share_ok(torch.cat(ps)), case
    for case in K.DS_CASES:
        if case[3] == "randn":
            inp, _ = K.ds_case(case)
            p = torch.exp(inp["sinks"].to(F64).view(1, -1, 1) - inp["lse"].to(F64))
            assert _share_ok(p / (1 + p)) or _share_ok(p.clamp(max=1.0)), case
    ext = K.fwd_case(("extreme", 33, 33, 32, 2))[0]["sinks"].tolist()
    assert ext == [-math.inf, -30.0, 0.0, 30.0]


# ------------------------------------------------------------------------------------ calibration of the budgets
def _fwd_model_of(case, windowed=False, **kw):
    inp, _ = K.fwd_case(case, windowed)
    return K.fwd_model(inp["q"], inp["k"], inp["v"], True, inp["scale"], inp["sinks"], inp["window"], **kw)


def _bwd_model_of(case, **kw):
    """dq / dk / dv by the plain backward model on the sink-inclusive lse, ds from the fp32 delta."""
    inp, _ = K.bwd_case(case)
    out = A.bwd_model(inp["do"], inp["q"], inp["k"], inp["v"], inp["o"], inp["lse"], True, inp["scale"])
    delta32 = (A._bh(inp["do"], F32) * A._bh(inp["o"], F32)).sum(-1)
    out["ds"] = K.dsinks_model(inp["lse"], delta32, inp["sinks"], scale=inp["scale"],
                               hmap=A.head_map(K.H, case[4]), **kw)
    return out


def _decode_model_of(case, **kw):
    inp, _ = K.decode_case(case)
    return K.decode_model(inp["q"], inp["k"], inp["v"], inp["scale"], inp["counts"], inp["sinks"], inp["window"], **kw)


def _model_items():
    """Every generic comparison of the GPU file, with the fp32 / bf16 CPU model in the kernel's place."""
    for case in K.fwd_cases():
        yield from K.fwd_checks(case, _fwd_model_of(case))
    for case in K.window_cases():
        yield from K.fwd_checks(case, _fwd_model_of(case, True), True)
    for case in K.bwd_cases():
        out = _bwd_model_of(case)
        yield from K.bwd_checks(case, out)
        yield ("sink_ds", "ds (delta from the pre-pass)", out["ds"], K.bwd_case(case)[1]["ds"])
    for case in K.DS_CASES:
        inp, r = K.ds_case(case)
        for dt in (BF16, F32):
            yield ("sink_ds", f"ds {dt}", K.dsinks_model(inp["lse"], inp["delta"], inp["sinks"], dt), r)
    for case in K.decode_cases():
        yield ("sink_decode_o", "o", _decode_model_of(case), K.decode_case(case)[1])


def test_budgets_are_calibrated_on_the_model():
    measured, worst = {}, {}
    for it in _model_items():
        op, name, out, (r, unit) = it
        u = K.ulps_needed(out, r, unit)
        if u >= measured.get(op, -1):
            measured[op], worst[op] = u, it
    print("measured smallest budgets:", measured)
    table = {**{op: b[0] for op, b in K.BUDGET.items()}}
    assert {op: m for op, m in measured.items() if op in table} == table, "the table in _attn_sink_refs.py is stale"
    for op in ("attn_dq", "attn_dk", "attn_dv"):  # the existing budgets hold on the sink-inclusive lse
        assert measured[op] <= A.BUDGET[op][0], (op, measured[op])
    for op, (m, b) in K.BUDGET.items():
        assert b == 2 * m and 0 < m < 10
        _, name, out, (r, unit) = worst[op]
        K.check(op, out, (r, unit), name)
        with pytest.raises(AssertionError):
            K.assert_close_ulps(out, r, 0, 0.0, what=f"{op}/{name}")


# ------------------------------------------------------------------------------------ the checks bite
def _some_case_fails(cases, run):
    """``run(case)`` -> [(op, out, ref_unit)]; True when some case fails one of its checks."""
    return any(K.fails(op, out, ru) for case in cases for op, out, ru in run(case))


@pytest.mark.parametrize("defect", K.DEFECTS_FWD)
@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("windowed", [False, True])
def test_forward_defects_break_the_bound(defect, family, windowed):
    cases = [c for c in (K.window_cases() if windowed else K.fwd_cases()) if c[0] == family]

    def run(case):
        return [(op, out, ru) for op, _, out, ru in K.fwd_checks(case, _fwd_model_of(case, windowed, defect=defect),
                                                                windowed)]
    assert _some_case_fails(cases, run), (defect, family, windowed)
    if family == "randn":  # ... on every case where the defect changes anything: all, or those with Hkv < H
        hit = [c for c in cases if defect != "kvhead" or c[4] != K.H]
        assert all(_some_case_fails([c], run) for c in hit), defect
    assert not _some_case_fails(cases, lambda c: [(op, out, ru) for op, _, out, ru in
                                                  K.fwd_checks(c, _fwd_model_of(c, windowed), windowed)])


@pytest.mark.parametrize("defect", K.DEFECTS_DS)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_dsinks_defects_break_the_bound(defect, family):
    cases = [c for c in K.bwd_cases() if c[0] == family]
    def run(d):
        return lambda case: [("sink_ds", _bwd_model_of(case, defect=d)["ds"], K.bwd_case(case)[1]["ds"])]
    assert _some_case_fails(cases, run(defect)), (defect, family)
    assert not _some_case_fails(cases, run(None))
    if defect in ("dropped", "sign"):  # the op on its own: lse and delta are inputs, scale and head map are not
        ds_cases = [c for c in K.DS_CASES if c[3] == family]

        def run_op(case, d=defect):
            inp, r = K.ds_case(case)
            return [("sink_ds", K.dsinks_model(inp["lse"], inp["delta"], inp["sinks"], F32, defect=d), r)]
        assert _some_case_fails(ds_cases, run_op), (defect, family)
        assert not _some_case_fails(ds_cases, lambda c: run_op(c, None))


@pytest.mark.parametrize("defect", K.DEFECTS_DECODE)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_decode_defects_break_the_bound(defect, family):
    cases = [c for c in K.decode_cases() if c[7] == family]
    def run(d):
        return lambda case: [("sink_decode_o", _decode_model_of(case, defect=d), K.decode_case(case)[1])]
    assert _some_case_fails(cases, run(defect)), (defect, family)
    assert not _some_case_fails(cases, run(None))
    if defect == "per_split" and family == "randn":  # every case that the combine kernel serves
        multi = [c for c in cases if K.decode_splits(c) > 1 and any(K.decode_case(c)[0]["counts"])]
        assert multi and all(_some_case_fails([c], run(defect)) for c in multi)
