"""CPU checks of ``_attention_refs``: every fp64 reference against an independent PyTorch double-precision path
(autograd through ``softmax``, ``logsumexp``) to 1e-12 relative, the calibration of the per-output budgets against the
fp32 / bf16 model of the kernels' documented roundings on the cases ``test_attention_edges_gpu.py`` runs, and the proof
that the per-element checks catch single-tile defects which a whole-tensor norm lets through."""
import math

import pytest
import torch

import _attention_refs as A

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32


def _same(a, b, what, tol=1e-12):
    """max|a - b| <= tol max|b|: both sides are fp64 evaluations of the same formula in a different order."""
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert float((a - b).abs().max()) <= tol * scale, f"{what}: {float((a - b).abs().max())} vs scale {scale}"


def _rel(a, b):
    """The whole-tensor relative error the norm tests judge by."""
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _torch_attention(q, k, v, causal, scale):
    """softmax attention on fp64 leaves [B, L, H, D] (kv heads repeated per group), by PyTorch's own ops."""
    T, Hq, S, Hkv = q.shape[1], q.shape[2], k.shape[1], k.shape[2]
    kk = k.repeat_interleave(Hq // Hkv, dim=2)
    vv = v.repeat_interleave(Hq // Hkv, dim=2)
    s = torch.einsum("bthd,bshd->bhts", q, kk) * scale
    if causal:
        s = s.masked_fill(~torch.ones(T, S, dtype=torch.bool).tril(diagonal=S - T), -math.inf)
    o = torch.einsum("bhts,bshd->bthd", torch.softmax(s, -1), vv)
    return o, torch.logsumexp(s, -1)


def _rope(x, cos, sin, pos0):
    """Rotate-half RoPE of x [B, L, H, D] in fp64, row l at position pos0 + l."""
    L, D = x.shape[1], x.shape[3]
    c = cos[pos0:pos0 + L].to(F64)[None, :, None, :]
    s = sin[pos0:pos0 + L].to(F64)[None, :, None, :]
    x1, x2 = x[..., : D // 2], x[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


REF_CASES = [("randn", 33, 33, 1, 32, 2), ("randn", 200, 264, 1, 64, 1), ("wide", 130, 70, 0, 128, 4),
             ("randn", 96, 300, 0, 32, 1), ("count", 65, 65, 1, 64, 2), ("randn", 1, 65, 1, 128, 4)]


# ------------------------------------------------------------------------------------ references vs PyTorch fp64
@pytest.mark.parametrize("case", REF_CASES, ids=str)
def test_fwd_bwd_refs_match_torch_double(case):
    inp = A.attn_inputs(*case)
    q, k, v = (inp[n].to(F64).requires_grad_() for n in ("q", "k", "v"))
    o, lse = _torch_attention(q, k, v, inp["causal"], inp["scale"])
    ref = A.fwd_ref(inp["q"], inp["k"], inp["v"], inp["causal"], inp["scale"])
    _same(ref["o"][0], o.detach(), "o")
    _same(ref["lse"][0], lse.detach(), "lse")
    _same(ref["p"].sum(-1), torch.ones_like(lse), "rows of p sum to 1")
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), inp["do"].to(F64))
    # the backward reference from the exact o and lse (the bf16 / fp32 ones the kernel is fed differ at 2^-9)
    bw = A.bwd_ref(inp["do"], inp["q"], inp["k"], inp["v"], o.detach(), lse.detach(), inp["causal"], inp["scale"])
    _same(bw["dq"][0], dq, "dq")
    _same(bw["dk"][0], dk, "dk")
    _same(bw["dv"][0], dv, "dv")
    for name in ("dq", "dk", "dv"):
        assert (bw[name][1] >= 0).all() and bw[name][1].shape == bw[name][0].shape


@pytest.mark.parametrize("case", [("randn", 40, 72, 1, 32, 2), ("randn", 70, 70, 1, 128, 1)], ids=str)
def test_rope_rotate_back_ref_matches_torch_double(case):
    """The expected dq / dk with tables are the gradients of the UNROTATED heads: autograd through an independent
    rotation, query t at position t + S - T."""
    fam, T, S, causal, D, Hkv = case
    inp = A.attn_inputs(*case)
    cos, sin = A.rope_tables(S + 3, D)
    q0, k0, v = (inp[n].to(F64).requires_grad_() for n in ("q", "k", "v"))
    qr, kr = _rope(q0, cos, sin, S - T), _rope(k0, cos, sin, 0)
    o, lse = _torch_attention(qr, kr, v, True, inp["scale"])
    dq, dk, dv = torch.autograd.grad(o, (q0, k0, v), inp["do"].to(F64))
    bw = A.bwd_ref(inp["do"], qr.detach(), kr.detach(), inp["v"], o.detach(), lse.detach(), True, inp["scale"],
                   cos, sin)
    _same(bw["dq"][0], dq, "dq rotated back")
    _same(bw["dk"][0], dk, "dk rotated back")
    _same(bw["dv"][0], dv, "dv")
    # the unit moves with the rotation: one that lives in a single dim spreads to that dim and its partner
    unit = torch.zeros(1, 1, 1, D, dtype=F64)
    unit[..., 3] = 1.0
    ru = A.rotate_back_unit(unit, cos, sin, 5)
    assert float(ru[0, 0, 0, 3]) == abs(float(cos[5, 3])) and float(ru[0, 0, 0, 3 + D // 2]) == abs(float(sin[5, 3]))
    assert float(ru.sum()) == float(ru[0, 0, 0, 3] + ru[0, 0, 0, 3 + D // 2])


@pytest.mark.parametrize("causal", [0, 1])
def test_partial_block_ref_matches_whole_row_autograd(causal):
    """The context-parallel form: the row's keys split into two blocks, each block's backward given the lse and o of
    the WHOLE row.  dk / dv of a block are the whole attention's gradients of its keys; the dq of the blocks add up."""
    T, S1, S2, D, Hkv = 40, 72, 40, 32, 2
    inp = A.attn_inputs("randn", T, S1 + S2, causal, D, Hkv)
    q, k, v = (inp[n].to(F64).requires_grad_() for n in ("q", "k", "v"))
    o, lse = _torch_attention(q, k, v, bool(causal), inp["scale"])
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), inp["do"].to(F64))
    # block 1: keys [0, S1), every one visible to every query under the causal mask too (S1 <= S - T): non-causal;
    # block 2: keys [S1, S), aligned to the end: the causal block
    b1 = A.bwd_ref(inp["do"], inp["q"], inp["k"][:, :S1], inp["v"][:, :S1], o.detach(), lse.detach(), False,
                   inp["scale"])
    b2 = A.bwd_ref(inp["do"], inp["q"], inp["k"][:, S1:], inp["v"][:, S1:], o.detach(), lse.detach(), bool(causal),
                   inp["scale"])
    _same(torch.cat([b1["dk"][0], b2["dk"][0]], 1), dk, "dk of the blocks")
    _same(torch.cat([b1["dv"][0], b2["dv"][0]], 1), dv, "dv of the blocks")
    _same(b1["dq"][0] + b2["dq"][0], dq, "dq summed over the blocks")
    # the partial family of the GPU file: P sums to less than 1 / 2 in every row
    pinp, _ = A.bwd_case(("randn", 200, 264, 1, 32, 4), "partial")
    fw = A.fwd_ref(pinp["q"], pinp["k"], pinp["v"], True, pinp["scale"])
    psum = torch.exp(fw["lse"][0] - pinp["lse"].to(F64))
    assert float(psum.max()) < 0.5 and float(psum.min()) > 0.05


def test_decode_ref_matches_torch_double():
    case = (64, 8, 4, 5, 1000, (0, 1, 1000, 65, 300))
    inp, (ref, unit) = A.decode_case(case)
    assert torch.isfinite(ref).all() and torch.isfinite(unit).all()  # the NaN rows past a count are never read
    for b, n in enumerate(inp["counts"]):
        if n == 0:
            assert not ref[b].any() and not unit[b].any()
            continue
        o, _ = _torch_attention(inp["q"][b:b + 1].to(F64), inp["k"][b:b + 1, :n].to(F64),
                                inp["v"][b:b + 1, :n].to(F64), False, inp["scale"])
        _same(ref[b:b + 1], o, f"decode row {b}")
    assert [A.decode_splits(2, 4, S) for S in A.DECODE_S] == [1, 1, 1, 1, 2, 5, 16]
    assert A.decode_splits(64, 8, 130) == 1 and A.decode_splits(8, 8, 1000) == 8 and A.decode_splits(1, 2, 4100) == 64


def test_mask_and_count_family():
    """Key j visible to query i iff j <= i + S - T; the count family's lse and o are what ``count_facts`` says."""
    vis = A.visible(3, 5, True)
    assert vis.tolist() == [[1, 1, 1, 0, 0], [1, 1, 1, 1, 0], [1, 1, 1, 1, 1]]
    assert A.visible(4, 2, False).all()
    for case in (("count", 200, 264, 1, 32, 2), ("count", 130, 70, 0, 64, 1)):
        inp, ref = A.fwd_case(case)
        out = A.fwd_model(inp["q"], inp["k"], inp["v"], inp["causal"], inp["scale"])
        A.count_facts(case, out)
        # one key more or less on one row is far outside the lse bound
        lse = out["lse"].clone()
        n = int(A.visible(case[1], case[2], case[3])[-1].sum())
        lse[1, 2, -1] = math.log(n - 1)
        with pytest.raises(AssertionError, match=r"count/lse.*1 of"):
            A.count_facts(case, dict(o=out["o"], lse=lse))


# ------------------------------------------------------------------------------------ calibration of the budgets
def _model_items():
    """Every generic comparison of the GPU file, with the fp32 / bf16 CPU model in the kernel's place."""
    for case in A.fwd_cases():
        inp, _ = A.fwd_case(case)
        out = A.fwd_model(inp["q"], inp["k"], inp["v"], inp["causal"], inp["scale"])
        if case[0] == "count":
            A.count_facts(case, out)
        yield from A.fwd_checks(case, out)
    for mode, cases in (("plain", A.bwd_cases()), ("rope", A.rope_cases()), ("partial", A.partial_cases())):
        for case in cases:
            inp, _ = A.bwd_case(case, mode)
            yield from A.bwd_checks(case, A.bwd_model(*A.bwd_args(inp)), mode)
    for case in A.decode_cases():
        inp, ref = A.decode_case(case)
        yield ("decode_o", "o", A.decode_model(inp["q"], inp["k"], inp["v"], inp["scale"], inp["counts"]), ref)


def test_budgets_are_calibrated_on_the_model():
    measured, worst = {}, {}
    for it in _model_items():
        op, name, out, (ref, unit) = it
        u = A.ulps_needed(out, ref, unit)
        if u >= measured.get(op, -1):
            measured[op], worst[op] = u, it
    print("measured smallest budgets:", measured)
    assert measured == {op: b[0] for op, b in A.BUDGET.items()}, "the table in _attention_refs.py is stale"
    for op, (m, b) in A.BUDGET.items():
        assert b == 2 * m and 0 < m < 10  # a two-digit budget means a unit is wrong
        _, name, out, (ref, unit) = worst[op]
        A.check(op, out, (ref, unit), name)  # the worst case passes at the budget
        with pytest.raises(AssertionError):  # and fails at a zero budget
            A.assert_close_ulps(out, ref, 0, 0.0, what=f"{op}/{name}")


def test_exact_zero_rows_need_no_floor():
    """dq of a causal row that sees one key is exactly 0 in the reference (P = 1, o = v, delta = dP); its bound is
    the fp32 cancellation term alone, and the model meets it."""
    case = ("randn", 33, 33, 1, 32, 2)
    inp, ref = A.bwd_case(case)
    dq_ref, unit = ref["dq"]
    assert float(dq_ref[:, 0].abs().max()) < 1e-2 * float(dq_ref[:, 5:].abs().max())
    assert float(unit[:, 0].max()) < 1e-5  # no bf16-sized allowance on that row
    out = A.bwd_model(*A.bwd_args(inp))
    A.check("attn_dq", out["dq"][:, :1], (dq_ref[:, :1], unit[:, :1]), "dq of the first row")


# ------------------------------------------------------------------------------------ the checks bite
def _fails(op, out, ref_unit):
    try:
        A.check(op, out, ref_unit, "defect")
    except AssertionError:
        return True
    return False


def _judge(tag, outs, refs, affected, ops, norm_blind=False):
    """Every affected output must fail its per-element check; the whole-tensor error is printed beside it."""
    for name in outs:
        failed = _fails(ops[name], outs[name], refs[name])
        ratio = A.worst_ratio(ops[name], outs[name], refs[name])
        print(f"{tag}: {name}: whole-tensor relative error {_rel(outs[name], refs[name][0]):.4f}, worst element "
              f"{ratio:.1f} x its bound, per-element check {'FAILS' if failed else 'passes'}")
        assert failed == (name in affected), (tag, name)
        if norm_blind and name in affected:  # the 2e-2 of the whole-tensor tests lets this defect through
            assert _rel(outs[name], refs[name][0]) < 2e-2, (tag, name)


OPS = dict(o="attn_o", lse="attn_lse", dq="attn_dq", dk="attn_dk", dv="attn_dv")


def _run_defect(tag, case, affected, vis=None, hmap=None, extra_key=False, norm_blind=False):
    inp, fref = A.fwd_case(case)
    binp, bref = A.bwd_case(case)
    k, v = inp["k"], inp["v"]
    if extra_key:  # the row after the last key: what a read one row past S finds
        g = A._gen(14, *case[1:])
        k = torch.cat([k, (0.8 * torch.randn(A.B, 1, case[5], case[4], generator=g)).to(BF16)], 1)
        v = torch.cat([v, torch.randn(A.B, 1, case[5], case[4], generator=g).to(BF16)], 1)
    S = inp["k"].shape[1]
    fo = A.fwd_model(inp["q"], k, v, inp["causal"], inp["scale"], vis=vis, hmap=hmap)
    bo = A.bwd_model(binp["do"], binp["q"], k, v, binp["o"], binp["lse"], binp["causal"], binp["scale"],
                     vis=vis, hmap=hmap)
    outs = dict(o=fo["o"], lse=fo["lse"], dq=bo["dq"], dk=bo["dk"][:, :S], dv=bo["dv"][:, :S])
    _judge(tag, outs, {**{n: fref[n] for n in ("o", "lse")}, **bref}, affected, OPS, norm_blind)
    # the unbroken model passes all five
    fo = A.fwd_model(inp["q"], inp["k"], inp["v"], inp["causal"], inp["scale"])
    bo = A.bwd_model(*A.bwd_args(binp))
    _judge(tag + " (no defect)", {**fo, **bo}, {**{n: fref[n] for n in ("o", "lse")}, **bref}, (), OPS)


@pytest.mark.parametrize("D", [64, 128])
def test_defect_one_key_past_the_diagonal_in_one_sub_block(D):
    """One 32-query sub-block (rows 96 .. 127 of one batch and head) admits the first key past the causal diagonal,
    as if it had taken the unmasked code path for that key column.  Every output fails its per-element check while its
    whole-tensor relative error stays under the 2e-2 of the norm tests -- at T = 300; at the workload's T = 2048 the
    one sub-block weighs less still."""
    case = ("randn", 300, 340, 1, D, 2)
    T, S = 300, 340
    vis = A.visible(T, S, True)[None, None].repeat(A.B, A.H, 1, 1)
    rows = torch.arange(96, 128)
    vis[1, 2, rows, rows + (S - T) + 1] = True
    _run_defect(f"diagonal+1, D={D}", case, ("o", "lse", "dq", "dk", "dv"), vis=vis, norm_blind=True)


def test_defect_one_key_past_S():
    """Every query also sees the row after the last key (non-causal, ragged last key tile).  P is fixed by the lse
    handed to the backward, so dk / dv of the real keys do not move: o, lse and dq do."""
    case = ("randn", 96, 700, 0, 64, 1)
    _run_defect("key S admitted", case, ("o", "lse", "dq"), vis=torch.ones(96, 701, dtype=torch.bool),
                extra_key=True)


def test_defect_one_gqa_head_reads_the_wrong_kv_head():
    case = ("randn", 200, 264, 1, 32, 2)
    hmap = A.head_map(A.H, 2).clone()
    hmap[1] = 1  # head 1 belongs to kv head 0
    _run_defect("head 1 -> kv head 1", case, ("o", "lse", "dq", "dk", "dv"), hmap=hmap)
