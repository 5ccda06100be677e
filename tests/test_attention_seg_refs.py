"""CPU checks of the per-row key-bound references (``_attention_seg_refs``): they equal torch double-precision
autograd through a masked softmax, the two bound forms describe one mask, ``ops.doc_bounds`` / ``bounds_from_start``
build them, the budgets of ``_attention_refs.BUDGET`` hold for these masks too, and the per-element checks catch one
key admitted before ``kv_start`` or one query admitted past ``q_last``."""
import math

import pytest
import torch

import _attention_refs as A
import _attention_seg_refs as G

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _torch_attention(q, k, v, vis, scale):
    """Masked softmax attention in plain torch (autograd-able); q [B, T, H, D], vis [B, T, T]."""
    Hq, Hkv = q.shape[2], k.shape[2]
    hmap = A.head_map(Hq, Hkv)
    qh, kh, vh = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3)[:, hmap], v.permute(0, 2, 1, 3)[:, hmap]
    s = (scale * (qh @ kh.transpose(-1, -2))).masked_fill(~vis[:, None], -math.inf)
    return (torch.softmax(s, -1) @ vh).permute(0, 2, 1, 3), torch.logsumexp(s, -1)


REF_CASES = [c for c in G.cases() if c[0] == "randn" and c[1] in (33, 257)] + G.rope_cases()[:1]


@pytest.mark.parametrize("case", REF_CASES, ids=str)
def test_refs_match_torch_double(case):
    inp, fw = G.fwd_case(case)
    q, k, v = (inp[n].to(F64).requires_grad_() for n in ("q", "k", "v"))
    o, lse = _torch_attention(q, k, v, inp["vis"], inp["scale"])
    torch.testing.assert_close(fw["o"][0], o.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(fw["lse"][0], lse.detach(), rtol=1e-12, atol=1e-12)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), inp["do"].to(F64))
    # the reference backward from the exact o / lse is the autograd gradient
    bw = G.bwd_ref(inp["do"], inp["q"], inp["k"], inp["v"], o.detach(), lse.detach(), inp["vis"], inp["scale"])
    for n, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        torch.testing.assert_close(bw[n][0], g, rtol=1e-9, atol=1e-11, msg=n)


def test_rope_rotate_back_ref_matches_torch_double():
    case = G.rope_cases()[0]
    inp, _ = G.bwd_case(case, "rope")
    T, D = case[1], case[2]
    cos, sin = inp["cos"].to(F64), inp["sin"].to(F64)

    def rot(x):
        c, s = cos[:T][None, :, None, :], sin[:T][None, :, None, :]
        x1, x2 = x[..., : D // 2], x[..., D // 2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)

    # unrotated heads whose rotation is the case's q / k
    q0 = A.rotate_back(inp["q"].to(F64), cos, sin, 0).requires_grad_()
    k0 = A.rotate_back(inp["k"].to(F64), cos, sin, 0).requires_grad_()
    o, lse = _torch_attention(rot(q0), rot(k0), inp["v"].to(F64), inp["vis"], inp["scale"])
    dq, dk = torch.autograd.grad(o, (q0, k0), inp["do"].to(F64))
    bw = G.bwd_ref(inp["do"], rot(q0).detach(), rot(k0).detach(), inp["v"], o.detach(), lse.detach(), inp["vis"],
                   inp["scale"], inp["cos"], inp["sin"])
    torch.testing.assert_close(bw["dq"][0], dq, rtol=1e-6, atol=1e-8)
    torch.testing.assert_close(bw["dk"][0], dk, rtol=1e-6, atol=1e-8)


# ------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize("T", G.GEOMS + (G.ROPE_T,))
@pytest.mark.parametrize("pattern", G.PATTERNS)
def test_both_bound_forms_give_one_mask(pattern, T):
    from pretraining_llm_amd import ops
    ks = G.kv_start_of(pattern, T)
    ql = G.q_last_of(ks)
    i = torch.arange(T, dtype=torch.int32)
    assert (ks[1:] >= ks[:-1]).all() and (ks >= 0).all() and (ks <= i).all()
    assert (ql[1:] >= ql[:-1]).all() and (ql >= i).all() and (ql <= T - 1).all()
    assert torch.equal(G.vis_from_start(ks), G.vis_from_last(ql))
    got = ops.bounds_from_start(ks[None])
    assert got.dtype == torch.int32 and torch.equal(got[0], ql)


def test_pattern_facts():
    """What the issue's cases rely on."""
    T = 513
    vis = G.vis_from_start(G.kv_start_of("halves", T))
    assert not vis[256:, :256].any() and vis[255, :256].all() and vis[512, 256:].all()
    assert G.q_last_of(G.kv_start_of("halves", T))[255] == 255          # block 0's sweep ends at the block edge
    assert (G.kv_start_of("halves", T)[256:] // A.KEY_BLOCK == 1).all()  # the reduce's kmin
    assert G.vis_from_start(G.kv_start_of("single", T)).sum() == T
    late = G.vis_from_start(G.kv_start_of("late", T))
    assert late[T - 1].sum() == 1 and late[T - 2].sum() == T - 1
    w = G.vis_from_start(G.kv_start_of("window40", T))
    assert w[100].sum() == 40 and w[100, 61] and not w[100, 60] and w[10].sum() == 11
    d = G.kv_start_of("docs", T).tolist()
    assert [d[i] for i in (0, 1, 30, 31, 32, 33, 63, 64, 65, 255, 256, 257, 510, 511, 512)] == \
        [0, 1, 1, 31, 32, 33, 33, 64, 65, 255, 256, 257, 300, 511, 512]
    assert torch.equal(G.vis_from_start(G.kv_start_of("one_doc", T)), A.visible(T, T, True))


SEP = 7


@pytest.mark.parametrize("row,ks,ql", [
    # a separator is the last token of the document it ends
    ([1, 2, SEP, 3, 4, 5], [0, 0, 0, 3, 3, 3], [2, 2, 2, 5, 5, 5]),
    ([SEP, 1, 2, 3], [0, 1, 1, 1], [0, 3, 3, 3]),                       # a separator at position 0
    ([1, 2, 3, SEP], [0, 0, 0, 0], [3, 3, 3, 3]),                       # ... at the last position
    ([1, SEP, SEP, 2, SEP, SEP], [0, 0, 2, 3, 3, 5], [1, 1, 2, 4, 4, 5]),  # adjacent separators
    ([1, 2, 3, 4], [0, 0, 0, 0], [3, 3, 3, 3]),                         # none at all
    ([SEP], [0], [0]),
])
def test_doc_bounds(row, ks, ql):
    from pretraining_llm_amd import ops
    other = [SEP] * len(row)  # a second batch row (every token its own document)
    k, q = ops.doc_bounds(torch.tensor([row, other]), SEP)
    assert k.dtype == torch.int32 and q.dtype == torch.int32 and k.is_contiguous() and q.is_contiguous()
    assert k[0].tolist() == ks and q[0].tolist() == ql
    assert k[1].tolist() == list(range(len(row))) and q[1].tolist() == list(range(len(row)))
    assert torch.equal(ops.bounds_from_start(k), q)
    assert torch.equal(G.vis_from_start(k[0]), G.vis_from_last(q[0]))


# ------------------------------------------------------------------------------------------------ budgets
def _model_items():
    for case in G.cases():
        inp, _ = G.fwd_case(case)
        vis = inp["vis"][:, None]
        out = A.fwd_model(inp["q"], inp["k"], inp["v"], True, inp["scale"], vis=vis)
        yield from G.fwd_checks(case, out)
        binp, _ = G.bwd_case(case)
        out = A.bwd_model(*A.bwd_args(binp), vis=vis)
        yield from G.bwd_checks(case, out)
    for case in G.rope_cases():
        binp, _ = G.bwd_case(case, "rope")
        out = A.bwd_model(*A.bwd_args(binp), vis=binp["vis"][:, None])
        yield from G.bwd_checks(case, out, "rope")


def test_budgets_hold_for_the_bounded_masks():
    """The plain PyTorch models of ``_attention_refs`` (the documented roundings, nothing else) under these masks need
    the budgets already tabulated there: 2 / 1 / 2 / 2 / 2 ulps for o / lse / dq / dk / dv measured, so the GPU tests
    use the table's 4 / 2 / 4 / 4 / 4.  The measured values are asserted, so a stale table fails."""
    measured = {}
    for op, name, out, (ref, unit) in _model_items():
        measured[op] = max(measured.get(op, 0), A.ulps_needed(out, ref, unit))
    print("measured smallest budgets under bounds:", measured)
    for op in ("attn_o", "attn_lse", "attn_dq", "attn_dk", "attn_dv"):
        assert measured[op] == A.BUDGET[op][0] and G.budget(op) == A.BUDGET[op], (op, measured[op])
    for op in ("attn_dq_rot", "attn_dk_rot"):  # the bounded RoPE case: see the helper's docstring
        assert measured[op] == G.ROT_BUDGET[op][0] and G.ROT_BUDGET[op][1] == 2 * measured[op], (op, measured[op])


# ------------------------------------------------------------------------------------------------ defects
def _fails(items):
    failed = []
    for op, name, out, ref_unit in items:
        try:
            G.check_all([(op, name, out, ref_unit)])
        except AssertionError:
            failed.append(name)
    return failed


@pytest.mark.parametrize("D", [32, 64, 128])
def test_defect_one_sub_block_admits_the_key_before_kv_start(D):
    """Rows 96 .. 127 of batch row 0 (pattern docs) see one key too many on the left."""
    case = ("randn", 200, D, 2, "docs", "window40")
    inp, _ = G.bwd_case(case)
    vis = inp["vis"].clone()
    ks = inp["kv_start"][0].long()
    rows = torch.arange(96, 128)
    assert (ks[rows] > 0).all()
    vis[0, rows, ks[rows] - 1] = True
    out = A.fwd_model(inp["q"], inp["k"], inp["v"], True, inp["scale"], vis=vis[:, None])
    assert set(_fails(G.fwd_checks(case, out))) == {"o", "lse"}
    out = A.bwd_model(*A.bwd_args(inp), vis=vis[:, None])
    assert set(_fails(G.bwd_checks(case, out))) == {"dq", "dk", "dv"}


@pytest.mark.parametrize("D", [32, 64, 128])
def test_defect_one_key_column_survives_one_query_past_q_last(D):
    """Key 100 of batch row 1 (pattern window40: q_last = 139) is also seen by query 140."""
    case = ("randn", 200, D, 2, "docs", "window40")
    inp, _ = G.bwd_case(case)
    assert inp["q_last"][1, 100] == 139
    vis = inp["vis"].clone()
    vis[1, 140, 100] = True
    out = A.bwd_model(*A.bwd_args(inp), vis=vis[:, None])
    failed = _fails(G.bwd_checks(case, out))
    assert "dk" in failed and "dv" in failed and "dq" in failed, failed
    out = A.fwd_model(inp["q"], inp["k"], inp["v"], True, inp["scale"], vis=vis[:, None])
    assert set(_fails(G.fwd_checks(case, out))) == {"o", "lse"}


# ------------------------------------------------------------------------------------------------ ops.reference
@pytest.mark.parametrize("case", [("randn", 200, 32, 2, "docs", "window40"), ("randn", 257, 64, 1, "halves", "single")],
                         ids=str)
def test_reference_ops_take_bounds(case):
    from pretraining_llm_amd.ops import reference as ref
    inp, fw = G.fwd_case(case)
    bounds = (inp["kv_start"], inp["q_last"])
    q, k, v, do = (inp[n].float() for n in ("q", "k", "v", "do"))
    o, lse = ref.attention(q, k, v, causal=True, scale=inp["scale"], bounds=bounds)
    torch.testing.assert_close(o.double(), fw["o"][0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse.double(), fw["lse"][0], rtol=1e-5, atol=1e-5)
    dq, dk, dv = ref.attention_bwd(do, q, k, v, o, lse, causal=True, scale=inp["scale"], bounds=bounds)
    bw = G.bwd_ref(do, q, k, v, o, lse, inp["vis"], inp["scale"])
    for n, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        torch.testing.assert_close(g.double(), bw[n][0], rtol=1e-4, atol=1e-5, msg=n)
    with pytest.raises(ValueError):
        ref.attention(q, k, v, causal=False, scale=inp["scale"], bounds=bounds)
