"""The attention HIP kernels with per-row key bounds (``attn_fwd(..., kv_start)``, ``attn_bwd(..., kv_start, q_last)``:
document and window masks), compared element by element with the fp64 references of ``_attention_seg_refs`` under the
budgets of ``_attention_refs`` (re-measured for these masks in ``test_attention_seg_refs.py``).  Every check judges
every element: no row, head or tile is left out.

The ops are called through ``torch.ops.pllm`` directly, so the tests control strides and optional arguments."""
import math

import pytest
import torch

import _attention_refs as A
import _attention_seg_refs as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()


def _ops():
    return torch.ops.pllm


def _d(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _fwd(inp, bounded=True):
    o, lse = _ops().attn_fwd(_d(inp["q"]), _d(inp["k"]), _d(inp["v"]), True, inp["scale"],
                             _d(inp["kv_start"]) if bounded else None)
    torch.cuda.synchronize()
    return dict(o=o, lse=lse)


def _bwd(inp, ws_mb=None, delta=False, bounded=True):
    """attn_bwd on a case's inputs; ``ws_mb``: the dQ slab workspace for this call (restored afterwards)."""
    do, q, k, v, o, lse = (_d(inp[n]) for n in ("do", "q", "k", "v", "o", "lse"))
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    dl = (do.float() * o.float()).sum(-1).permute(0, 2, 1).contiguous() if delta else None  # [B, H, T] fp32
    ks, ql = (_d(inp["kv_start"]), _d(inp["q_last"])) if bounded else (None, None)
    try:
        if ws_mb is not None:
            _ops().attn_bwd_set_workspace_mb(ws_mb)
        _ops().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, True, inp["scale"], _d(inp["cos"]), _d(inp["sin"]), dl, ks, ql)
        torch.cuda.synchronize()
    finally:
        if ws_mb is not None:
            _ops().attn_bwd_set_workspace_mb(4096)
    return dict(dq=dq, dk=dk, dv=dv)


# ----------------------------------------------------------------------------------------------- forward / backward
@pytest.mark.parametrize("case", G.cases(), ids=str)
def test_attn_fwd_bounds(case):
    inp, _ = G.fwd_case(case)
    out = _fwd(inp)
    G.check_all(G.fwd_checks(case, out))
    if case[0] == "count":
        G.count_facts(case, out)


# D = 32 / 64 run the fused-role kernel, D = 128 the key-stationary one.  one_block: one 256-key block per pass (the
# fp32 running sum between passes, with passes that lie wholly before a query tile's kmin); delta: rowsum(dO o) handed in
@pytest.mark.parametrize("variant", ["default", "one_block", "delta"])
@pytest.mark.parametrize("case", G.cases(), ids=str)
def test_attn_bwd_bounds(case, variant):
    inp, _ = G.bwd_case(case)
    out = _bwd(inp, ws_mb=1e-3 if variant == "one_block" else None, delta=variant == "delta")
    G.check_all(G.bwd_checks(case, out))


@pytest.mark.parametrize("variant", ["default", "one_block"])
@pytest.mark.parametrize("case", G.rope_cases(), ids=str)
def test_attn_bwd_bounds_rope_rotate_back(case, variant):
    inp, _ = G.bwd_case(case, "rope")
    out = _bwd(inp, ws_mb=1e-3 if variant == "one_block" else None)
    G.check_all(G.bwd_checks(case, out, "rope"))


# ----------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("D,Hkv", [(32, 1), (64, 4), (128, 2)])
def test_one_document_is_bit_identical_to_no_bounds(D, Hkv):
    case = ("randn", 513, D, Hkv, "one_doc", "one_doc")
    inp, _ = G.bwd_case(case)
    a, b = _fwd(inp), _fwd(inp, bounded=False)
    for n in a:
        assert torch.equal(_bits(a[n]), _bits(b[n])), n
    a, b = _bwd(inp), _bwd(inp, bounded=False)
    for n in a:
        assert torch.equal(_bits(a[n]), _bits(b[n])), n


@pytest.mark.parametrize("D,Hkv", [(32, 2), (64, 1), (128, 4)])
def test_repeated_calls_are_bit_identical(D, Hkv):
    case = ("randn", 513, D, Hkv, "docs", "window40")
    inp, _ = G.bwd_case(case)
    a, b = _fwd(inp), _fwd(inp)
    a.update(_bwd(inp))
    b.update(_bwd(inp))
    for n in a:
        assert torch.equal(_bits(a[n]), _bits(b[n])), n


# ----------------------------------------------------------------------------------------------- memory independence
# The inputs are views into NaN-filled buffers, the bound arrays views into a buffer of out-of-range values, the
# gradients go into views of a patterned buffer: the results equal, bit for bit, those of the compact call, and nothing
# outside the views is written.
PATTERN = 0x3C5A  # a finite bf16 (about 0.0133)


def _nan_view(t, pad_rows, pad_heads):
    Bb, L, Hx, D = t.shape
    buf = torch.full((Bb, L + pad_rows, Hx + pad_heads, D), math.nan, dtype=t.dtype, device=DEV)
    view = buf[:, :L, :Hx]
    view.copy_(t)
    return view


def _bound_in_junk(t):
    """An int32 [B, T] bound array as a contiguous view inside a buffer whose other elements are far out of range."""
    Bb, T = t.shape
    buf = torch.full((Bb * T + 64,), 1 << 30, dtype=torch.int32, device=DEV)
    buf[:32] = -(1 << 30)
    view = buf[32:32 + Bb * T].view(Bb, T)
    view.copy_(t)
    return view


@pytest.mark.parametrize("D,Hkv", [(32, 1), (64, 4), (128, 2)])
def test_bounded_reads_and_writes_stay_inside_padded_views(D, Hkv):
    case = ("randn", 257, D, Hkv, "docs", "window40")
    inp, _ = G.bwd_case(case)
    want = _fwd(inp)
    want.update(_bwd(inp))
    q, k, v, do, o_in = (_nan_view(_d(inp[n]), 5, 1) for n in ("q", "k", "v", "do", "o"))
    ks, ql = _bound_in_junk(_d(inp["kv_start"])), _bound_in_junk(_d(inp["q_last"]))
    o, lse = _ops().attn_fwd(q, k, v, True, inp["scale"], ks)
    shapes = [q.shape, k.shape, v.shape]
    bufs = [torch.full((s[0], s[1] + 3, s[2] + 1, s[3]), PATTERN, dtype=torch.int16, device=DEV) for s in shapes]
    dq, dk, dv = (b.view(BF16)[:, :s[1], :s[2]] for b, s in zip(bufs, shapes))
    _ops().attn_bwd(do, q, k, v, o_in, _d(inp["lse"]), dq, dk, dv, True, inp["scale"], None, None, None, ks, ql)
    torch.cuda.synchronize()
    for n, t in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(want[n].float()).all()
        assert torch.equal(_bits(t), _bits(want[n])), f"{n}: strided / padded call differs from the compact one"
    for b, s in zip(bufs, shapes):
        outside = torch.ones(b.shape, dtype=torch.bool, device=DEV)
        outside[:, :s[1], :s[2]] = False
        assert (b[outside] == PATTERN).all(), "a write outside the output view"


# ----------------------------------------------------------------------------------------------- host checks
def _small():
    case = ("randn", 33, 32, 2, "docs", "window40")
    inp, _ = G.bwd_case(case)
    return {n: _d(t) if torch.is_tensor(t) else t for n, t in inp.items()}


def _call_bwd(c, ks, ql, causal=True, q=None, do=None, o=None, lse=None):
    q = c["q"] if q is None else q
    do, o, lse = (c["do"] if do is None else do), (c["o"] if o is None else o), (c["lse"] if lse is None else lse)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(c["k"]), torch.empty_like(c["v"])
    _ops().attn_bwd(do, q, c["k"], c["v"], o, lse, dq, dk, dv, causal, c["scale"], None, None, None, ks, ql)


def test_host_checks_reject_bad_bounds():
    c = _small()
    ks, ql = c["kv_start"], c["q_last"]
    Tq = 20  # S != T: the last 20 queries over all 33 keys
    with pytest.raises(RuntimeError, match="int32"):
        _ops().attn_fwd(c["q"], c["k"], c["v"], True, c["scale"], ks.long())
    with pytest.raises(RuntimeError, match="shape"):
        _ops().attn_fwd(c["q"], c["k"], c["v"], True, c["scale"], ks[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="shape"):
        _ops().attn_fwd(c["q"], c["k"], c["v"], True, c["scale"], ks[:1])
    with pytest.raises(RuntimeError, match="contiguous"):
        _ops().attn_fwd(c["q"], c["k"], c["v"], True, c["scale"], torch.stack([ks, ks], -1)[..., 0])
    with pytest.raises(RuntimeError, match="S == T"):
        _ops().attn_fwd(c["q"][:, -Tq:], c["k"], c["v"], True, c["scale"], ks[:, -Tq:].contiguous())
    with pytest.raises(RuntimeError, match="causal"):
        _ops().attn_fwd(c["q"], c["k"], c["v"], False, c["scale"], ks)
    with pytest.raises(RuntimeError, match="device"):
        _ops().attn_fwd(c["q"], c["k"], c["v"], True, c["scale"], ks.cpu())
    with pytest.raises(RuntimeError, match="int32"):
        _call_bwd(c, ks, ql.long())
    with pytest.raises(RuntimeError, match="shape"):
        _call_bwd(c, ks, ql[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="causal"):
        _call_bwd(c, ks, ql, causal=False)
    with pytest.raises(RuntimeError, match="S == T"):
        _call_bwd(c, ks[:, -Tq:].contiguous(), ql, q=c["q"][:, -Tq:], do=c["do"][:, -Tq:], o=c["o"][:, -Tq:],
                  lse=c["lse"][..., -Tq:].contiguous())
    with pytest.raises(RuntimeError, match="both or neither"):
        _call_bwd(c, ks, None)
    with pytest.raises(RuntimeError, match="both or neither"):
        _call_bwd(c, None, ql)
    torch.cuda.synchronize()


def test_opcheck_of_the_fakes_with_bounds():
    c = _small()
    ks, ql = c["kv_start"], c["q_last"]
    tu = ("test_schema", "test_faketensor")
    torch.library.opcheck(_ops().attn_fwd.default, (c["q"], c["k"], c["v"], True, c["scale"], ks), test_utils=tu)
    dq, dk, dv = torch.empty_like(c["q"]), torch.empty_like(c["k"]), torch.empty_like(c["v"])
    torch.library.opcheck(_ops().attn_bwd.default,
                          (c["do"], c["q"], c["k"], c["v"], c["o"], c["lse"], dq, dk, dv, True, c["scale"]),
                          dict(kv_start=ks, q_last=ql), test_utils=tu)
