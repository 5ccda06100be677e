"""The attention HIP kernels (``attn_fwd``, ``attn_bwd`` with its workspace passes, ``delta=`` and RoPE rotate-back
arms, ``attention_block_bwd``, ``attn_decode``) at tile and mask edges, compared element by element with the fp64
references of ``_attention_refs`` under the budgets calibrated there (``test_attention_refs.py``).  Every check judges
every element: no row, head or tile is left out.

The ops are called through ``torch.ops.pllm`` directly, so the tests control strides and optional arguments."""
import math
import time

import pytest
import torch

import _attention_refs as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
WORST = {}  # op -> (worst element error / its bound, where): printed at the end, information only


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    t0 = time.time()
    yield
    print(f"\nattention edges: {time.time() - t0:.1f} s; worst element, in units of its bound, per output:")
    for op, (r, where) in sorted(WORST.items()):
        print(f"  {op:12s} {r:5.2f}  ({where})")


def _ops():
    return torch.ops.pllm


def _d(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _judge(items, where):
    for op, name, out, ref_unit in items:
        r = A.worst_ratio(op, out, ref_unit)
        if r > WORST.get(op, (-1.0, ""))[0]:
            WORST[op] = (r, f"{where} {name}")
    A.check_all(items)


# ----------------------------------------------------------------------------------------------- forward
# which (T, S) reaches which tile / mask branch: see A.FWD_GEOMS
@pytest.mark.parametrize("case", A.fwd_cases(), ids=str)
def test_attn_fwd_edges(case):
    inp, _ = A.fwd_case(case)
    o, lse = _ops().attn_fwd(_d(inp["q"]), _d(inp["k"]), _d(inp["v"]), inp["causal"], inp["scale"])
    torch.cuda.synchronize()
    out = dict(o=o, lse=lse)
    _judge(A.fwd_checks(case, out), f"fwd {case}")
    if case[0] == "count":
        A.count_facts(case, out)


# ----------------------------------------------------------------------------------------------- backward
def _attn_bwd(inp, ws_mb=None, delta=False):
    """attn_bwd on a case's inputs; ``ws_mb``: the dQ slab workspace for this call (restored afterwards)."""
    do, q, k, v, o, lse = (_d(inp[n]) for n in ("do", "q", "k", "v", "o", "lse"))
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    dl = (do.float() * o.float()).sum(-1).permute(0, 2, 1).contiguous() if delta else None  # [B, H, T] fp32
    try:
        if ws_mb is not None:
            _ops().attn_bwd_set_workspace_mb(ws_mb)
        _ops().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, inp["causal"], inp["scale"], _d(inp["cos"]), _d(inp["sin"]),
                        dl)
        torch.cuda.synchronize()
    finally:
        if ws_mb is not None:
            _ops().attn_bwd_set_workspace_mb(4096)
    return dict(dq=dq, dk=dk, dv=dv)


# D = 32 / 64 run the fused-role kernel, D = 128 the key-stationary one; see A.BWD_GEOMS for the branches.
# one_block: one 256-key block per pass (the fp32 running sum between passes); delta: rowsum(dO o) handed in
@pytest.mark.parametrize("variant", ["default", "one_block", "delta"])
@pytest.mark.parametrize("case", A.bwd_cases(), ids=str)
def test_attn_bwd_edges(case, variant):
    inp, _ = A.bwd_case(case)
    out = _attn_bwd(inp, ws_mb=1e-3 if variant == "one_block" else None, delta=variant == "delta")
    _judge(A.bwd_checks(case, out), f"bwd {variant} {case}")


# the ROT_BACK instantiations: Q / dO staged through registers instead of DMA, dk rotated back before its store and
# dq in the reduce (query t at position t + S - T: an offset into the tables)
@pytest.mark.parametrize("variant", ["default", "one_block"])
@pytest.mark.parametrize("case", A.rope_cases(), ids=str)
def test_attn_bwd_rope_rotate_back_edges(case, variant):
    inp, _ = A.bwd_case(case, "rope")
    out = _attn_bwd(inp, ws_mb=1e-3 if variant == "one_block" else None)
    _judge(A.bwd_checks(case, out, "rope"), f"rope {variant} {case}")


# context parallel: the lse and o of the whole row with one key block of it, causal (the diagonal block) and not
@pytest.mark.parametrize("case", A.partial_cases(), ids=str)
def test_attention_block_bwd_partial_edges(case):
    from pretraining_llm_amd import ops
    inp, _ = A.bwd_case(case, "partial")
    dq, dk, dv = ops.attention_block_bwd(*(_d(inp[n]) for n in ("do", "q", "k", "v", "o", "lse")),
                                         causal=inp["causal"], scale=inp["scale"])
    torch.cuda.synchronize()
    _judge(A.bwd_checks(case, dict(dq=dq, dk=dk, dv=dv), "partial"), f"partial {case}")


# ----------------------------------------------------------------------------------------------- decode
# group sizes, key counts and split counts: see A.decode_cases
@pytest.mark.parametrize("case", A.decode_cases(), ids=str)
def test_attn_decode_edges(case):
    D, Hq, Hkv, Bb, S, counts = case
    inp, ref = A.decode_case(case)
    if counts is None:
        seqlen = None
    elif isinstance(counts, int):
        seqlen = torch.tensor([counts], dtype=torch.int32, device=DEV)  # a device scalar smaller than the buffer
    else:
        seqlen = torch.tensor(counts, dtype=torch.int32, device=DEV)    # one count per sequence
    o = _ops().attn_decode(_d(inp["q"]), _d(inp["k"]), _d(inp["v"]), inp["scale"], seqlen)
    torch.cuda.synchronize()
    assert o.shape == (Bb, 1, Hq, D)
    _judge([("decode_o", "o", o, ref)], f"decode {case}")
    for b, n in enumerate(inp["counts"]):
        if n == 0:  # no key: exact zeros, no NaN
            assert not _bits(o[b]).any()


# ----------------------------------------------------------------------------------------------- memory independence
# The documented contract: rows past the range read as zeros through the descriptor range or an explicit guard, every
# read stays inside the tensors' own rows, every write inside the output views.  The inputs are views into larger
# buffers whose every element outside the view is NaN, the gradients go into views of a buffer pre-filled with a bit
# pattern; the results must equal, bit for bit, those of the same call on compact copies.
PATTERN = 0x3C5A  # a finite bf16 (about 0.0133)


def _nan_view(t, pad_rows, pad_heads):
    """``t`` [B, L, Hx, D] as a view of a NaN-filled [B, L + pad_rows, Hx + pad_heads, D] buffer: NaN rows past L
    (which also pad the batches apart) and NaN heads between the rows."""
    Bb, L, Hx, D = t.shape
    buf = torch.full((Bb, L + pad_rows, Hx + pad_heads, D), math.nan, dtype=t.dtype, device=DEV)
    view = buf[:, :L, :Hx]
    view.copy_(t)
    return view


def _pattern_views(shapes):
    """Views of the given [B, L, Hx, D] shapes, each inside its own pattern-filled buffer with spare rows and heads;
    returns (views, check) where check() asserts that nothing outside the views was written."""
    bufs, views = [], []
    for (Bb, L, Hx, D) in shapes:
        buf = torch.full((Bb, L + 3, Hx + 1, D), PATTERN, dtype=torch.int16, device=DEV)
        bufs.append(buf)
        views.append(buf.view(BF16)[:, :L, :Hx])

    def check():
        for buf, (Bb, L, Hx, D) in zip(bufs, shapes):
            outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
            outside[:, :L, :Hx] = False
            assert (buf[outside] == PATTERN).all(), "a write outside the output view"
    return views, check


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: strided / NaN-padded call differs from the compact one"


def _fwd_bwd_compact(inp):
    """Forward and backward on compact device copies; returns the device tensors."""
    q, k, v, do = (_d(inp[n]).contiguous() for n in ("q", "k", "v", "do"))
    o, lse = _ops().attn_fwd(q, k, v, inp["causal"], inp["scale"])
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _ops().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, inp["causal"], inp["scale"])
    torch.cuda.synchronize()
    assert all(torch.isfinite(t.float()).all() for t in (o, lse, dq, dk, dv))
    return dict(q=q, k=k, v=v, do=do, o=o, lse=lse, dq=dq, dk=dk, dv=dv)


# T = 75, S = 203: ragged sub-block, key tile and key block, offset 128
@pytest.mark.parametrize("D,Hkv", [(32, 1), (64, 4), (128, 2)])
def test_attention_reads_and_writes_stay_inside_padded_views(D, Hkv):
    inp = A.attn_inputs("randn", 75, 203, 1, D, Hkv)
    c = _fwd_bwd_compact(inp)
    q, k, v, do, o_in = (_nan_view(c[n], 5, 1) for n in ("q", "k", "v", "do", "o"))
    o, lse = _ops().attn_fwd(q, k, v, True, inp["scale"])
    _same_bits(o, c["o"], "o")
    _same_bits(lse, c["lse"], "lse")
    (dq, dk, dv), check = _pattern_views([q.shape, k.shape, v.shape])
    _ops().attn_bwd(do, q, k, v, o_in, c["lse"], dq, dk, dv, True, inp["scale"])
    torch.cuda.synchronize()
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        _same_bits(t, c[n], n)
    check()


# the packed [q | k | v] rows of ops._split_qkv (T = S = 203), with NaN rows appended and NaN columns after v
@pytest.mark.parametrize("D,Hkv", [(32, 2), (64, 1), (128, 4)])
def test_attention_packed_qkv_layout_with_nan_rows(D, Hkv):
    from pretraining_llm_amd import ops
    T = 203
    inp = A.attn_inputs("randn", T, T, 1, D, Hkv)
    c = _fwd_bwd_compact(inp)
    W = (A.H + 2 * Hkv) * D
    big = torch.full((A.B, T + 3, W + 8), math.nan, dtype=BF16, device=DEV)
    qkv = big[:, :T, :W]
    q, k, v = ops._split_qkv(qkv, A.H, Hkv, D)
    q.copy_(c["q"]), k.copy_(c["k"]), v.copy_(c["v"])
    o, lse = _ops().attn_fwd(q, k, v, True, inp["scale"])
    _same_bits(o, c["o"], "o")
    _same_bits(lse, c["lse"], "lse")
    gbuf = torch.full((A.B, T + 3, W + 8), PATTERN, dtype=torch.int16, device=DEV)
    dq, dk, dv = ops._split_qkv(gbuf.view(BF16)[:, :T, :W], A.H, Hkv, D)
    _ops().attn_bwd(_nan_view(c["do"], 2, 0), q, k, v, _nan_view(c["o"], 2, 0), c["lse"], dq, dk, dv, True,
                    inp["scale"])
    torch.cuda.synchronize()
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        _same_bits(t, c[n], n)
    assert (gbuf[:, T:] == PATTERN).all() and (gbuf[:, :, W:] == PATTERN).all(), "a write outside the packed rows"


# a KV cache with NaN rows past S and a NaN head between the rows; S from the shape and one count per sequence
@pytest.mark.parametrize("D,Hq,Hkv", [(32, 8, 8), (64, 8, 2), (128, 8, 1)])
def test_attn_decode_reads_stay_inside_the_cache_view(D, Hq, Hkv):
    inp, _ = A.decode_case((D, Hq, Hkv, 2, 203, None))
    q, k, v = (_d(inp[n]).contiguous() for n in ("q", "k", "v"))
    counts = torch.tensor([203, 77], dtype=torch.int32, device=DEV)
    qv, kv, vv = _nan_view(q, 0, 1), _nan_view(k, 9, 1), _nan_view(v, 9, 1)
    for seqlen in (None, counts):
        want = _ops().attn_decode(q, k, v, inp["scale"], seqlen)
        got = _ops().attn_decode(qv, kv, vv, inp["scale"], seqlen)
        torch.cuda.synchronize()
        assert torch.isfinite(want.float()).all()
        _same_bits(got, want, "decode o")
