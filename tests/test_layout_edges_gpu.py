"""The gather, layout and merge HIP kernels (embedding forward / backward, RoPE, batched transpose, LSE merge,
``bias_grad``, ``scale_``) at the shapes where their index arithmetic, chunk carries and dispatch arms change,
compared element by element with the fp64 references of ``_layout_refs`` under the budgets calibrated there
(``test_layout_refs.py``), bitwise wherever the arithmetic makes the result derivable; and the host checks that
keep a bad argument from reaching a kernel.

Every op is called through ``torch.ops.pllm`` directly, so the tests control strides and optional arguments."""
import math

import pytest
import torch

import _layout_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _ops():
    return torch.ops.pllm


def _d(t):
    return None if t is None else t.to(DEV)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(R.bits(a), R.bits(b)), f"{what}: bits differ"


# ----------------------------------------------------------------------------------------------- embedding forward
# which shape reaches what: see R.EMB_FWD_SHAPES
@pytest.mark.parametrize("case", R.embed_fwd_cases(), ids=lambda c: "-".join(map(str, c)))
def test_embedding_fwd_edges(case):
    inp = R.embed_fwd_inputs(*case)
    out = _ops().embedding_fwd(_d(inp["idx"]), _d(inp["wte"]), _d(inp["wpe"]), inp["pos_offset"]).cpu()
    ref, unit = R.embed_fwd_ref(**inp)
    want = R.rne_bf16(ref)  # the exact family: one rounding of an exact fp32 sum
    B, T, C = out.shape
    rows_o, rows_w = out.reshape(B * T, C), want.reshape(B * T, C)
    if B * T > R.EMB_FWD_WRAP_FIRST_ROW:  # the rows of the grid's second pass, on their own
        _same_bits(rows_o[R.EMB_FWD_WRAP_FIRST_ROW:], rows_w[R.EMB_FWD_WRAP_FIRST_ROW:], "rows past the grid")
        assert rows_w[R.EMB_FWD_WRAP_FIRST_ROW:].any()
    _same_bits(out, want, "embedding forward")
    R.check("embed_fwd", out, (want.to(F64), unit), "out")
    # out-of-range ids read a zero row: nothing, or the position's row alone
    i = inp["idx"].reshape(-1).long()
    bad = (i < 0) | (i >= inp["wte"].shape[0])
    assert int(bad.sum()) == 3
    if inp["wpe"] is None:
        assert not R.bits(rows_o[bad]).any()
        _same_bits(rows_o[~bad], inp["wte"][i[~bad]], "a pure gather copies bits")
    else:
        t = bad.nonzero().flatten() % T + inp["pos_offset"]
        _same_bits(rows_o[bad], inp["wpe"][t], "wpe row alone")


# ----------------------------------------------------------------------------------------------- embedding backward
def _embed_bwd(inp, target):
    dx, idx = _d(inp["dx"]), _d(inp["idx"])
    ft, fp, _ = R.embed_bwd_fills(inp, target)
    if target == "fresh":
        dwte, dwpe = _ops().embedding_bwd(dx, idx, inp["V"], inp["n_pos"], True)
    else:
        dwte, dwpe = _d(ft).clone(), _d(fp).clone()
        _ops().embedding_bwd_acc(dx, idx, inp["V"], inp["n_pos"], True, dwte, dwpe)
    return dict(dwte=dwte.cpu(), dwpe=dwpe.cpu()), ft, fp


# which plan reaches which relation of a run to the chunk grid: see R.EMB_BWD_PLANS
@pytest.mark.parametrize("family", R.EMB_BWD_FAMILIES)
@pytest.mark.parametrize("plan,C", R.EMB_BWD_CASES, ids=lambda v: str(v))
def test_embedding_bwd_edges(plan, C, family):
    inp = R.embed_bwd_inputs(plan, C, family)
    te, pe = R.embed_bwd_untouched(inp["idx"], inp["V"], inp["n_pos"])
    for target in R.EMB_BWD_TARGETS:
        out, ft, fp = _embed_bwd(inp, target)
        R.check_all(R.embed_bwd_checks(inp, target, out))
        # rows of ids that do not occur, and positions past T, keep their bits
        _same_bits(out["dwte"][te], ft[te], f"{target}: dwte rows of absent ids")
        _same_bits(out["dwpe"][pe], fp[pe], f"{target}: dwpe rows t >= T")
        again, _, _ = _embed_bwd(inp, target)
        for k in out:
            _same_bits(out[k], again[k], f"{target}: {k} of a second call")
    # without positions: the same dwte, and no dwpe
    dwte, dwpe = _ops().embedding_bwd(_d(inp["dx"]), _d(inp["idx"]), inp["V"], 0, False)
    fresh, _, _ = _embed_bwd(inp, "fresh")
    _same_bits(dwte.cpu(), fresh["dwte"], "dwte without positions")
    assert dwpe.numel() == 0


# ----------------------------------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("T", R.ROPE_T)
@pytest.mark.parametrize("D", R.ROPE_D)
def test_rope_edges(D, T):
    for nh, n_rot in R.ROPE_HEADS:
        for po in (0, 3):
            inp = R.rope_inputs(D, nh, T, po)
            x, cos, sin = _d(inp["x"]), _d(inp["cos"]), _d(inp["sin"])
            kw = dict(nh=nh, n_rot=n_rot, T=T, pos_offset=po)
            what = f"{nh}/{n_rot} +{po}"
            outs = {}
            for inv in (False, True):
                out = outs[inv] = _ops().rope(x, cos, sin, nh, n_rot, T, po, inv)
                assert out.shape == x.shape and out.data_ptr() != x.data_ptr()
                R.check("rope", out, R.rope_ref(**inp, **kw, inverse=inv), f"{what} inverse={inv}")
                # the copied (v) heads, bit for bit
                _same_bits(out.reshape(-1, nh, D)[:, n_rot:].cpu(), inp["x"].reshape(-1, nh, D)[:, n_rot:], what)
            assert n_rot == 0 or not torch.equal(outs[False], outs[True])
            back = _ops().rope(outs[False], cos, sin, nh, n_rot, T, po, True)
            R.check("rope_rt", back, R.rope_roundtrip_ref(**inp, **kw), what)
            if n_rot and po == 0:  # the compacted layout is the leading columns of the full one
                qk = _ops().rope_qk(x, cos, sin, nh, n_rot, T)
                assert qk.shape == x.shape[:-1] + (n_rot * D,) and qk.is_contiguous()
                _same_bits(qk.cpu(), outs[False][..., :n_rot * D].cpu(), f"rope_qk {what}")
                R.check("rope", qk, R.rope_ref(**inp, **kw, out_heads=n_rot), f"rope_qk {what}")


@pytest.mark.parametrize("D", R.ROPE_D)
def test_rope_reads_the_row_of_its_position(D):
    """Tables that are the identity in every row but one, which swaps the halves: each (row, pos_offset) pair
    must turn exactly the tokens at that position and copy the others, bit for bit."""
    nh, n_rot, T, po = 4, 3, 5, 3
    inp = R.rope_inputs(D, nh, T, po)
    x = inp["x"].reshape(R.ROPE_B, T, nh, D)
    for t in range(T):
        cos, sin = R.marker_tables(T + po + 2, D, po + t)
        out = _ops().rope(_d(inp["x"]), _d(cos), _d(sin), nh, n_rot, T, po, False).cpu().reshape(x.shape)
        keep = torch.arange(T) != t
        _same_bits(out[:, keep], x[:, keep], f"t={t}: the other positions")
        _same_bits(out[:, t, n_rot:], x[:, t, n_rot:], f"t={t}: copied heads")
        assert torch.equal(out[:, t, :n_rot, :D // 2], -x[:, t, :n_rot, D // 2:])
        assert torch.equal(out[:, t, :n_rot, D // 2:], x[:, t, :n_rot, :D // 2])
    # a marker outside [pos_offset, pos_offset + T) is never read
    for row in (po - 1, po + T):
        cos, sin = R.marker_tables(T + po + 2, D, row)
        out = _ops().rope(_d(inp["x"]), _d(cos), _d(sin), nh, n_rot, T, po, False)
        _same_bits(out.cpu(), inp["x"], f"marker in row {row}")


# ----------------------------------------------------------------------------------------------- batched transpose
SENTINEL = -7.0
GUARD = 64  # elements (128 B) on either side of each dst


def _transpose(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    srcs = [torch.randn(s, generator=g).to(BF16) for s in shapes]
    bufs = [torch.full((r * c + 2 * GUARD,), SENTINEL, device=DEV, dtype=BF16) for r, c in shapes]
    dsts = [b[GUARD:GUARD + r * c].view(c, r) for b, (r, c) in zip(bufs, shapes)]
    dev = [_d(s) for s in srcs]
    tiles = R.transpose_tile_total(shapes)
    _ops().transpose_run(_ops().transpose_plan(dev, dsts), tiles)
    torch.cuda.synchronize()
    for i, (s, sd, d, b) in enumerate(zip(srcs, dev, dsts, bufs)):
        _same_bits(d.cpu(), s.t().contiguous(), f"matrix {i} {tuple(s.shape)}")
        guards = torch.cat([b[:GUARD], b[-GUARD:]]).cpu()
        assert (guards == SENTINEL).all(), f"matrix {i}: guard bytes written"
        _same_bits(sd.cpu(), s, f"matrix {i}: the source")
    return tiles


def test_transpose_persistent_loop_second_tiles():
    """More tiles than workgroups: every workgroup takes a second tile, found by continuing its table scan, most of
    them in another matrix than the first, the ragged ones after a full tile (see R.TRANSPOSE_PLAN)."""
    tiles = R.transpose_tile_total(R.TRANSPOSE_PLAN)
    assert tiles == R.TRANSPOSE_TILES and 2 * R.TRANSPOSE_GRID > tiles > R.TRANSPOSE_GRID
    assert _transpose(R.TRANSPOSE_PLAN, 31) == tiles


def test_transpose_single_tile():
    assert _transpose(((8, 8),), 32) == 1


# ----------------------------------------------------------------------------------------------- LSE merge
@pytest.mark.parametrize("T", R.LSE_T)
@pytest.mark.parametrize("D", R.LSE_D)
def test_lse_merge_edges(D, T):
    """o_acc / lse_acc as views of larger buffers (a T-chunk, padded head rows), o with padded head rows, lse
    transposed: every stride of the twelve differs from the contiguous one."""
    inp = R.lse_inputs(D, T)
    B, H = R.LSE_B, R.LSE_H
    ofull = torch.full((B, T + 4, H, D + 8), 3.25, device=DEV)
    o_acc = ofull[:, 2:2 + T, :, :D]
    o_acc.copy_(inp["o_acc"])
    lfull = torch.full((B, H, T + 2), 3.25, device=DEV)
    lse_acc = lfull[:, :, 1:1 + T]
    lse_acc.copy_(inp["lse_acc"])
    opad = torch.full((B, T, H, D + 8), 3.25, device=DEV, dtype=BF16)
    o = opad[..., :D]
    o.copy_(inp["o"])
    lse = _d(inp["lse"]).transpose(1, 2).contiguous().transpose(1, 2)  # [B, H, T] with strides (T H, 1, H)
    assert lse.stride() == (T * H, 1, H) and not o_acc.is_contiguous() and not o.is_contiguous()
    before = [t.clone() for t in (ofull, lfull, opad, lse)]
    _ops().lse_merge_(o_acc, lse_acc, o, lse)
    torch.cuda.synchronize()
    R.check_all(R.lse_merge_checks(inp, dict(o_acc=o_acc, lse_acc=lse_acc)))
    # both -inf: lse_acc stays -inf, o_acc is exactly 0; nothing anywhere is NaN
    both = inp["kind"] == 3
    assert (lse_acc.cpu()[both] == -math.inf).all() and not o_acc.cpu()[both.transpose(1, 2)].any()
    assert not torch.isnan(o_acc).any() and not torch.isnan(lse_acc).any()
    # the rest of the accumulators' buffers and the inputs keep their bits
    for full, view, b4 in ((ofull, o_acc, before[0]), (lfull, lse_acc, before[1])):
        view.copy_(b4[(slice(None), slice(2, 2 + T), slice(None), slice(0, D)) if full is ofull else
                      (slice(None), slice(None), slice(1, 1 + T))])
        _same_bits(full.cpu(), b4.cpu(), "outside the accumulator's view")
    _same_bits(opad.cpu(), before[2].cpu(), "o")
    _same_bits(lse.cpu(), before[3].cpu(), "lse")


# ----------------------------------------------------------------------------------------------- bias_grad
# which N reaches which colsum_groups arm: see R.BIAS_GRAD_N
@pytest.mark.parametrize("family", ["exact", "randn"])
@pytest.mark.parametrize("N,C", R.bias_grad_cases())
def test_bias_grad_edges(N, C, family):
    dy = R.bias_grad_inputs(N, C, family)
    x = _d(dy)
    for target in ("fresh", "f32", "bf16"):
        if target == "fresh":
            out = _ops().bias_grad(x, None)
            assert out.dtype == BF16 and out.shape == (C,)
        else:
            out = _d(R.acc_fill((C,), family, F32 if target == "f32" else BF16)).clone()
            ret = _ops().bias_grad(x, out)
            assert ret.numel() == 0
        R.check_all(R.bias_grad_checks(dy, family, target, out))
    _same_bits(x.cpu(), dy, "dy")


# ----------------------------------------------------------------------------------------------- scale_
@pytest.mark.parametrize("numel", R.SCALE_NUMEL)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_scale_inplace_edges(dtype, numel):
    xc = R.scale_inputs(dtype, numel)
    for s in R.SCALE_S + (0.0,):
        x = _d(xc).clone()
        _ops().scale_(x, torch.tensor([s], device=DEV, dtype=F32))
        R.assert_same_bits(x, R.scale_ref(xc, s), f"s={s}")
    # s = 0: signed zeros; inf and NaN give NaN
    fin = torch.isfinite(xc)
    z = x.cpu()
    assert not z[fin].any() and torch.equal(torch.signbit(z[fin]), torch.signbit(xc[fin]))
    assert torch.isnan(z[~fin]).all()
    # s = 1: no bit changes, NaN payloads and -0 included
    x = _d(xc).clone()
    _ops().scale_(x, torch.ones(1, device=DEV, dtype=F32))
    _same_bits(x.cpu(), xc, "s=1")


# ----------------------------------------------------------------------------------------------- host checks
def _rope_args(D=32, nh=4, T=5, po=3):
    inp = R.rope_inputs(D, nh, T, po)
    return _d(inp["x"]), _d(inp["cos"]), _d(inp["sin"]), nh, T, po


def test_rope_rejects_bad_tables_and_offsets():
    """Each of these would read a table or x out of bounds; all raise on the host, before any launch."""
    x, cos, sin, nh, T, po = _rope_args()
    _ops().rope(x, cos, sin, nh, nh, T, po, False)  # the valid call
    with pytest.raises(RuntimeError, match="cos and sin"):  # a shorter sin table
        _ops().rope(x, cos, sin[:T].contiguous(), nh, nh, T, po, False)
    with pytest.raises(RuntimeError, match="cos and sin"):
        _ops().rope_qk(x, cos, sin[:T].contiguous(), nh, nh, T)
    with pytest.raises(RuntimeError, match="cos and sin"):  # table rank
        _ops().rope(x, cos[None], sin[None], nh, nh, T, po, False)
    with pytest.raises(RuntimeError, match="cos and sin"):
        _ops().rope_qk(x, cos.reshape(-1), sin.reshape(-1), nh, nh, T)
    with pytest.raises(RuntimeError, match="device"):
        _ops().rope(x, cos.cpu(), sin.cpu(), nh, nh, T, po, False)
    with pytest.raises(RuntimeError, match="device"):
        _ops().rope_qk(x, cos, sin.cpu(), nh, nh, T)
    with pytest.raises(RuntimeError, match="pos_offset"):  # passes the size check, reads before the table
        _ops().rope(x, cos, sin, nh, nh, T, -1, False)
    with pytest.raises(RuntimeError, match="table shape"):
        _ops().rope(x, cos, sin, nh, nh, T, po + 3, False)
    for n_rot in (-1, nh + 1):
        with pytest.raises(RuntimeError, match="n_rot"):
            _ops().rope(x, cos, sin, nh, n_rot, T, po, False)
    for n_rot in (0, nh + 1):
        with pytest.raises(RuntimeError, match="heads"):
            _ops().rope_qk(x, cos, sin, nh, n_rot, T)
    # x 2 bytes off a 16-byte boundary
    buf = torch.zeros(x.numel() + 8, device=DEV, dtype=BF16)
    off = buf[1:1 + x.numel()].view(x.shape)
    assert off.is_contiguous() and off.data_ptr() % 16 == 2
    with pytest.raises(RuntimeError, match="aligned"):
        _ops().rope(off, cos, sin, nh, nh, T, po, False)
    with pytest.raises(RuntimeError, match="aligned"):
        _ops().rope_qk(off, cos, sin, nh, nh, T)


def test_embedding_rejects_bad_offsets_and_ranks():
    inp = R.embed_fwd_inputs(3, 7, 264, 11, 1, 5, "int64")
    idx, wte, wpe = _d(inp["idx"]), _d(inp["wte"]), _d(inp["wpe"])
    _ops().embedding_fwd(idx, wte, wpe, 5)  # the valid call
    with pytest.raises(RuntimeError, match="pos_offset"):  # passes the wpe size check, reads before the table
        _ops().embedding_fwd(idx, wte, wpe, -1)
    with pytest.raises(RuntimeError, match="pos_offset"):
        _ops().embedding_fwd(idx, wte, None, -1)
    with pytest.raises(RuntimeError, match="wpe shape"):
        _ops().embedding_fwd(idx, wte, wpe, 8)
    with pytest.raises(RuntimeError, match="wte must be"):
        _ops().embedding_fwd(idx, wte.reshape(-1), wpe, 0)
    with pytest.raises(RuntimeError, match="wte must be"):
        _ops().embedding_fwd(idx, wte[None], wpe, 0)
    with pytest.raises(RuntimeError, match=r"\[B, T\]"):
        _ops().embedding_fwd(idx.reshape(-1), wte, wpe, 0)
    dx = torch.zeros(3, 7, 264, device=DEV, dtype=BF16)
    _ops().embedding_bwd(dx, idx, 11, 9, True)  # the valid call
    for bad in (idx.reshape(-1), idx[None]):
        with pytest.raises(RuntimeError, match=r"idx must be \[B, T\]"):
            _ops().embedding_bwd(dx, bad, 11, 9, True)
        with pytest.raises(RuntimeError, match=r"idx must be \[B, T\]"):
            _ops().embedding_bwd_acc(dx, bad, 11, 9, False, torch.zeros(11, 264, device=DEV), None)
