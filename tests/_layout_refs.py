"""fp64 references, case builders and budgets for the gather, layout and merge kernels: the embedding
(forward, and the chunked backward over sorted ids), RoPE (``rope`` / ``rope_qk``), the batched transpose, ring
attention's LSE merge, the standalone bias gradient (``bias_grad``) and the in-place ``scale_``.

Not collected by pytest.  ``test_layout_refs.py`` (CPU) checks the references against independent double-precision
paths, calibrates the budgets below and shows which defects the bound rejects; ``test_layout_edges_gpu.py`` runs
the HIP kernels on the same cases under the same bounds.

The bound is the one of ``_streaming_refs``: every element must satisfy

    |out - ref| <= budget * (ulp_out(ref) + unit)

with ``unit`` = 2^-23 times the magnitudes the kernel sums in fp32 (documented at each reference).  ``measured`` is
the smallest integer budget at which a CPU fp32 model of the op -- in the kernel's documented operation order;
where the compiler may contract ``a c - b s`` into an FMA, the larger of the fused and unfused models -- passes on
all of the op's cases; ``budget`` is twice that.  For the LSE merge the doubling is also what covers ``__expf`` /
``log1pf`` (v_exp_f32 / v_log_f32 at about 1 fp32 ulp instead of correctly rounded functions, as for
``gelu_fwd``), and its units carry the exponent's argument (the rounding of ``x log2 e`` scales with ``|x|``) and a
flushed weight below 2^-126.  Budget 0 (``exact``) wherever the arithmetic makes the result derivable: those
checks pin the rounding mode and catch a single wrong element.  Filled from ``pytest tests/test_layout_refs.py``
(which fails when a row is stale); nothing here was tuned against kernel output.

    op            measured  budget   outputs
    ------------  --------  ------   ---------------------------------------------------------------------
    embed_fwd            0       0   out (bf16): the exact family, bf16_rne(wte[idx] + wpe[t + pos_offset])
    embed_bwd            1       2   dwte, dwpe (fresh bf16; fp32 / bf16 targets), the randn family
    rope                 1       2   rope, rope_qk (bf16)
    rope_rt              1       2   inverse(forward(x)) against x (bf16)
    lse_merge_o          1       2   o_acc (fp32)
    lse_merge_lse        1       2   lse_acc (fp32)
    bias_grad            1       2   bias_grad (fresh bf16; fp32 / bf16 targets): the ``colsum`` row of
                                     ``_streaming_refs``, measured again on these cases
    exact                0       0   integer families of embed_bwd / bias_grad, copied RoPE heads, scale_,
                                     the transpose

The batched-transpose plan ``TRANSPOSE_PLAN`` totals 4029 tiles of 64 x 64 (> 2048 workgroups: every workgroup
takes a second tile).  ``test_layout_edges_gpu.py`` (88 tests) took 3.6 s of wall time on an MI355X, the slowest
test 0.4 s.  Every kernel passed on its first run: the tests forced no kernel change, only the host checks of
``rope`` / ``rope_qk`` / ``embedding_fwd`` / ``embedding_bwd`` that ``test_layout_edges_gpu.py`` lists at its end.
"""
from __future__ import annotations

import math

import torch

import _streaming_refs as S
from _streaming_refs import BF16, F32, F64, E32, FLUSH, EPS_OUT, _gen, assert_close_ulps, ulps_needed, colsum_ref

# op -> (measured, budget); see the table above
BUDGET = {
    "embed_fwd": (0, 0),
    "embed_bwd": (1, 2),
    "rope": (1, 2),
    "rope_rt": (1, 2),
    "lse_merge_o": (1, 2),
    "lse_merge_lse": (1, 2),
    "bias_grad": (1, 2),
    "exact": (0, 0),
}


def check(op, out, ref_unit, what, fmt=None):
    """``out`` against a reference ``(ref64, unit)`` under the op's budget."""
    ref, unit = ref_unit
    u = BUDGET[op][1]
    assert_close_ulps(out, ref, u, u * torch.as_tensor(unit, dtype=F64), what=f"{op}/{what}", fmt=fmt)


def check_all(items):
    """``items``: (op, name, out, (ref64, unit)) tuples as the ``*_checks`` functions below return."""
    for op, name, out, ref_unit in items:
        check(op, out, ref_unit, name)


def bits(t):
    """The bit patterns of a bf16 / fp32 tensor (NaN payloads and the sign of zero compare too)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def rne_bf16(x64):
    """An fp64 value that fp32 holds exactly, rounded to bf16 (nearest even) -- what the kernels' one cast gives."""
    assert torch.equal(x64.to(F32).to(F64), x64), "not exact in fp32"
    return x64.to(F32).to(BF16)


def rounded(x64, dtype):
    return rne_bf16(x64) if dtype == BF16 else x64.to(F32)


def acc_fill(shape, family, dtype, base=0):
    """A non-zero accumulation target.  exact: integers (fp32: about 1000, so that the tensor's norm hides a lost
    partial sum from a norm ratio; bf16: |.| <= 8); randn: 1.5 + 0.01 k rounded to the dtype."""
    n = math.prod(shape)
    k = torch.arange(n, dtype=F64) + base
    if family == "exact":
        v = (1000 + k % 17) if dtype == F32 else (k % 17 - 8)
    else:
        v = 1.5 + 0.01 * (k % 997)
    return v.reshape(shape).to(dtype)


def _fma_models(p, q, r, s, sign):
    """p q + sign r s as fp32 hardware may evaluate it: both products rounded; or either one kept exact inside an
    FMA (a bf16 / fp32 by fp32 product is exact in fp64)."""
    p32, q32, r32, s32 = (t.to(F32) for t in (p, q, r, s))
    p64, q64, r64, s64 = (t.to(F64) for t in (p, q, r, s))
    return [p32 * q32 + sign * (r32 * s32),
            (p64 * q64 + sign * (r32 * s32).to(F64)).to(F32),
            ((p32 * q32).to(F64) + sign * (r64 * s64)).to(F32)]


# ------------------------------------------------------------------------------------------------ embedding forward
# (B, T, C, V).  C = 8: one vector per row; 264: 33 vectors; (2, 2050, 2048): N C / 8 = 4100 * 256 work items, over
# the grid's 4096 * 256 threads, so the grid-stride loop wraps for the last four rows
EMB_FWD_SHAPES = ((2, 5, 8, 11), (3, 7, 264, 11), (2, 2050, 2048, 64))
EMB_FWD_WRAP_FIRST_ROW = 4096  # rows from here on belong to the second pass of the grid


def embed_fwd_cases():
    """(B, T, C, V, with_wpe, pos_offset, idx_dtype); the wrap shape on two of the six combinations."""
    out = []
    for shape in EMB_FWD_SHAPES[:2]:
        for wpe, po in ((0, 0), (1, 0), (1, 5)):
            for dt in ("int32", "int64"):
                out.append(shape + (wpe, po, dt))
    out += [EMB_FWD_SHAPES[2] + (1, 5, "int64"), EMB_FWD_SHAPES[2] + (0, 0, "int32")]
    return out


def embed_fwd_inputs(B, T, C, V, with_wpe, pos_offset, idx_dtype):
    """The exact family: wte integers |.| <= 255 and wpe eighths of such integers -- both exact in bf16, their sum
    exact in fp32 (11 bits and more: it needs the rounding to bf16, ties included).  wpe is two rows longer than
    T + pos_offset.  Ids -1, V, V + 3 (out of range) at positions 1, N / 2, N - 2."""
    g = _gen(11, B, T, C, V, with_wpe, pos_offset)
    wte = torch.randint(-255, 256, (V, C), generator=g).to(F64).to(BF16)
    wpe = (torch.randint(-255, 256, (T + pos_offset + 2, C), generator=g).to(F64) / 8).to(BF16) if with_wpe else None
    idx = torch.randint(0, V, (B * T,), generator=g)
    n = B * T
    idx[1], idx[n // 2], idx[n - 2] = -1, V, V + 3
    return dict(idx=idx.reshape(B, T).to(getattr(torch, idx_dtype)), wte=wte, wpe=wpe, pos_offset=pos_offset)


def embed_fwd_ref(idx, wte, wpe, pos_offset, **_):
    """wte[idx] (a zero row for an id outside [0, V)) + wpe[t + pos_offset]; one fp32 sum: no unit."""
    V, T = wte.shape[0], idx.shape[1]
    i = idx.long()
    ok = (i >= 0) & (i < V)
    rows = torch.where(ok[..., None], wte.to(F64)[i.clamp(0, V - 1)], torch.zeros((), dtype=F64))
    if wpe is not None:
        rows = rows + wpe.to(F64)[pos_offset:pos_offset + T][None]
    return rows, 0.0


def embed_fwd_model_f32(idx, wte, wpe, pos_offset, defect=None, **_):
    """``defect``: no_offset (wpe row t instead of t + pos_offset); truncate (fp32 -> bf16 by truncation)."""
    V, T = wte.shape[0], idx.shape[1]
    i = idx.long()
    ok = (i >= 0) & (i < V)
    rows = torch.where(ok[..., None], wte[i.clamp(0, V - 1)], torch.zeros((), dtype=BF16))
    if wpe is None:
        return rows
    po = 0 if defect == "no_offset" else pos_offset
    s = rows.float() + wpe.float()[po:po + T][None]
    if defect == "truncate":
        return (s.view(torch.int32) & -65536).view(F32).to(BF16)
    return s.to(BF16)


# ------------------------------------------------------------------------------------------------ embedding backward
EK = 64  # sorted positions per chunk (embedding.hip)

# name -> (V, B, T, runs of the SORTED order as (id, length)).  Chunks are [64 j, 64 j + 64).
EMB_BWD_PLANS = {
    # -3: 0..69, an out-of-range run across the end of chunk 0; -1: 70..79; 0: 80..99, wholly inside chunk 1;
    # 1: 100..127, ends exactly on the chunk's end with another id next; 3: 128..200, starts exactly on a chunk's
    # start, crosses its end and ends inside chunk 3 (a run that crosses a start and ends inside); 4: 201..210;
    # 5: 211..460, starts inside chunk 3, covers chunks 4, 5, 6 whole (head-only chunks) and ends inside chunk 7;
    # 7: 461..511, ends on a chunk's end; 8: 512..575, exactly chunk 8; 9: 576..580; 12 = V: 581..650, out of range
    # across the end of chunk 9; 15 = V + 3: 651..699, out of range up to N = 700 (chunk 10 is partial).
    # Ids 2, 6, 10, 11 do not occur.
    "runs": (12, 4, 175, ((-3, 70), (-1, 10), (0, 20), (1, 28), (3, 73), (4, 10), (5, 250), (7, 51), (8, 64), (9, 5),
                          (12, 70), (15, 49))),
    # N = 200, no multiple of 64: 1: 0..39; 2: 40..127, starts inside chunk 0 and ends exactly on the end of chunk 1
    # with another id next (a head that closes its run); 5: 128..199, across one end, reaching N in a partial chunk
    "tail": (7, 2, 100, ((1, 40), (2, 88), (5, 72))),
    "one": (5, 1, 1, ((3, 1),)),                      # N = 1
    "chunk": (6, 2, 32, ((1, 30), (4, 34))),          # N = 64 exactly: one whole chunk, nothing crosses
    "same": (4, 3, 100, ((2, 300),)),                 # one id everywhere: 4 whole chunks and a partial one
}
EMB_BWD_C = (8, 264)  # cv = 1 and 33: one 64-thread workgroup, one / 33 of its threads at work
# (plan, C); C = 2056: cv = 257, the 256-thread workgroup whose threads loop (thread 0 takes a second vector)
EMB_BWD_CASES = tuple((p, C) for p in EMB_BWD_PLANS for C in EMB_BWD_C) + (("tail", 2056),)
EMB_BWD_FAMILIES = ("exact", "randn")
EMB_BWD_TARGETS = ("fresh", "f32", "bf16")


def embed_bwd_inputs(plan, C, family):
    """Token positions shuffled, so that the stable sort's ``perm`` is no identity.  exact: integer dx, |.| <= 3 (a
    sum of up to 300 of them is exact in fp32 and needs the rounding to bf16); n_pos = T + 3."""
    V, B, T, runs = EMB_BWD_PLANS[plan]
    N = B * T
    assert sum(n for _, n in runs) == N and list(runs) == sorted(runs)
    g = _gen(12, list(EMB_BWD_PLANS).index(plan), C, family == "exact")
    ids = torch.cat([torch.full((n,), i) for i, n in runs])
    flat = torch.empty(N, dtype=torch.long)
    flat[torch.randperm(N, generator=g)] = ids
    if family == "exact":
        dx = torch.randint(-3, 4, (B, T, C), generator=g).to(BF16)
    else:
        dx = torch.randn(B, T, C, generator=g).to(BF16)
    return dict(dx=dx, idx=flat.reshape(B, T), V=V, n_pos=T + 3, family=family)


def embed_bwd_fills(inp, target):
    """(dwte, dwpe) as the targets hold them before the call (zeros for ``fresh``), and their dtype."""
    V, C, n_pos = inp["V"], inp["dx"].shape[-1], inp["n_pos"]
    if target == "fresh":
        return torch.zeros(V, C, dtype=BF16), torch.zeros(n_pos, C, dtype=BF16), BF16
    dt = F32 if target == "f32" else BF16
    return acc_fill((V, C), inp["family"], dt), acc_fill((n_pos, C), inp["family"], dt, base=5), dt


def embed_bwd_ref(dx, idx, V, fill_te, fill_pe):
    """dwte[v] = fill[v] + sum of dx over the tokens with id v (ids outside [0, V) add nothing); dwpe[t] = fill[t] +
    sum_b dx[b, t] for t < T.  Sums of mixed signs: unit 2^-23 (|fill| + sum |dx|)."""
    C = dx.shape[-1]
    d = dx.to(F64).reshape(-1, C)
    i = idx.reshape(-1).long()
    ok = (i >= 0) & (i < V)
    s = torch.zeros(V, C, dtype=F64).index_add_(0, i[ok], d[ok])
    sa = torch.zeros(V, C, dtype=F64).index_add_(0, i[ok], d[ok].abs())
    T = idx.shape[1]
    p, pa = torch.zeros(fill_pe.shape, dtype=F64), torch.zeros(fill_pe.shape, dtype=F64)
    p[:T], pa[:T] = dx.to(F64).sum(0), dx.to(F64).abs().sum(0)
    ft, fp = fill_te.to(F64), fill_pe.to(F64)
    return dict(dwte=(ft + s, E32 * (ft.abs() + sa)), dwpe=(fp + p, E32 * (fp.abs() + pa)))


def embed_bwd_untouched(idx, V, n_pos):
    """Row masks of dwte (ids that do not occur) and dwpe (t >= T): these rows keep their bits."""
    i = idx.reshape(-1).long()
    te = torch.ones(V, dtype=torch.bool)
    te[i[(i >= 0) & (i < V)]] = False
    pe = torch.arange(n_pos) >= idx.shape[1]
    return te, pe


def embed_bwd_model_f32(dx, idx, V, fill_te, fill_pe, defect=None):
    """The two kernels of embedding.hip in fp32, in their order: per chunk of 64 sorted positions the rows of a run
    are summed from zero in sorted order; a run complete inside its chunk is added into dwte at once; the part of
    a run that crosses the chunk's start is left in head[j], of one that starts inside and crosses the end in
    tail[j]; then tail[j] + head[j + 1] + ... in chunk order is added into dwte.  One rounding to the target's
    dtype per row.  ``defect``: drop_head (the second head of a run is skipped); double_tail (a tail added twice);
    oob_into_last (a crossing out-of-range run is added into row V - 1)."""
    C = dx.shape[-1]
    d = dx.float().reshape(-1, C)
    srt, perm = torch.sort(idx.reshape(-1).to(torch.int32), stable=True)
    s, perm, N = srt.tolist(), perm.tolist(), srt.numel()
    nch = (N + EK - 1) // EK
    dw = fill_te.clone()
    head, tail = torch.zeros(nch, C), torch.zeros(nch, C)

    def add(i, acc):
        dw[i] = (dw[i].float() + acc).to(dw.dtype)

    for j in range(nch):
        p0, p1 = j * EK, min(N, j * EK + EK)
        from_prev = p0 > 0 and s[p0 - 1] == s[p0]
        to_next = p1 < N and s[p1] == s[p1 - 1]
        acc, started = torch.zeros(C), not from_prev
        for p in range(p0, p1):
            acc = acc + d[perm[p]]
            if p + 1 < p1 and s[p + 1] == s[p]:
                continue
            if not started:
                head[j] = acc
            elif p + 1 == p1 and to_next:
                tail[j] = acc
            elif 0 <= s[p] < V:
                add(s[p], acc)
            acc, started = torch.zeros(C), True
    for j in range(nch):
        p0, p1 = j * EK, min(N, j * EK + EK)
        i = s[p1 - 1]
        if not (p1 < N and s[p1] == i) or (p0 > 0 and s[p0] == i and s[p0 - 1] == i):
            continue
        oob = i < 0 or i >= V
        if oob and defect != "oob_into_last":
            continue
        acc = tail[j] + tail[j] if defect == "double_tail" else tail[j].clone()
        for k, jj in enumerate(range(j + 1, nch)):
            if not (defect == "drop_head" and k == 1):
                acc = acc + head[jj]
            e = min(N, (jj + 1) * EK)
            if not (e < N and s[e - 1] == i and s[e] == i):
                break
        add(V - 1 if oob else i, acc)
    T = idx.shape[1]
    dp = fill_pe.clone()
    acc = dp[:T].float()
    for b in range(dx.shape[0]):
        acc = acc + dx[b].float()
    dp[:T] = acc.to(dp.dtype)
    return dict(dwte=dw, dwpe=dp)


def embed_bwd_checks(inp, target, out):
    """``out``: dwte, dwpe after the call.  The exact family under budget 0 against the sums rounded once to the
    target's dtype (every row is written by one thread, once)."""
    ft, fp, dt = embed_bwd_fills(inp, target)
    ref = embed_bwd_ref(inp["dx"], inp["idx"], inp["V"], ft, fp)
    if inp["family"] == "exact":
        return [("exact", f"{target}/{k}", out[k], (rounded(ref[k][0], dt).to(F64), 0.0)) for k in ("dwte", "dwpe")]
    return [("embed_bwd", f"{target}/{k}", out[k], ref[k]) for k in ("dwte", "dwpe")]


# ------------------------------------------------------------------------------------------------ RoPE
ROPE_D = (16, 32, 64, 128)   # hv = D / 16 = 1, 2, 4, 8 vectors per half head
ROPE_T = (1, 5)
ROPE_HEADS = ((8, 6), (4, 4), (8, 0))  # (n_heads_total, n_rot): packed qkv of H = 4, Hkv = 2; all rotated; a pure copy
ROPE_B = 2


def rope_inputs(D, nh, T, pos_offset):
    """Tables of independent random angles, two rows longer than T + pos_offset: neighbouring rows share nothing,
    so a position off by one changes every rotated element."""
    g = _gen(13, D, nh, T, pos_offset)
    x = torch.randn(ROPE_B, T, nh * D, generator=g).to(BF16)
    ang = torch.rand(T + pos_offset + 2, D // 2, generator=g, dtype=F64) * (2 * math.pi)
    return dict(x=x, cos=ang.cos().to(F32), sin=ang.sin().to(F32))


def marker_tables(n_pos, D, row):
    """cos = 1, sin = 0 (the identity) in every row but ``row``, which turns by a quarter: a kernel that reads
    another row copies where it should swap halves."""
    cos, sin = torch.ones(n_pos, D // 2), torch.zeros(n_pos, D // 2)
    cos[row], sin[row] = 0.0, 1.0
    return cos, sin


def _rope_parts(x, cos, sin, nh, T, pos_offset, inverse, dtype):
    D = x.shape[-1] // nh
    xd = x.to(dtype).reshape(-1, nh, D)
    t = torch.arange(xd.shape[0]) % T + pos_offset
    c = cos.to(dtype)[t][:, None, :]
    s = sin.to(dtype)[t][:, None, :] * (-1.0 if inverse else 1.0)
    return xd, xd[..., :D // 2], xd[..., D // 2:], c, s, D


def rope_ref(x, cos, sin, nh, n_rot, T, pos_offset=0, inverse=False, out_heads=None):
    """Rotate-half of the first n_rot heads of each packed row, position t = (row % T) + pos_offset:
    (a, b) -> (a c - b s, b c + a s), s negated for the inverse; the other heads are copied.  Each output cancels
    two products: unit 2^-23 (|a c| + |b s|), resp. (|b c| + |a s|); 0 on copied heads.  ``out_heads``: the
    leading heads kept per row (rope_qk: n_rot)."""
    xd, a, b, c, s, D = _rope_parts(x, cos, sin, nh, T, pos_offset, inverse, F64)
    o = torch.cat([a * c - b * s, b * c + a * s], -1)
    u = E32 * torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
    out, unit = xd.clone(), torch.zeros_like(xd)
    out[:, :n_rot], unit[:, :n_rot] = o[:, :n_rot], u[:, :n_rot]
    keep = nh if out_heads is None else out_heads
    shape = tuple(x.shape[:-1]) + (keep * D,)
    return out[:, :keep].reshape(shape), unit[:, :keep].reshape(shape)


def rope_models_f32(x, cos, sin, nh, n_rot, T, pos_offset=0, inverse=False, defect=None):
    """The kernel's fp32 arithmetic rounded to bf16: [unfused, fused one way, fused the other].  ``defect``:
    no_offset (t = row % T); no_inverse (the sign of s ignored); rotate_v (every head rotated)."""
    if defect == "no_offset":
        pos_offset = 0
    if defect == "no_inverse":
        inverse = False
    if defect == "rotate_v":
        n_rot = nh
    xd, a, b, c, s, D = _rope_parts(x, cos, sin, nh, T, pos_offset, inverse, F32)
    c, s = c.expand_as(a), s.expand_as(a)
    outs = []
    for lo, hi in zip(_fma_models(a, c, b, s, -1.0), _fma_models(b, c, a, s, 1.0)):
        out = xd.clone()
        out[:, :n_rot] = torch.cat([lo, hi], -1)[:, :n_rot]
        outs.append(out.reshape(x.shape).to(BF16))
    return outs


def rope_roundtrip_ref(x, cos, sin, nh, n_rot, T, pos_offset=0):
    """inverse(forward(x)) against x.  The forward's outputs (o1, o2) are rounded to bf16 in between, and the
    inverse sums o1 c + o2 s, resp. o2 c - o1 s: unit 2^-8 (|o1 c| + |o2 s|), resp. (|o2 c| + |o1 s|), which
    also covers both passes' fp32 units."""
    fwd, _ = rope_ref(x, cos, sin, nh, n_rot, T, pos_offset, False)
    _, o1, o2, c, s, D = _rope_parts(fwd, cos, sin, nh, T, pos_offset, False, F64)
    u = EPS_OUT[BF16] * torch.cat([(o1 * c).abs() + (o2 * s).abs(), (o2 * c).abs() + (o1 * s).abs()], -1)
    unit = torch.zeros_like(u)
    unit[:, :n_rot] = u[:, :n_rot]
    return x.to(F64), unit.reshape(x.shape)


# ------------------------------------------------------------------------------------------------ batched transpose
TT = 64  # tile edge (transpose.hip)
TRANSPOSE_GRID = 2048  # workgroups of the persistent grid
# (rows, cols) in table order: tiles 0, 1..2080, 2081..2088, 2089..2664, 2665, 2666..4028.  Workgroup b takes tiles
# b and b + 2048: the second tiles of b >= 33 lie in a later matrix than the first, and the ragged matrices (72 x
# 200: 8 rows / 8 columns / both left over; 1992 x 1096 likewise; 3000 x 1800: 56 rows, 8 columns) are all second
# tiles, taken after a full tile of the 2560 x 3328 matrix whose rows stale LDS would show
TRANSPOSE_PLAN = ((8, 8), (2560, 3328), (72, 200), (1992, 1096), (64, 64), (3000, 1800))
TRANSPOSE_TILES = 4029


def transpose_tile_total(shapes):
    return sum(-(-r // TT) * -(-c // TT) for r, c in shapes)


def transpose_model(srcs, grid, sentinel, defect=None):
    """The kernel's tile walk on the CPU: workgroup b takes tiles b, b + grid, ... through one LDS tile that
    keeps its contents between tiles; only the valid part of a tile is loaded and stored.  ``defect``: stale_row
    (a tile with fewer than 64 rows does not load its last row, and stores what LDS held there)."""
    first, n = [], 0
    for s in srcs:
        first.append(n)
        n += transpose_tile_total([tuple(s.shape)])
    dsts = [torch.full((s.shape[1], s.shape[0]), sentinel, dtype=s.dtype) for s in srcs]
    for b in range(min(grid, n)):
        lds = torch.full((TT, TT), sentinel, dtype=srcs[0].dtype)
        for t in range(b, n, grid):
            m = max(i for i in range(len(srcs)) if first[i] <= t)
            R, C = srcs[m].shape
            tiles_c = -(-C // TT)
            r0, c0 = (t - first[m]) // tiles_c * TT, (t - first[m]) % tiles_c * TT
            nr, nc = min(TT, R - r0), min(TT, C - c0)
            load = nr - 1 if defect == "stale_row" and nr < TT else nr
            lds[:load, :nc] = srcs[m][r0:r0 + load, c0:c0 + nc]
            dsts[m][c0:c0 + nc, r0:r0 + nr] = lds[:nr, :nc].t()
    return dsts


# ------------------------------------------------------------------------------------------------ LSE merge
LSE_D = (8, 16, 32, 64, 128)  # cpr = D / 8 = 1, 2, 4, 8, 16 lanes per row
LSE_T = (3, 33)
LSE_B, LSE_H = 2, 3  # rows = 18, 198: rows * cpr is no multiple of the 256-thread block for any D
LSE_KINDS = 8


def lse_inputs(D, T):
    """Row r (in [B, H, T] order) is of kind r % 8: 0 both finite, unrelated; 1 lse_acc = -inf; 2 lse = -inf;
    3 both -inf; 4..7 lse = lse_acc + {0, 1e-3, -20, 100}."""
    g = _gen(14, D, T)
    B, H = LSE_B, LSE_H
    o_acc = torch.randn(B, T, H, D, generator=g)
    o = torch.randn(B, T, H, D, generator=g).to(BF16)
    la = 3 * torch.randn(B * H * T, generator=g)
    lb = 3 * torch.randn(B * H * T, generator=g)
    kind = torch.arange(B * H * T) % LSE_KINDS
    for k, dlt in ((4, 0.0), (5, 1e-3), (6, -20.0), (7, 100.0)):
        lb = torch.where(kind == k, la + dlt, lb)
    ninf = torch.tensor(-math.inf)
    la = torch.where((kind == 1) | (kind == 3), ninf, la)
    lb = torch.where((kind == 2) | (kind == 3), ninf, lb)
    return dict(o_acc=o_acc, lse_acc=la.reshape(B, H, T), o=o, lse=lb.reshape(B, H, T), kind=kind.reshape(B, H, T))


def _rows(w):
    return w.transpose(1, 2).unsqueeze(-1)  # [B, H, T] -> [B, T, H, 1]


def lse_merge_ref(o_acc, lse_acc, o, lse, **_):
    """new = logaddexp(lse_acc, lse) = max + log1p(e^-|lse_acc - lse|); o_acc = o_acc e^(lse_acc - new) + o e^(lse -
    new); a weight whose exponent is -inf - -inf is 0; both -inf: new = -inf and o_acc = 0.

    Units.  new sums max and the log1p, whose exponential e = e^-d carries its argument's rounding:
    2^-23 (|max| + log1p(e) + e (1 + d)).  o_acc cancels its two products, and each weight e^(l - new) carries the
    rounding of new, of the difference and of the exponent's argument: 2^-23 (|o_acc wa| (1 + |new| + |lse_acc -
    new|) + |o wb| (1 + |new| + |lse - new|)), plus a weight below 2^-126 flushed to 0: 2^-126 (|o_acc| + |o|)."""
    la, lb = lse_acc.to(F64), lse.to(F64)
    mx = torch.maximum(la, lb)
    both = mx == -math.inf
    d = (la - lb).abs()
    d = torch.where(torch.isnan(d), torch.zeros_like(d), d)  # both -inf
    e = torch.exp(-d)
    zero = torch.zeros_like(mx)
    new = torch.where(both, mx, mx + torch.log1p(e))
    unit_l = torch.where(both, zero, E32 * (mx.abs() + torch.log1p(e) + e * (1 + torch.where(e > 0, d, zero))))
    newf = torch.where(both, zero, new)
    outs, units = [], []
    for l, v in ((la, o_acc.to(F64)), (lb, o.to(F64))):
        dead = l == -math.inf
        arg = torch.where(dead, zero, l - newf)
        w = torch.where(dead, zero, torch.exp(arg))
        outs.append(v * _rows(w))
        units.append((v * _rows(w)).abs() * _rows(1 + newf.abs() + arg.abs()))
    unit_o = E32 * (units[0] + units[1]) + FLUSH * (o_acc.to(F64).abs() + o.to(F64).abs())
    return dict(o_acc=(outs[0] + outs[1], unit_o), lse_acc=(new, unit_l))


def lse_merge_models_f32(o_acc, lse_acc, o, lse, defect=None, **_):
    """The kernel's formula in fp32: [unfused, fused one way, fused the other] as dicts.  ``defect``: no_nan_to_num
    (the weights' -inf tests left out); stale_lse (the lanes of the columns from 8 on read lse_acc after lane 0
    has stored the merged value -- what a row split over two waves would do)."""
    ninf = -math.inf

    def weights(la, lb):
        mx = torch.maximum(la, lb)
        new = mx + torch.log1p(torch.exp(-(la - lb).abs()))
        wa, wb = torch.exp(la - new), torch.exp(lb - new)
        if defect != "no_nan_to_num":
            new = torch.where(mx == ninf, mx, new)
            wa = torch.where(la == ninf, torch.zeros_like(wa), wa)
            wb = torch.where(lb == ninf, torch.zeros_like(wb), wb)
        return new, wa, wb

    la, lb = lse_acc.to(F32), lse.to(F32)
    new, wa, wb = weights(la, lb)
    wa, wb = _rows(wa).expand_as(o_acc), _rows(wb).expand_as(o_acc)
    if defect == "stale_lse":
        _, wa2, wb2 = weights(new, lb)
        wa, wb = wa.clone(), wb.clone()
        wa[..., 8:], wb[..., 8:] = _rows(wa2).expand_as(o_acc)[..., 8:], _rows(wb2).expand_as(o_acc)[..., 8:]
    return [dict(o_acc=v, lse_acc=new) for v in _fma_models(o_acc, wa, o, wb, 1.0)]


def lse_merge_checks(inp, out):
    ref = lse_merge_ref(**inp)
    return [("lse_merge_o", "o_acc", out["o_acc"], ref["o_acc"]),
            ("lse_merge_lse", "lse_acc", out["lse_acc"], ref["lse_acc"])]


# ------------------------------------------------------------------------------------------------ bias_grad
# colsum_groups(N) = clamp(N / 256, 1, 256): N = 1, 255 -> one group (1: three idle row lanes); 256, 257, 511 ->
# still one group of up to 511 rows; 256 * 256 + 1 -> the cap of 256 groups, 257 rows each, the last one of two rows
BIAS_GRAD_N = (1, 255, 256, 257, 511, 256 * 256 + 1)
BIAS_GRAD_C = (8, 520)  # one vector; a second, mostly idle 512-column panel


def bias_grad_cases():
    return [(N, C) for N in BIAS_GRAD_N for C in BIAS_GRAD_C if not (N > 511 and C > 8)]


def bias_grad_inputs(N, C, family):
    g = _gen(15, N, C, family == "exact")
    if family == "exact":  # |sum| <= 3 * 65537 < 2^24: exact in fp32 in any order
        return torch.randint(-3, 4, (N, C), generator=g).to(BF16)
    return torch.randn(N, C, generator=g).to(BF16)


def bias_grad_checks(dy, family, target, out):
    """``out``: the fresh bf16 result, or the fp32 / bf16 target (pre-filled with ``_fill``) after the call."""
    C = dy.shape[-1]
    fill = None if target == "fresh" else acc_fill((C,), family, F32 if target == "f32" else BF16)
    dt = F32 if target == "f32" else BF16
    ref, unit = colsum_ref(dy, fill, dt)
    if family == "exact":
        return [("exact", target, out, (rounded(ref, dt).to(F64), 0.0))]
    return [("bias_grad", target, out, (ref, unit))]


def bias_grad_model_f32(dy, family, target, defect=None):
    """``defect``: no_tail (the last N mod 256 rows are not summed)."""
    N, C = dy.shape
    rows = dy[:N - N % 256] if defect == "no_tail" else dy
    sm = rows.float().sum(0)
    if target == "fresh":
        return sm.to(BF16)
    dt = F32 if target == "f32" else BF16
    return (acc_fill((C,), family, dt).float() + sm).to(dt)


# ------------------------------------------------------------------------------------------------ scale_
SCALE_NUMEL = (8, 8 * 257)  # one vector; a second block of one vector
SCALE_S = (0.5, 3.0, -1.25)  # exact in bf16


def scale_inputs(dtype, numel):
    """randn with +-0, +-inf, a quiet and a signalling NaN (payloads set) and the largest finite bf16 (times 3: it
    overflows) in the first and in the last vector."""
    g = _gen(16, dtype == F32, numel)
    x = torch.randn(numel, generator=g).to(dtype)
    sp = torch.tensor([0.0, -0.0, math.inf, -math.inf, 0.0, 0.0, S.BF16_MAX]).to(dtype)
    b = bits(sp)
    if dtype == BF16:
        b[4], b[5] = 0x7FC1, -91  # 0xFFA5: sign set, quiet bit clear
    else:
        b[4], b[5] = 0x7FC00001, -8388603  # 0xFF800005
    x[:7] = sp
    x[-7:] = sp
    return x


def scale_ref(x, s):
    """x s, rounded once to x's type.  A bf16 x times a bf16-exact s is exact in fp32 (16 bits), so the kernel's
    fp32 product and its cast round once; an fp32 x s is one correctly rounded fp32 product."""
    y = (x.to(F64) * s).to(F32)
    return y.to(BF16) if x.dtype == BF16 else y


def assert_same_bits(out, want, what):
    """Bitwise, except that a NaN need only be a NaN (its payload after arithmetic is not specified)."""
    out, want = out.detach().cpu(), want.detach().cpu()
    assert out.shape == want.shape and out.dtype == want.dtype, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(out), nan), f"{what}: NaNs differ"
    bad = (bits(out) != bits(want)) & ~nan
    assert not bad.any(), f"{what}: {int(bad.sum())} of {out.numel()} elements differ in bits, first at " \
                          f"{bad.nonzero()[0].tolist()}"
