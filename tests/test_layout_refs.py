"""CPU checks of ``_layout_refs``: every fp64 reference against an independent double-precision path, the
calibration of the budgets against fp32 models of the kernels on the cases that ``test_layout_edges_gpu.py`` runs,
and the defects that the per-element bound rejects (several of which the older whole-tensor criterion accepts)."""
import math

import pytest
import torch
import torch.nn.functional as F

import _layout_refs as R
import _streaming_refs as S
from _gemm_refs import rel_norm

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32


def _same(a, b, what, tol=1e-12):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert float((a - b).abs().max()) <= tol * scale, f"{what}: {float((a - b).abs().max())} vs scale {scale}"


def _rejected(op, out, ref_unit, what):
    with pytest.raises(AssertionError):
        R.check(op, out, ref_unit, what)


# ------------------------------------------------------------------------------------ references vs independent fp64
@pytest.mark.parametrize("case", R.embed_fwd_cases()[:12], ids=str)
def test_embed_fwd_ref_matches_torch_double(case):
    inp = R.embed_fwd_inputs(*case)
    ref, _ = R.embed_fwd_ref(**inp)
    V, (B, T) = inp["wte"].shape[0], inp["idx"].shape
    table = torch.cat([inp["wte"].to(F64), torch.zeros(1, inp["wte"].shape[1], dtype=F64)])  # row V: zeros
    i = inp["idx"].long()
    i = torch.where((i < 0) | (i >= V), torch.full_like(i, V), i)
    want = F.embedding(i, table)
    assert int((i == V).sum()) == 3
    if inp["wpe"] is not None:
        pos = torch.arange(T) + inp["pos_offset"]
        want = want + F.embedding(pos, inp["wpe"].to(F64))[None]
    _same(ref, want, "embedding forward")
    assert torch.equal(ref.to(F32).to(F64), ref), "the exact family is not exact in fp32"
    if inp["wpe"] is not None:  # ... and needs the rounding to bf16, exact ties between two neighbours included
        r16 = ref.to(F32).to(BF16)
        b = R.bits(r16).int()
        near = [(b + d).to(torch.int16).view(BF16).to(F64) for d in (1, -1)]  # the neighbours in magnitude
        err = (ref - r16.to(F64)).abs()
        tie = (err == (near[0] - ref).abs()) | (err == (near[1] - ref).abs())
        assert (err != 0).any() and ((err != 0) & tie).any()


@pytest.mark.parametrize("plan,C", R.EMB_BWD_CASES[:10], ids=str)
def test_embed_bwd_ref_matches_autograd_double(plan, C):
    inp = R.embed_bwd_inputs(plan, C, "randn")
    ft, fp, _ = R.embed_bwd_fills(inp, "f32")
    ref = R.embed_bwd_ref(inp["dx"], inp["idx"], inp["V"], ft, fp)
    V, (B, T) = inp["V"], inp["idx"].shape
    i = inp["idx"]
    if len(R.EMB_BWD_PLANS[plan][3]) > 1:  # the stable sort's perm is no identity
        assert not torch.equal(torch.sort(i.reshape(-1), stable=True)[1], torch.arange(B * T))
    w = torch.zeros(V + 1, C, dtype=F64, requires_grad=True)  # row V takes the out-of-range ids
    p = torch.zeros(inp["n_pos"], C, dtype=F64, requires_grad=True)
    y = F.embedding(torch.where((i < 0) | (i >= V), torch.full_like(i, V), i), w) + p[:T][None]
    y.backward(inp["dx"].to(F64))
    _same(ref["dwte"][0], ft.to(F64) + w.grad[:V], "dwte")
    _same(ref["dwpe"][0], fp.to(F64) + p.grad, "dwpe")
    te, pe = R.embed_bwd_untouched(i, V, inp["n_pos"])
    assert torch.equal(ref["dwte"][0][te], ft.to(F64)[te]) and torch.equal(ref["dwpe"][0][pe], fp.to(F64)[pe])
    assert int(pe.sum()) == 3 and (plan != "runs" or te.nonzero().flatten().tolist() == [2, 6, 10, 11])


def test_embed_bwd_plans_reach_every_run_and_chunk_relation():
    """Classifies each run of each plan by how it meets the chunk grid, as the kernels do."""
    seen = set()
    for name, (V, B, T, runs) in R.EMB_BWD_PLANS.items():
        N, p = B * T, 0
        for i, n in runs:
            a, e = p, p + n  # [a, e)
            p = e
            oob = "oob" if i < 0 or i >= V else "in"
            j0, j1 = a // R.EK, (e - 1) // R.EK
            whole = max(0, (e // R.EK) - (-(-a // R.EK)))  # whole chunks covered
            if j0 == j1:
                kind = "inside" + ("/ends_on_end" if e % R.EK == 0 and e < N else "") \
                    + ("/whole_chunk" if a % R.EK == 0 and e % R.EK == 0 else "")
            else:
                kind = ("starts_on_start" if a % R.EK == 0 else "starts_inside") + "/crosses" \
                    + ("/3_head_chunks" if j1 - j0 >= 4 and whole >= 3 else "") \
                    + ("/ends_inside" if e % R.EK else "/ends_on_end")
            seen.add((oob, kind))
            if e == N and N % R.EK:
                seen.add((oob, "reaches_ragged_N"))
        seen.add(("N", N))
    for want in [("in", "inside"), ("in", "inside/ends_on_end"), ("in", "inside/ends_on_end/whole_chunk"),
                 ("in", "starts_on_start/crosses/ends_inside"),
                 ("in", "starts_inside/crosses/3_head_chunks/ends_inside"),
                 ("in", "starts_inside/crosses/ends_on_end"), ("in", "reaches_ragged_N"),
                 ("oob", "starts_on_start/crosses/ends_inside"), ("oob", "starts_inside/crosses/ends_inside"),
                 ("oob", "reaches_ragged_N"), ("N", 1), ("N", 64), ("N", 700), ("N", 200), ("N", 300)]:
        assert want in seen, (want, sorted(map(str, seen)))


@pytest.mark.parametrize("D", R.ROPE_D)
def test_rope_ref_matches_complex_double(D):
    for nh, n_rot in R.ROPE_HEADS:
        for T in R.ROPE_T:
            for po in (0, 3):
                for inv in (False, True):
                    inp = R.rope_inputs(D, nh, T, po)
                    ref, unit = R.rope_ref(**inp, nh=nh, n_rot=n_rot, T=T, pos_offset=po, inverse=inv)
                    x = inp["x"].to(F64).reshape(R.ROPE_B, T, nh, D)
                    z = torch.complex(x[..., :D // 2], x[..., D // 2:])
                    c, s = inp["cos"].to(F64)[po:po + T], inp["sin"].to(F64)[po:po + T]
                    w = torch.complex(c, -s if inv else s)[None, :, None, :]
                    r = z * w
                    want = x.clone()
                    want[:, :, :n_rot] = torch.cat([r.real, r.imag], -1)[:, :, :n_rot]
                    _same(ref, want.reshape(inp["x"].shape), "rope")
                    assert torch.equal(ref.reshape(-1, nh, D)[:, n_rot:], x.reshape(-1, nh, D)[:, n_rot:])
                    assert not unit.reshape(-1, nh, D)[:, n_rot:].any()
                    if n_rot:  # rope_qk's layout: the leading n_rot heads of each row
                        qk, _ = R.rope_ref(**inp, nh=nh, n_rot=n_rot, T=T, pos_offset=po, inverse=inv, out_heads=n_rot)
                        assert torch.equal(qk, ref[..., :n_rot * D])


@pytest.mark.parametrize("D,T", [(8, 3), (16, 33), (128, 3)])
def test_lse_merge_ref_matches_torch_double(D, T):
    inp = R.lse_inputs(D, T)
    assert set(inp["kind"].reshape(-1).tolist()) == set(range(R.LSE_KINDS))
    ref = R.lse_merge_ref(**inp)
    la, lb = inp["lse_acc"].to(F64), inp["lse"].to(F64)
    new = torch.logaddexp(la, lb)  # the formula of parallel/context.py, in double
    a = torch.exp(la - new).nan_to_num_(0.0).transpose(1, 2).unsqueeze(-1)
    b = torch.exp(lb - new).nan_to_num_(0.0).transpose(1, 2).unsqueeze(-1)
    both = (inp["kind"] == 3)
    assert torch.equal(ref["lse_acc"][0] == -math.inf, both) and torch.equal(new == -math.inf, both)
    fin = ~both
    _same(ref["lse_acc"][0][fin], new[fin], "lse")
    _same(ref["o_acc"][0], inp["o_acc"].to(F64) * a + inp["o"].to(F64) * b, "o_acc")
    rows = both.transpose(1, 2)
    assert not ref["o_acc"][0][rows].any() and torch.isfinite(ref["o_acc"][0]).all()
    # |lse_acc - lse| = 100: the smaller weight is below the unit
    far = (inp["kind"] == 7).transpose(1, 2)
    small = (inp["o_acc"].to(F64) * a)[far].abs()
    assert (small <= ref["o_acc"][1][far]).all()


def test_transpose_model_and_plan():
    assert R.transpose_tile_total(R.TRANSPOSE_PLAN) == R.TRANSPOSE_TILES
    assert R.TRANSPOSE_GRID < R.TRANSPOSE_TILES < 4100
    first = [R.transpose_tile_total(R.TRANSPOSE_PLAN[:i]) for i in range(len(R.TRANSPOSE_PLAN))]
    # every ragged matrix lies wholly in the second pass of the grid, so its tiles follow another one in LDS
    for (r, c), f in zip(R.TRANSPOSE_PLAN[2:], first[2:]):
        assert f >= R.TRANSPOSE_GRID
    assert [(r % 64, c % 64) for r, c in R.TRANSPOSE_PLAN[2:4]] == [(8, 8), (8, 8)]
    g = torch.Generator().manual_seed(3)
    srcs = [torch.randn(s, generator=g).to(BF16) for s in ((128, 64), (72, 72), (8, 8))]
    for grid in (1, 2, 7):
        for d, s in zip(R.transpose_model(srcs, grid, -7.0), srcs):
            assert torch.equal(d, s.t())


def test_scale_ref_is_one_rounding():
    for dt in (BF16, F32):
        x = R.scale_inputs(dt, 8 * 257)
        assert int(torch.isnan(x).sum()) == 4 and int(torch.isinf(x).sum()) == 4
        for s in R.SCALE_S:
            assert float(torch.tensor(s).to(BF16)) == s
            R.assert_same_bits(R.scale_ref(x, s), (x.float() * s).to(dt), f"scale {s}")
        z = R.scale_ref(x, 0.0)
        fin = torch.isfinite(x)
        assert torch.equal(R.bits(z)[fin] != 0, torch.signbit(x)[fin]) and not z[fin].any()
        assert torch.isnan(z[~fin]).all()
        R.assert_same_bits(R.scale_ref(x, 1.0), x, "scale 1")
        bad = R.scale_ref(x, 0.5).clone()
        R.bits(bad)[20] ^= 1
        with pytest.raises(AssertionError, match="1 of"):
            R.assert_same_bits(bad, R.scale_ref(x, 0.5), "one bit")


# ------------------------------------------------------------------------------------ calibration of the budgets
def _embed_fwd_items(defect=None):
    for case in R.embed_fwd_cases()[:12]:  # the wrap shape adds rows, no arithmetic
        inp = R.embed_fwd_inputs(*case)
        ref, unit = R.embed_fwd_ref(**inp)
        yield ("embed_fwd", str(case), R.embed_fwd_model_f32(**inp, defect=defect), (R.rne_bf16(ref).to(F64), unit))


def _embed_bwd_items():
    for plan, C in R.EMB_BWD_CASES:
        for fam in R.EMB_BWD_FAMILIES:
            inp = R.embed_bwd_inputs(plan, C, fam)
            for target in R.EMB_BWD_TARGETS:
                ft, fp, _ = R.embed_bwd_fills(inp, target)
                out = R.embed_bwd_model_f32(inp["dx"], inp["idx"], inp["V"], ft, fp)
                yield from R.embed_bwd_checks(inp, target, out)


def _rope_items():
    for D in R.ROPE_D:
        for nh, n_rot in R.ROPE_HEADS:
            for T in R.ROPE_T:
                for po in (0, 3):
                    inp = R.rope_inputs(D, nh, T, po)
                    kw = dict(nh=nh, n_rot=n_rot, T=T, pos_offset=po)
                    for inv in (False, True):
                        ref = R.rope_ref(**inp, **kw, inverse=inv)
                        for out in R.rope_models_f32(**inp, **kw, inverse=inv):
                            yield ("rope", f"D{D} {nh}/{n_rot} T{T} +{po} inv{inv}", out, ref)
                    rt = R.rope_roundtrip_ref(**inp, **kw)
                    for fwd in R.rope_models_f32(**inp, **kw):
                        for back in R.rope_models_f32(fwd, inp["cos"], inp["sin"], **kw, inverse=True):
                            yield ("rope_rt", f"D{D} {nh}/{n_rot} T{T} +{po}", back, rt)


def _lse_items():
    for D in R.LSE_D:
        for T in R.LSE_T:
            inp = R.lse_inputs(D, T)
            for out in R.lse_merge_models_f32(**inp):
                yield from R.lse_merge_checks(inp, out)


def _bias_grad_items():
    for N, C in R.bias_grad_cases():
        for fam in ("exact", "randn"):
            dy = R.bias_grad_inputs(N, C, fam)
            for target in ("fresh", "f32", "bf16"):
                yield from R.bias_grad_checks(dy, fam, target, R.bias_grad_model_f32(dy, fam, target))


def _model_items():
    for gen in (_embed_fwd_items, _embed_bwd_items, _rope_items, _lse_items, _bias_grad_items):
        yield from gen()


def test_budgets_are_calibrated_on_the_fp32_models():
    measured, worst = {}, {}
    for it in _model_items():
        op, name, out, (ref, unit) = it
        u = R.ulps_needed(out, ref, unit)
        if u >= measured.get(op, -1):
            measured[op], worst[op] = u, it
    print("measured smallest budgets:", measured)
    assert measured == {op: b[0] for op, b in R.BUDGET.items()}, "the table in _layout_refs.py is stale"
    assert R.BUDGET["bias_grad"] == S.BUDGET["colsum"] and R.BUDGET["exact"] == S.BUDGET["exact"]
    for op, (m, b) in R.BUDGET.items():
        assert b == 2 * m
        if m == 0:
            continue
        _, name, out, ref_unit = worst[op]
        R.check(op, out, ref_unit, name)  # the worst case passes at the budget
        with pytest.raises(AssertionError):  # and fails at a zero budget
            R.assert_close_ulps(out, ref_unit[0], 0, 0.0, what=f"{op}/{name}")


# ------------------------------------------------------------------------------------ defects the bound rejects
def test_embed_bwd_defects_are_rejected_where_a_norm_ratio_accepts_them():
    inp = R.embed_bwd_inputs("runs", 264, "exact")
    ft, fp, _ = R.embed_bwd_fills(inp, "f32")
    good = R.embed_bwd_model_f32(inp["dx"], inp["idx"], inp["V"], ft, fp)
    R.check_all(R.embed_bwd_checks(inp, "f32", good))
    rows = {"drop_head": 5, "double_tail": None, "oob_into_last": inp["V"] - 1}
    for defect, row in rows.items():
        bad = R.embed_bwd_model_f32(inp["dx"], inp["idx"], inp["V"], ft, fp, defect=defect)
        assert torch.equal(bad["dwpe"], good["dwpe"])
        diff = (bad["dwte"] != good["dwte"]).any(-1).nonzero().flatten().tolist()
        assert diff == ([3, 5] if row is None else [row]), (defect, diff)  # the crossing runs: ids 3 and 5
        assert rel_norm(bad["dwte"], good["dwte"]) < 1e-2, defect  # the older criterion accepts it
        (op, name, _, ref_unit), _ = R.embed_bwd_checks(inp, "f32", bad)
        _rejected(op, bad["dwte"], ref_unit, defect)
    # the randn family under its measured budget rejects them as well
    inp = R.embed_bwd_inputs("runs", 264, "randn")
    for target in ("fresh", "bf16"):
        ft, fp, _ = R.embed_bwd_fills(inp, target)
        for defect in rows:
            bad = R.embed_bwd_model_f32(inp["dx"], inp["idx"], inp["V"], ft, fp, defect=defect)
            (op, name, out, ref_unit), _ = R.embed_bwd_checks(inp, target, bad)
            _rejected(op, out, ref_unit, defect)


def test_embed_fwd_defects_are_rejected():
    case = R.embed_fwd_cases()[11]
    assert case[4:6] == (1, 5)
    inp = R.embed_fwd_inputs(*case)
    ref, unit = R.embed_fwd_ref(**inp)
    want = (R.rne_bf16(ref).to(F64), unit)
    R.check("embed_fwd", R.embed_fwd_model_f32(**inp), want, "model")
    _rejected("embed_fwd", R.embed_fwd_model_f32(**inp, defect="no_offset"), want, "wpe row t")
    trunc = R.embed_fwd_model_f32(**inp, defect="truncate")
    assert rel_norm(trunc, want[0]) < 1e-2  # truncation is half a bf16 ulp on average: the older criterion accepts it
    _rejected("embed_fwd", trunc, want, "truncation")


def test_rope_defects_are_rejected():
    D, (nh, n_rot), T, po = 32, R.ROPE_HEADS[0], 5, 3
    inp = R.rope_inputs(D, nh, T, po)
    kw = dict(nh=nh, n_rot=n_rot, T=T, pos_offset=po)
    for inv, defect in ((False, "no_offset"), (True, "no_inverse"), (False, "rotate_v")):
        ref = R.rope_ref(**inp, **kw, inverse=inv)
        for good, bad in zip(R.rope_models_f32(**inp, **kw, inverse=inv),
                             R.rope_models_f32(**inp, **kw, inverse=inv, defect=defect)):
            R.check("rope", good, ref, "model")
            _rejected("rope", bad, ref, defect)
    # the marker tables: only row pos_offset + t turns, so a wrong position copies where it should swap halves
    t = 2
    cos, sin = R.marker_tables(T + po + 2, D, po + t)
    mk = dict(x=inp["x"], cos=cos, sin=sin)
    ref = R.rope_ref(**mk, **kw)
    x = inp["x"].reshape(R.ROPE_B, T, nh, D)
    got = R.rope_models_f32(**mk, **kw)[0].reshape(R.ROPE_B, T, nh, D)
    keep = torch.arange(T) != t
    assert torch.equal(got[:, keep], x[:, keep])
    assert torch.equal(got[:, t, :n_rot, :D // 2], -x[:, t, :n_rot, D // 2:])
    assert torch.equal(got[:, t, :n_rot, D // 2:], x[:, t, :n_rot, :D // 2])
    assert torch.equal(got[:, t, n_rot:], x[:, t, n_rot:])
    _rejected("rope", R.rope_models_f32(**mk, **kw, defect="no_offset")[0], ref, "marker row missed")


def test_transpose_stale_lds_row_is_rejected():
    g = torch.Generator().manual_seed(4)
    srcs = [torch.randn(s, generator=g).to(BF16) for s in ((128, 64), (72, 72), (8, 8))]
    bad = R.transpose_model(srcs, 1, -7.0, defect="stale_row")
    assert torch.equal(bad[0], srcs[0].t())  # full tiles are not affected
    for d, s in zip(bad[1:], srcs[1:]):
        wrong = (d != s.t()).any(0).nonzero().flatten().tolist()
        assert wrong == [s.shape[0] - 1], wrong  # exactly the stale source row (a column of dst)
        assert not (d == -7.0).any()  # it holds the previous tile's data, no sentinel


def test_lse_merge_defects_are_rejected():
    inp = R.lse_inputs(32, 33)
    for good in R.lse_merge_models_f32(**inp):
        R.check_all(R.lse_merge_checks(inp, good))
    bad = R.lse_merge_models_f32(**inp, defect="no_nan_to_num")[0]
    both = inp["kind"] == 3
    assert torch.isnan(bad["lse_acc"][both]).all()
    for it in R.lse_merge_checks(inp, bad):
        _rejected(*it[:1], it[2], it[3], "no nan_to_num")
    bad = R.lse_merge_models_f32(**inp, defect="stale_lse")[0]
    items = R.lse_merge_checks(inp, bad)
    R.check(*items[1][:1], items[1][2], items[1][3], "lse itself is right")
    _rejected("lse_merge_o", bad["o_acc"], items[0][3], "stale lse_acc")
    R.check("lse_merge_o", bad["o_acc"][..., :8], tuple(t[..., :8] for t in items[0][3]), "lane 0's columns are right")


def test_bias_grad_missing_tail_is_rejected_where_a_norm_ratio_accepts_it():
    N, C = R.BIAS_GRAD_N[-1], 8
    for fam in ("exact", "randn"):
        dy = R.bias_grad_inputs(N, C, fam)
        good, bad = (R.bias_grad_model_f32(dy, fam, "f32", defect=d) for d in (None, "no_tail"))
        assert rel_norm(bad, good) < 1e-2
        (op, name, _, ref_unit), = R.bias_grad_checks(dy, fam, "f32", good)
        R.check(op, good, ref_unit, name)
        _rejected(op, bad, ref_unit, "no tail")
    dy = R.bias_grad_inputs(257, 520, "exact")
    for target in ("fresh", "bf16"):
        (op, name, _, ref_unit), = R.bias_grad_checks(dy, "exact", target, None)
        _rejected(op, R.bias_grad_model_f32(dy, "exact", target, defect="no_tail"), ref_unit, "no tail")
