"""The streaming HIP kernels (norms, activations, SwiGLU, cross-entropy, AdamW, gradient norm, sampling) at edge
shapes and on the dispatch arms ``test_kernels_gpu.py`` does not reach, compared element by element with the fp64
references of ``_streaming_refs`` under the budgets calibrated there (``test_streaming_refs.py``).

Every op is called through ``torch.ops.pllm`` directly, so the tests control strides and optional arguments."""
import math

import pytest
import torch

import _streaming_refs as R

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


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ----------------------------------------------------------------------------------------------- norms
# which C reaches which K instantiation, and which N which grid shape: see R.norm_cases
@pytest.mark.parametrize("rms,res,C,N", R.norm_cases())
def test_norm_edges(rms, res, C, N):
    inp = R.norm_inputs(rms, res, C, N)
    fw, mean32, rstd32 = R.norm_stats32(inp)
    x, r, w, b, dy, ds = (_d(inp[k]) for k in ("x", "r", "w", "b", "dy", "ds"))
    y, s, mean, rstd = _ops().norm_fwd(x, r, w, b, inp["eps"], bool(rms))
    # the backward from the reference's statistics and residual sum, so that it is judged on its own
    s_in, mu, rs = _d(fw["s_bf16"]), _d(mean32), _d(rstd32)
    dx, dw, db = _ops().norm_bwd(dy, s_in, w, mu, rs, ds, not rms, bool(rms))
    acc = [_d(inp["fill"][i]).clone() for i in range(3)]  # fp32 targets, pre-filled non-zero
    dx_acc = _ops().norm_bwd_acc(dy, s_in, w, mu, rs, ds, not rms, bool(rms), acc[0], None if rms else acc[1], acc[2])
    torch.cuda.synchronize()
    out = dict(s=s, mean=mean, rstd=rstd, y=y, dx=dx, dw=dw, db=db, dx_acc=dx_acc, dw_acc=acc[0], db_acc=acc[1],
               xb_acc=acc[2])
    assert s.numel() == (x.numel() if res else 0)
    if rms:
        assert not mean.any() and torch.equal(acc[1].cpu(), inp["fill"][1])  # no mean, bias target untouched
    R.check_all(R.norm_checks(inp, out))


# ----------------------------------------------------------------------------------------------- activations
def _saturation(x, out, dy_out, big=10.0):
    """The limits the fast-math forms promise: for x >= 10 the activation is x and its derivative 1 (to the last
    bf16 bit: the true deviation is below 2^-100); for x <= -10 both are 0 to within 2^-110 (the true values are
    below 2^-117 in magnitude, and a flushed exponential only brings them closer to 0); nothing is NaN / Inf."""
    xc, oc, dc = x.cpu().double(), out.cpu().double(), dy_out.cpu().double()
    assert torch.isfinite(oc).all() and torch.isfinite(dc).all()
    hi, lo = xc >= big, xc <= -big
    assert torch.equal(oc[hi], xc[hi]) and (dc[hi] == 1).all()
    assert (oc[lo].abs() <= 2.0 ** -110).all() and (dc[lo].abs() <= 2.0 ** -110).all()


# numel 8: one vector; 8*257: a second block of one vector; 8*(256*3+1): act_fwd's two-vector pairing with a tail
@pytest.mark.parametrize("data", ["randn", "grid"])
@pytest.mark.parametrize("numel", R.ACT_NUMEL)
@pytest.mark.parametrize("kind", ["relu", "gelu"])
def test_activation_edges(kind, numel, data):
    inp = R.act_inputs(kind, numel, data)
    op = 0 if kind == "relu" else 1
    x, dy = _d(inp["x"]), _d(inp["dy"])
    y = _ops().act_fwd(x, op)
    dx = _ops().act_bwd(dy, _d(R.relu_of(inp["x"])) if kind == "relu" else x, op)  # ReLU backward takes the output
    R.check_all(R.act_checks(kind, inp, dict(y=y, dx=dx)))
    if kind == "relu":
        assert torch.equal(y.cpu(), R.relu_of(inp["x"]))
    elif data == "grid":
        _saturation(x, y, dx)


def test_relu_bwd_takes_output_with_signed_zeros():
    y = torch.tensor([0.0, -0.0, 2.0 ** -20, 1.0, R.BF16_MAX, -0.0, 0.0, 3.0], dtype=F64).to(BF16)
    dy = torch.tensor([1.0, 2.0, 3.0, -4.0, 5.0, 6.0, 7.0, -8.0]).to(BF16)
    dx = _ops().act_bwd(_d(dy), _d(y), 0)
    assert torch.equal(dx.cpu().float(), torch.tensor([0.0, 0.0, 3.0, -4.0, 5.0, 0.0, 0.0, -8.0]))


# F = 8: one vector per row; 136, 688: rows that end inside a block; rows = 5: the row / column split of the index
@pytest.mark.parametrize("data", ["randn", "grid"])
@pytest.mark.parametrize("rows,Fd", R.SWIGLU_SHAPES)
def test_swiglu_edges(rows, Fd, data):
    inp = R.swiglu_inputs(rows, Fd, data)
    gu, dy = _d(inp["gu"]), _d(inp["dy"])
    y = _ops().swiglu_fwd(gu)
    dgu = _ops().swiglu_bwd(dy, gu)
    R.check_all(R.swiglu_checks(inp, dict(y=y, dgu=dgu)))
    if data == "grid":  # SiLU's limits: silu(g) -> g, silu'(g) -> 1 for large g; both -> 0 for large -g (dy = 1)
        g, u = inp["gu"][:, :Fd].double(), inp["gu"][:, Fd:].double()
        yc, dg, du = y.cpu().double(), dgu.cpu()[:, :Fd].double(), dgu.cpu()[:, Fd:].double()
        assert torch.isfinite(yc).all() and torch.isfinite(dgu.cpu().double()).all()
        hi, lo = g >= 30, g <= -100
        assert torch.equal(yc[hi], (g * u).to(BF16).double()[hi]) and torch.equal(dg[hi], u[hi])
        assert torch.equal(du[hi], g[hi])
        for t in (yc, dg, du):
            assert (t[lo].abs() <= 2.0 ** -110).all()


def _act_bwd_bias(kind, inp, acc):
    bias = _d(inp["fill"].to(acc)).clone()
    dx = _ops().act_bwd_bias(_d(inp["dy"]), _d(inp["x"]), 0 if kind == "relu" else 1, bias)
    assert dx.shape == inp["x"].shape
    R.check_all(R.act_bias_checks(kind, inp, dict(dx=dx, bias=bias), acc))
    ref, floor = R.act_bias_ref_sums(kind, inp, acc)
    R.assert_close_ulps(bias, ref, R.BUDGET["colsum"][1], floor, what="bias against the reference's column sums")
    return dx


# (1, 8): one row, one vector, three idle row lanes; (5, 520): a second, mostly idle 512-column panel (c8 < nch);
# (13, 1032): the two-row loop's `two == false` tail in one row lane only; (300, 3080): the tail in all four;
# (600, 24): two row groups of 300
@pytest.mark.parametrize("acc", [BF16, F32], ids=["bf16acc", "f32acc"])
@pytest.mark.parametrize("N,C", R.ACT_BIAS_SHAPES)
@pytest.mark.parametrize("kind", ["relu", "gelu"])
def test_act_bwd_bias_edges(kind, N, C, acc):
    _act_bwd_bias(kind, R.act_bias_inputs(kind, N, C), acc)


# the magnitude grid through the fused kernel too (dy = 1): the derivative's limits, and column sums of them
@pytest.mark.parametrize("N,C", R.ACT_BIAS_GRID_SHAPES)
@pytest.mark.parametrize("kind", ["relu", "gelu"])
def test_act_bwd_bias_on_magnitude_grid(kind, N, C):
    inp = R.act_bias_inputs(kind, N, C, "grid")
    dx = _act_bwd_bias(kind, inp, F32).cpu().double()
    x = inp["x"].double()
    assert torch.isfinite(dx).all()
    if kind == "relu":
        assert torch.equal(dx, (x > 0).double())
    else:  # as _saturation: 1 for x >= 10, 0 to within 2^-110 for x <= -10
        assert (dx[x >= 10] == 1).all() and (dx[x <= -10].abs() <= 2.0 ** -110).all()


# ----------------------------------------------------------------------------------------------- cross-entropy
def _ce_run(inp, variant, inv_n=None):
    """-> loss, dlogits; ``variant``: dlogits aliasing logits, a separate buffer, or column slices of padded ones."""
    lg, t = _d(inp["logits"]), _d(inp["targets"])
    N, V = lg.shape
    inv = None if inv_n is None else torch.tensor([inv_n], device=DEV, dtype=F32)
    if variant == "alias":
        dl = lg.clone()
        return _ops().cross_entropy(dl, t, dl, R.IGNORE, inv), dl
    if variant == "separate":
        dl = torch.full_like(lg, math.nan)
        keep = lg.clone()
        loss = _ops().cross_entropy(lg, t, dl, R.IGNORE, inv)
        assert torch.equal(_bits(lg), _bits(keep)), "logits changed"
        return loss, dl
    src = torch.full((N, V + 24), math.nan, device=DEV, dtype=BF16)
    dst = torch.full((N, V + 24), math.nan, device=DEV, dtype=BF16)
    src[:, :V] = lg
    pad_src, pad_dst = _bits(src[:, V:]).clone(), _bits(dst[:, V:]).clone()
    loss = _ops().cross_entropy(src[:, :V], t, dst[:, :V], R.IGNORE, inv)
    assert torch.equal(_bits(src[:, V:]), pad_src) and torch.equal(_bits(dst[:, V:]), pad_dst), "padding written"
    assert torch.equal(_bits(src[:, :V]), _bits(lg)), "logits changed"
    return loss, dst[:, :V]


# which V reaches which CH instantiation: see R.ce_inputs
@pytest.mark.parametrize("variant", ["alias", "separate", "strided"])
@pytest.mark.parametrize("V", R.CE_V)
def test_cross_entropy_edges(V, variant):
    inp = R.ce_inputs(V)
    loss, dl = _ce_run(inp, variant)
    R.check_all(R.ce_checks(inp, dict(loss=loss, dlogits=dl)))


@pytest.mark.parametrize("V", [8, 4104, 131072])
def test_cross_entropy_explicit_inv_n(V):
    inp = R.ce_inputs(V)
    loss, dl = _ce_run(inp, "separate", inv_n=0.125)
    R.check_all(R.ce_checks(inp, dict(loss=loss, dlogits=dl), inv_n=0.125))
    # the default path is the explicit one at 1 / #valid: bit for bit
    loss_d, dl_d = _ce_run(inp, "separate")
    n_valid = int((inp["targets"] != R.IGNORE).sum())
    loss_e, dl_e = _ce_run(inp, "separate", inv_n=1.0 / n_valid)
    assert torch.equal(_bits(dl_d), _bits(dl_e)) and torch.equal(loss_d, loss_e) and torch.equal(loss_d, loss)


@pytest.mark.parametrize("variant", ["alias", "strided"])
def test_cross_entropy_all_rows_ignored(variant):
    inp = R.ce_inputs(4104, all_ignored=True)
    loss, dl = _ce_run(inp, variant)  # inv_n = 1 / max(#valid, 1): clamped, nothing is NaN
    assert not loss.any() and not dl.float().any()
    R.check_all(R.ce_checks(inp, dict(loss=loss, dlogits=dl)))


def test_cross_entropy_vocab_limit():
    """The last accepted vocabulary is the largest one of test_cross_entropy_edges (checked there per element, with
    dlogits NaN-poisoned); the first multiple of 8 past it raises."""
    vmax = _ops().cross_entropy_max_vocab()
    assert vmax == R.CE_V[-1] and vmax % 8 == 0
    tg = torch.zeros(1, device=DEV, dtype=torch.long)
    _ops().cross_entropy(torch.zeros(1, vmax, device=DEV, dtype=BF16), tg, None, R.IGNORE, None)
    with pytest.raises(RuntimeError, match="vocab too large"):
        _ops().cross_entropy(torch.zeros(1, vmax + 8, device=DEV, dtype=BF16), tg, None, R.IGNORE, None)


# ----------------------------------------------------------------------------------------------- AdamW
# which n / mask / variant reaches what: see R.adamw_cases
@pytest.mark.parametrize("n,gd,mask,variant", R.adamw_cases())
def test_adamw_edges(n, gd, mask, variant):
    inp = R.adamw_inputs(n, gd, mask, variant)
    master, m, v = (_d(inp[k]).clone() for k in ("master", "m", "v"))
    param = torch.full((n,), math.nan, device=DEV, dtype=BF16) if inp["with_param"] else \
        torch.empty(0, device=DEV, dtype=BF16)
    scale = None if inp["scale"] is None else torch.tensor([inp["scale"]], device=DEV, dtype=F32)
    _ops().adamw_(param, master, m, v, _d(inp["grad"]), inp["lr"], inp["b1"], inp["b2"], inp["eps"], inp["wd"],
                  inp["step"], inp["grad_scale"], scale, _d(inp["wd_mask"]), _d(inp["hyper"]))
    R.check_all(R.adamw_checks(inp, dict(master=master, m=m, v=v)))
    if inp["with_param"]:  # the bf16 weights are the rounded new master, bit for bit
        assert torch.equal(_bits(param), _bits(master.to(BF16)))


# ----------------------------------------------------------------------------------------------- gradient norm
# n = 8: one vector; 8*255: one partly idle block; 8*(256*1024*2+3): the grid capped at 1024 blocks loops twice
# and a bit, with the large magnitudes in the second sweep only
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sumsq_and_grad_norm_clip_edges(n, dtype):
    xc = R.sumsq_inputs(n, dtype)
    x = _d(xc)
    a, b = _ops().sumsq(x), _ops().sumsq(x)
    assert torch.equal(a, b), "sumsq is not deterministic"
    R.check("sumsq", a, R.sumsq_ref(xc), "sumsq")
    nrm = math.sqrt(float(R.sumsq_ref(xc)[0])) * 0.5
    for max_norm in (nrm * 0.25, nrm * 4.0):  # the clipping and the non-clipping side
        out = _ops().grad_norm_clip(x, 0.5, max_norm)
        ref = R.grad_norm_clip_ref(xc, 0.5, max_norm)
        assert (ref[0][1] < 1) == (max_norm < nrm)
        R.check("sumsq", out, ref, "grad_norm_clip")
        if max_norm > nrm:
            assert out[1].item() == 1.0


# ----------------------------------------------------------------------------------------------- sampling
SAMPLE_V = (1, 7, 1025, 16385)  # one logit; under one wave; one past the block's 1024 threads; one past a 1024*16 sweep


def _logits(V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (3 * torch.randn(5, V, generator=g)).to(dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", SAMPLE_V)
def test_sample_greedy_ties_masks_and_nans(V, dtype):
    lg = _logits(V, dtype, V)
    # greedy is argmax (the lowest index among equal maxima, as bf16 rounding makes some)
    first_max = (lg == lg.max(-1, keepdim=True).values).float().argmax(-1)
    assert torch.equal(_ops().sample(_d(lg), 0.0, 1).cpu()[:, 0], first_max)
    # ties take the lowest index: duplicates of the maximum in other threads, other waves and later sweeps, with
    # the lowest index in a low wave (row 0), in a high wave (row 1), and in a later sweep of thread 0 (row 2)
    ties = [[i for i in grp if i < V] for grp in ([5, 70, 1029, 16384], [900, 1025, 2000], [1024, 1030, 16000])]
    for row, grp in enumerate(ties):
        lg[row, grp] = 50.0
    want = [min(grp) if grp else int(first_max[row]) for row, grp in enumerate(ties)]
    # a row of all -inf falls back to token 0; NaN entries are never returned
    lg[3] = -math.inf
    lg[4, ::2] = math.nan
    want += [0, None]
    got = _ops().sample(_d(lg), 0.0, 1).cpu()[:, 0]
    assert got[:4].tolist() == want[:4]
    if V > 1:
        rest = lg[4].clone()
        rest[::2] = -math.inf
        assert int(got[4]) == int(rest.float().argmax()) and int(got[4]) % 2 == 1
        for seed in range(3):  # with a temperature too: never a NaN entry, never a masked one
            tok = _ops().sample(_d(lg), 0.7, seed).cpu()[:, 0]
            assert (tok[4] % 2 == 1) and tok[3] == 0
            assert all(math.isfinite(float(lg[i, tok[i]])) for i in (0, 1, 2, 4))
    else:
        assert int(got[4]) == 0  # the only entry is NaN: the fallback


# a few dominant entries, the rest masked; R rows of identical logits.  Each frequency must lie within
# 5 sqrt(p (1 - p) / R) of softmax(l / T) in fp64 (5 standard deviations of a binomial frequency); R = 65536 keeps
# that band under 5 * 0.5 / 256 < 0.01
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", [7, 1025])
def test_sample_temperature_distribution(V, dtype):
    Rr, T = 65536, 0.7
    row = torch.full((V,), -math.inf)
    hot = [0, 3, V - 1] + ([700, 1023] if V > 7 else [])
    row[hot] = torch.tensor([1.0, 0.25, -0.5, 2.0, 0.0])[:len(hot)]
    row = row.to(dtype)
    lg = _d(row)[None, :].expand(Rr, V)  # row stride 0: every row reads the same logits
    tok = _ops().sample(lg, T, 1234)[:, 0]
    assert torch.equal(tok, _ops().sample(lg, T, 1234)[:, 0]), "same seed, different draws"
    assert not torch.equal(tok, _ops().sample(lg, T, 1235)[:, 0])
    freq = torch.bincount(tok.cpu(), minlength=V).double() / Rr
    p = torch.softmax(row.double() / T, -1)
    band = 5 * torch.sqrt(p * (1 - p) / Rr)
    assert float(band.max()) <= 0.01
    assert (freq[p == 0] == 0).all(), "a masked token was drawn"
    assert ((freq - p).abs() <= band).all(), f"frequencies {freq[hot].tolist()} vs {p[hot].tolist()}"
    assert len(set(tok[:64].tolist())) > 1, "rows of identical logits all drew the same token"
