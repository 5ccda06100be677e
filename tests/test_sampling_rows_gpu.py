"""``torch.ops.pllm.sample_rows`` (csrc/sampling_rows.hip) on the GPU: the kept set of every filter against the fp64
reference of ``_sampling_rows_ref`` (exactly: ``kept`` and ``min_kept``), edge rows, independence of a row from its
batch, the coupling of filtered and unfiltered draws, the drawn distribution, hipGraph replay, the fake impl, and the
continuous-batching server sampling any mix of samplers in one launch per step."""
import math

import numpy as np
import pytest
import torch

import _sampling_rows_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def _ext():
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    yield


def _params(B, T=1.0, k=0, p=1.0, mp=0.0, seed=0, step=0):
    def col(v, dt):
        v = [v] * B if not isinstance(v, (list, tuple, torch.Tensor, np.ndarray)) else v
        return torch.as_tensor(v, dtype=dt).to(DEV)
    return (col(T, torch.float32), col(k, torch.int32), col(p, torch.float32), col(mp, torch.float32),
            col(seed, torch.long), col(step, torch.long))


def _run(lg, **kw):
    """(tokens [B], kept [B], min_kept [B]) on the CPU for device logits ``lg``."""
    tok, kept, mn = torch.ops.pllm.sample_rows(lg, *_params(lg.shape[0], **kw))
    assert tok.shape == (lg.shape[0], 1) and tok.dtype == torch.long
    assert kept.dtype == torch.int32 and mn.dtype == torch.float32
    return tok[:, 0].cpu(), kept.cpu(), mn.cpu()


def _expand(row, B):
    return row.to(DEV)[None, :].expand(B, row.numel())  # row stride 0


# ------------------------------------------------------------------------------------------- filters, exact
@pytest.mark.parametrize("T", [1.0, 0.7, 1.3])
@DTYPES
@pytest.mark.parametrize("V,scale,ranks", S.CASES)
def test_filters_keep_exactly_the_reference_set(V, scale, ranks, dtype, T):
    x = S.logits_row(V, scale, dtype)
    rows = S.filter_rows(V, scale, ranks, dtype, T)  # (label, top_k, top_p, min_p, kept, min_kept)
    tok, kept, mn = _run(_expand(x, len(rows)), T=T, k=[r[1] for r in rows], p=[r[2] for r in rows],
                         mp=[r[3] for r in rows], seed=list(range(len(rows))))
    got = [(int(a), float(b)) for a, b in zip(kept, mn)]
    want = [(r[4], r[5]) for r in rows]
    print({str(r[0]): (g, w) for r, g, w in zip(rows, got, want)})
    assert got == want, [(r[0], g, w) for r, g, w in zip(rows, got, want) if g != w]
    xf = x.float()
    assert all(float(xf[int(i)]) >= m for i, m in zip(tok, mn)), "a token from outside the kept set"


@DTYPES
def test_switches_off_and_maximum_only(dtype):
    V = 1025
    x = S.logits_row(V, 3.0, dtype).float()
    x[[3, 700, 1024]] = float(x.max()) + 1.0  # a tied maximum in three different waves
    x = x.to(dtype)
    top = float(x.float().max())
    low = float(x.float().min())
    cases = [dict(k=0), dict(k=V), dict(k=V + 5), dict(k=-1), dict(p=1.0), dict(p=1.5), dict(mp=0.0), dict(mp=-1.0),
             dict(p=0.0), dict(p=-0.5), dict(mp=1.0), dict(mp=2.0), dict(k=1), dict(k=3), dict(k=2, p=1.0, mp=0.0)]
    want = [(V, low)] * 8 + [(3, top)] * 7
    for T in (1.0, 0.7):
        tok, kept, mn = _run(_expand(x, len(cases)), T=T, k=[c.get("k", 0) for c in cases],
                             p=[c.get("p", 1.0) for c in cases], mp=[c.get("mp", 0.0) for c in cases],
                             seed=list(range(len(cases))))
        assert [(int(a), float(b)) for a, b in zip(kept, mn)] == want
        assert all(int(i) in (3, 700, 1024) for i in tok[8:])


@DTYPES
def test_mixed_batch_every_row_its_own_sampler(dtype):
    lg, T, k, p, mp, kept_ref, mn_ref = S.mixed_batch(dtype)
    B = lg.shape[0]
    tok, kept, mn = _run(lg.to(DEV), T=T, k=k, p=p, mp=mp, seed=list(range(100, 100 + B)), step=list(range(B)))
    assert kept.tolist() == kept_ref and mn.tolist() == mn_ref
    assert all(float(lg[b, int(tok[b])]) >= mn_ref[b] for b in range(B))
    assert int(tok[3]) == int(lg[3].float().argmax())  # the greedy row


# ------------------------------------------------------------------------------------------- edge rows
@DTYPES
@pytest.mark.parametrize("V", [1, 7, 64, 1025, 16385])
def test_edge_rows_ties_masks_nans_and_strides(V, dtype):
    g = torch.Generator().manual_seed(V)
    base = torch.empty(5, V + 3, dtype=dtype)
    base[:, :V] = (3 * torch.randn(5, V, generator=g)).to(dtype)
    lg = base[:, :V]  # a row stride that is no multiple of anything
    first_max = (lg == lg.max(-1, keepdim=True).values).float().argmax(-1)
    # duplicated maxima in other threads, other waves and later sweeps of the row
    ties = [[i for i in grp if i < V] for grp in ([5, 70, 1029, 16384], [900, 1025, 2000], [1024, 1030, 16000])]
    for row, grp in enumerate(ties):
        lg[row, grp] = 50.0
    want = [min(grp) if grp else int(first_max[row]) for row, grp in enumerate(ties)]
    lg[3] = -math.inf
    lg[4, ::2] = math.nan
    dl = base.to(DEV)[:, :V]
    assert dl.stride(0) == V + 3
    tok, kept, mn = _run(dl, T=0.0, k=1, p=0.1, mp=1.0)  # greedy ignores the filters
    ref = [S.kept_set(lg[b], 0.0) for b in range(5)]
    assert [int(v) for v in kept] == [r[1] for r in ref] and [float(v) for v in mn] == [r[2] for r in ref]
    assert int(kept[3]) == 0 and float(mn[3]) == math.inf and int(tok[3]) == 0
    assert tok[:3].tolist() == want
    rest = lg[4].float().clone()
    rest[::2] = -math.inf
    if V > 1:
        assert int(tok[4]) == int(rest.argmax()) and int(kept[4]) == V // 2
    else:
        assert int(tok[4]) == 0 and int(kept[4]) == 0  # its only entry is NaN
    # sampled, with filters: NaN entries are not counted by top-k, never kept, never drawn
    for seed in range(3):
        for prm in (dict(k=2), dict(p=0.5), dict(mp=0.3), dict(k=3, p=0.9, mp=0.01), dict()):
            tok, kept, mn = _run(dl, T=0.7, seed=seed, **prm)
            for b in range(5):
                mask, n, m = S.kept_set(lg[b], 0.7, prm.get("k", 0), prm.get("p", 1.0), prm.get("mp", 0.0))
                if b in (0, 1, 2) and ties[b] and "p" not in prm:  # the ties at 50 dominate: exact whatever the filter
                    assert (int(kept[b]), float(mn[b])) == (n, m), (b, prm)
                if b == 3:
                    assert (int(tok[b]), int(kept[b]), float(mn[b])) == (0, 0, math.inf)
                elif n == 0:
                    assert (int(tok[b]), int(kept[b])) == (0, 0)
                else:
                    i = int(tok[b])
                    assert 0 <= i < V and math.isfinite(float(lg[b, i])) and float(lg[b, i]) >= float(mn[b])
            if V > 1 and "p" not in prm and "mp" not in prm:
                assert int(kept[4]) == S.kept_set(lg[4], 0.7, prm.get("k", 0))[1]
    # row stride 0
    tok0 = _run(dl[1:2].expand(4, V), T=0.7, k=2, seed=[5, 5, 6, 5], step=[1, 1, 1, 2])[0]
    assert int(tok0[0]) == int(tok0[1])


# ------------------------------------------------------------------------------------------- row independence
@DTYPES
def test_a_row_does_not_depend_on_its_batch(dtype):
    V, B = 1025, 8
    g = torch.Generator().manual_seed(2)
    lg = (3 * torch.randn(B, V, generator=g)).to(dtype).to(DEV)
    kw = dict(T=[1.0, 0.7, 1.3, 0.9, 0.0, 1.0, 0.6, 1.1], k=[0, 5, 0, 40, 3, 0, 0, 900],
              p=[1.0, 1.0, 0.8, 0.95, 0.5, 1.0, 0.6, 1.0], mp=[0.0, 0.0, 0.0, 0.02, 0.0, 0.1, 0.0, 0.0],
              seed=[9, 8, 7, 6, 5, 4, 3, 2], step=[0, 1, 2, 3, 4, 5, 6, 7])
    out = _run(lg, **kw)
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4])
    outp = _run(lg[perm.to(DEV)], **{n: [v[i] for i in perm.tolist()] for n, v in kw.items()})
    for a, b in zip(out, outp):
        assert torch.equal(a[perm], b)
    for b in range(B):
        alone = _run(lg[b:b + 1], **{n: [v[b]] for n, v in kw.items()})
        assert all(torch.equal(x[b:b + 1], y) for x, y in zip(out, alone)), b
    # the same (seed, step) repeats every draw; another step or seed changes some
    R = 4096
    row = _expand(S.logits_row(V, 3.0, dtype), R)
    seeds = list(range(R))
    a = _run(row, T=1.0, seed=seeds, step=3)[0]
    assert torch.equal(a, _run(row, T=1.0, seed=seeds, step=3)[0])
    assert not torch.equal(a, _run(row, T=1.0, seed=seeds, step=4)[0])
    assert not torch.equal(a, _run(row, T=1.0, seed=[s + R for s in seeds], step=3)[0])
    assert len(set(a.tolist())) > 100


# ------------------------------------------------------------------------------------------- coupling
@DTYPES
def test_filtered_draw_is_the_unfiltered_draw_when_that_is_kept(dtype):
    V, R, T = 1025, 4096, 1.0
    x = S.logits_row(V, 3.0, dtype)
    row = _expand(x, R)
    seeds, steps = [i // 64 for i in range(R)], [i % 64 for i in range(R)]
    free = _run(row, T=T, seed=seeds, step=steps)
    assert (free[1] == V).all()
    full = _run(row, T=T, k=V, seed=seeds, step=steps)
    assert all(torch.equal(a, b) for a, b in zip(free, full))
    t = S.tiers_of(V, 3.0, dtype, T)
    p = float(np.float32(0.9))
    assert abs(t.cum / t.cum[-1] - p).min() >= S.TOP_P_MARGIN  # 0.9 sits clear of every tier boundary
    mask, n, m = S.kept_set(x, T, top_p=p)
    tok, kept, mn = _run(row, T=T, p=p, seed=seeds, step=steps)
    assert (kept == n).all() and (mn == m).all()
    inside = torch.from_numpy(mask)[free[0]]
    assert 0.85 * R < int(inside.sum()) < 0.95 * R
    assert torch.equal(tok[inside], free[0][inside])
    assert torch.from_numpy(mask)[tok].all()


# ------------------------------------------------------------------------------------------- distribution
@DTYPES
@pytest.mark.parametrize("V", [7, 1025])
@pytest.mark.parametrize("which", ["top_k", "top_p", "min_p"])
def test_truncated_distribution(which, V, dtype):
    Rr, T = 65536, 0.7
    row = torch.full((V,), -math.inf)
    hot = [0, 3, V - 1] + ([700, 1023] if V > 7 else [])
    row[hot] = torch.tensor([1.0, 0.25, -0.5, 2.0, 0.0])[:len(hot)]
    row = row.to(dtype)
    k, p, mp, n, _ = S.boundary_params(S.Tiers(row, T), 2)[which]  # keeps the two largest of the hot entries
    assert n == 2
    tok, kept, _ = _run(_expand(row, Rr), T=T, k=k, p=p, mp=mp, seed=list(range(Rr)))
    assert (kept == 2).all()
    mask = S.kept_set(row, T, k, p, mp)[0]
    z = torch.where(torch.from_numpy(mask), row.double() * S.inv_temperature(T), torch.tensor(-math.inf).double())
    want = torch.softmax(z, -1)
    freq = torch.bincount(tok, minlength=V).double() / Rr
    band = 5 * torch.sqrt(want * (1 - want) / Rr)
    assert float(band.max()) <= 0.01
    assert (freq[want == 0] == 0).all(), "an excluded token was drawn"
    assert ((freq - want).abs() <= band).all(), f"frequencies {freq[hot].tolist()} vs {want[hot].tolist()}"


# ------------------------------------------------------------------------------------------- hipGraph, opcheck
def test_graph_replay_reads_the_parameters_from_device_memory():
    V, B = 1025, 4
    lg = (3 * torch.randn(B, V, generator=torch.Generator().manual_seed(1))).to(DEV)
    prm = list(_params(B, T=0.8, k=[0, 20, 0, 5], p=[1.0, 0.9, 0.7, 1.0], mp=0.0, seed=[1, 2, 3, 4], step=0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.ops.pllm.sample_rows(lg, *prm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torch.ops.pllm.sample_rows(lg, *prm)
    for step, p2 in ((0, 0.7), (1, 0.7), (2, 0.2), (3, 1.0)):
        prm[5].fill_(step)
        prm[2][2] = p2
        graph.replay()
        eager = torch.ops.pllm.sample_rows(lg, *prm)
        assert all(torch.equal(a, b) for a, b in zip(out, eager)), (step, p2)


@DTYPES
def test_opcheck_fake_matches_kernel(dtype):
    lg = torch.randn(4, 300, device=DEV).to(dtype)
    torch.library.opcheck(torch.ops.pllm.sample_rows.default, (lg, *_params(4, T=0.9, k=5, p=0.9, mp=0.01, seed=3)),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError):
        torch.ops.pllm.sample_rows(lg, *_params(3))  # parameter tensors of the wrong length
    with pytest.raises(RuntimeError):
        prm = list(_params(4))
        prm[1] = prm[1].long()
        torch.ops.pllm.sample_rows(lg, *prm)


# ------------------------------------------------------------------------------------------- the server
def test_continuous_server_samples_any_mix_in_one_launch_per_step():
    from pretraining_llm_amd.inference.server import ContinuousGenerationServer, GenRequest
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(4)
    dev = torch.device("cuda", 0)
    cfg = get_preset("gpt2-tiny").replace(context_length=128)
    model = GPT(cfg).to(device=dev, dtype=torch.bfloat16).eval()
    g = torch.Generator().manual_seed(5)
    #          prompt length, new tokens, temperature, top_k, top_p, min_p, seed
    specs = [(9, 12, 0.0, None, None, None, None), (33, 5, 0.8, None, None, None, 1), (3, 20, 1.0, 40, None, None, 2),
             (64, 8, 0.7, None, 0.9, None, 3), (17, 1, 1.3, None, None, 0.05, 4), (40, 16, 0.9, 50, 0.95, None, 5),
             (5, 10, 0.0, 10, 0.5, None, 6), (12, 14, 1.1, 200, 0.8, 0.01, 7), (21, 9, 0.6, None, 0.5, 0.1, 8),
             (8, 11, 1.0, 1, None, None, 9), (30, 7, 1.5, None, 0.99, None, 10), (2, 18, 0.85, 5, None, 0.2, 1)]
    reqs = [(torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist(),) + s[1:] for s in specs for n in [s[0]]]
    assert len({r[2:] for r in reqs}) == 12
    calls = []
    real = torch.ops.pllm.sample_rows

    def counting(*args):
        calls.append(args[0].shape[0])
        return real(*args)
    srv = ContinuousGenerationServer(model, max_batch=4, max_len=160)
    torch.ops.pllm.sample_rows = counting
    try:
        futs = [srv.submit(GenRequest(p, max_new_tokens=n, temperature=T, top_k=k, seed=seed, top_p=tp, min_p=mp))
                for p, n, T, k, tp, mp, seed in reqs]
        res = [f.result(timeout=120) for f in futs]
    finally:
        torch.ops.pllm.sample_rows = real
        srv.close()
    # one launch per prefill batch and per decode step, however many samplers share the step
    assert srv.stats["max_active_slots"] == 4
    assert len(calls) == srv.stats["prefills"] + srv.stats["decode_steps"]
    for (p, n, T, k, tp, mp, seed), r in zip(reqs, res):
        ref = model.generate(torch.tensor([p], device=dev), max_new_tokens=n, temperature=T, top_k=k, top_p=tp,
                             min_p=mp, seed=seed, cuda_graph=True)[0].tolist()
        assert r.tokens == ref, (len(p), n, T, k, tp, mp, seed)
