"""Per-row top-k / top-p / min-p sampling on the CPU: the fp64 reference of the kept set (``_sampling_rows_ref``)
against independent torch constructions, the boundary cases the GPU tests draw from it, and the torch path of
``sample_next`` / ``generate`` / the servers with the new sampler parameters."""
import math

import numpy as np
import pytest
import torch

import _sampling_rows_ref as S

from pretraining_llm_amd.inference.generate import filter_logits, sample_next
from pretraining_llm_amd.inference.server import ContinuousGenerationServer, GenerationServer, GenRequest
from pretraining_llm_amd.models import GPT, get_preset

F32, BF16 = torch.float32, torch.bfloat16


def _untied(V, seed):
    x = 3 * torch.randn(V, generator=torch.Generator().manual_seed(seed))
    assert x.unique().numel() == V
    return x


@pytest.mark.parametrize("T", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("V", [7, 1025])
def test_reference_top_k_is_topk_masking(V, T):
    x = _untied(V, V)
    for k in (1, 2, 5, V - 1):
        v, _ = torch.topk(x, k)
        want = (x >= v[-1]).numpy()
        mask, kept, mn = S.kept_set(x, T, top_k=k)
        assert (mask == want).all() and kept == k and mn == float(v[-1])
    for k in (0, -3, V, V + 5):  # off
        assert S.kept_set(x, T, top_k=k)[1] == V


@pytest.mark.parametrize("T", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("V", [7, 1025])
def test_reference_top_p_and_min_p_are_the_sorted_softmax_constructions(V, T):
    x = _untied(V, V + 1)
    z = x.double() * S.inv_temperature(T)
    probs, order = torch.softmax(z, -1).sort(descending=True)
    cum = probs.cumsum(-1)
    for p in (0.1, 0.5, 0.9, 0.99):
        n = int((cum < float(np.float32(p))).sum()) + 1  # the shortest prefix of mass >= p
        # a p within rounding of a cumulative sum would make the two constructions differ for no fault of either
        assert (cum - p).abs().min() > 1e-9
        want = np.zeros(V, bool)
        want[order[:n].numpy()] = True
        mask, kept, mn = S.kept_set(x, T, top_p=p)
        assert (mask == want).all() and kept == n and mn == float(x[order[n - 1]])
    for mp in (0.01, 0.2, 0.7):
        want = (torch.softmax(z, -1) >= float(np.float32(mp)) * probs[0]).numpy()
        mask, kept, _ = S.kept_set(x, T, min_p=mp)
        assert (mask == want).all() and kept == int(want.sum())
    # the switches: off, and the maximum's ties only
    assert S.kept_set(x, T, top_p=1.0, min_p=0.0)[1] == V
    assert S.kept_set(x, T, top_p=0.0)[1] == 1 and S.kept_set(x, T, min_p=1.0)[1] == 1
    # top-p counts the mass of the top-k survivors only, and the tightest filter wins
    k = 5
    ck = probs[:k].cumsum(-1) / probs[:k].sum()
    n = int((ck < float(np.float32(0.6))).sum()) + 1
    assert S.kept_set(x, T, top_k=k, top_p=0.6)[1] == n
    assert S.kept_set(x, T, top_k=k, top_p=0.6, min_p=1.0)[1] == 1


def test_reference_ties_invalid_entries_and_greedy():
    x = torch.tensor([1.0, 2.0, math.nan, 2.0, -math.inf, 0.5, 2.0, 1.0])
    assert S.kept_set(x, 1.0)[1:] == (6, 0.5)                       # NaN and -inf are not counted
    assert S.kept_set(x, 1.0, top_k=1)[1:] == (3, 2.0)              # ties stay together
    assert S.kept_set(x, 1.0, top_k=4)[1:] == (5, 1.0)
    assert S.kept_set(x, 1.0, top_k=6)[1:] == (6, 0.5)              # k = number of valid entries: off
    assert S.kept_set(x, 1.0, top_p=0.0)[1:] == (3, 2.0)
    assert S.kept_set(x, 0.0, top_k=1, top_p=0.1, min_p=1.0)[1:] == (6, 0.5)  # greedy ignores the filters
    assert S.kept_set(torch.tensor([math.nan, -math.inf]), 1.0, top_k=1)[1:] == (0, math.inf)


@pytest.mark.parametrize("T", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,scale,ranks", S.CASES)
def test_boundary_cases_select_their_tier(V, scale, ranks, dtype, T):
    """The parameters the GPU tests derive for a boundary rank keep, in the reference, exactly the entries down to
    the end of that rank's tier -- and every case of the table finds its margin."""
    x = S.logits_row(V, scale, dtype)
    for label, k, p, mp, kept, mn in S.filter_rows(V, scale, ranks, dtype, T):
        assert S.kept_set(x, T, k, p, mp)[1:] == (kept, mn), label
        assert p == 1.0 or 0.0 < p < 1.0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_mixed_batch_cases_agree_with_the_reference(dtype):
    lg, T, k, p, mp, kept, mn = S.mixed_batch(dtype)
    for b in range(lg.shape[0]):
        assert S.kept_set(lg[b], T[b], k[b], p[b], mp[b])[1:] == (kept[b], mn[b]), b
    assert len(set(zip(T, k, p, mp))) == lg.shape[0]


@pytest.mark.parametrize("T", [0.7, 1.3])
def test_cpu_sample_next_stays_inside_the_kept_set(T):
    V, R = 1025, 2000
    x = S.logits_row(V, 3.0, F32)
    t = S.tiers_of(V, 3.0, F32, T)
    g = torch.Generator().manual_seed(3)
    lg = x[None, :].expand(R, V)
    b = S.boundary_params(t, 17)
    for k, p, mp in ((None, b["top_p"][1], None), (None, None, b["min_p"][2]), (40, b["top_p"][1], None),
                     (5, 0.999, 1e-6), (None, 0.0, None), (None, None, 1.0)):
        mask, kept, _ = S.kept_set(x, T, k or 0, 1.0 if p is None else p, 0.0 if mp is None else mp)
        z = filter_logits(x[None, :], T, k, p, mp)[0]
        assert (torch.isfinite(z).numpy() == mask).all()
        tok = sample_next(lg, T, k, g, top_p=p, min_p=mp)
        assert tok.shape == (R, 1) and mask[tok[:, 0].numpy()].all()
        if kept > 1:
            assert len(set(tok[:, 0].tolist())) > 1


def test_sample_next_without_the_new_arguments_is_unchanged():
    lg = 2 * torch.randn(6, 50, generator=torch.Generator().manual_seed(0))
    for k in (None, 7):
        a = sample_next(lg, 0.8, k, torch.Generator().manual_seed(5))
        masked = lg if k is None else lg.masked_fill(lg < torch.topk(lg, k).values[:, [-1]], -math.inf)
        want = torch.multinomial(torch.softmax(masked / 0.8, -1), 1, generator=torch.Generator().manual_seed(5))
        assert torch.equal(a, want)
    assert torch.equal(sample_next(lg, 0.0, top_p=0.5, seed=3), lg.argmax(-1, keepdim=True))
    # an integer seed: the same (seed, step) repeats the draw, another step or seed changes it
    big = lg[:1].expand(256, 50)
    a = sample_next(big, 1.0, seed=9, step=2)
    assert torch.equal(a, sample_next(big, 1.0, seed=9, step=2))
    assert not torch.equal(a, sample_next(big, 1.0, seed=9, step=3))
    assert not torch.equal(a, sample_next(big, 1.0, seed=10, step=2))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GPT(get_preset("gpt2-tiny").replace(context_length=64)).eval()


def test_generate_and_servers_take_the_new_parameters(model):
    p = [5, 9, 13, 2]
    a = model.generate(torch.tensor([p]), max_new_tokens=6, temperature=0.9, top_p=0.8, min_p=0.01, seed=4)
    assert torch.equal(a, model.generate(torch.tensor([p]), max_new_tokens=6, temperature=0.9, top_p=0.8, min_p=0.01,
                                         seed=4))
    top1 = model.generate(torch.tensor([p]), max_new_tokens=6, temperature=0.9, top_p=0.0)  # the maximum only
    assert torch.equal(top1, model.generate(torch.tensor([p]), max_new_tokens=6, temperature=0.0))
    # positional construction as the HTTP layer does it, and the new fields behind t_submit
    r = GenRequest(p, 6, 0.9, 3, 11)
    assert (r.top_k, r.seed, r.top_p, r.min_p) == (3, 11, None, None)
    assert GenRequest(p, top_p=0.5).group_key() != GenRequest(p).group_key()
    assert GenRequest(p, min_p=0.5).group_key() != GenRequest(p).group_key()
    for srv in (GenerationServer(model, max_batch=4, max_wait_ms=50.0), ContinuousGenerationServer(model, max_batch=4)):
        try:
            futs = [srv.submit(GenRequest(p, max_new_tokens=6, temperature=0.9, top_p=0.0)),
                    srv.submit(GenRequest(p, max_new_tokens=6, temperature=0.9, min_p=1.0)),
                    srv.submit(GenRequest(p, max_new_tokens=6, temperature=0.9, top_p=0.7, min_p=0.05, seed=1)),
                    srv.submit(GenRequest(p, max_new_tokens=6, temperature=0.9))]
            res = [f.result(timeout=120) for f in futs]
        finally:
            srv.close()
        assert res[0].tokens == top1[0].tolist() and res[1].tokens == top1[0].tolist()
        assert all(len(r.new_tokens) == 6 for r in res)


def test_http_body_accepts_top_p_and_min_p(model):
    from fastapi.testclient import TestClient

    from pretraining_llm_amd.inference.server import create_app
    srv = GenerationServer(model, max_batch=2, max_wait_ms=10.0)
    try:
        c = TestClient(create_app(srv))
        greedy = c.post("/generate", json={"tokens": [1, 2, 3], "max_new_tokens": 4, "temperature": 0.0}).json()
        out = c.post("/generate", json={"tokens": [1, 2, 3], "max_new_tokens": 4, "temperature": 0.8, "top_p": 0.0,
                                        "min_p": 0.5})
        assert out.status_code == 200 and out.json()["tokens"] == greedy["tokens"]
    finally:
        srv.close()
