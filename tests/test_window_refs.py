"""The windowed decode cases of ``_window_refs`` on the CPU: the references read only the window, and the fp32 model
of the decode kernel needs no more than the ``decode_o`` budget the table of ``_attention_refs`` already holds."""
import torch

import _attention_refs as A
import _window_refs as Wn

F64 = torch.float64


def test_cases_are_the_listed_ones():
    cases = Wn.window_cases()
    assert len(cases) == 28 and len(set(cases)) == 28
    per_row = [c for c in cases if c[3] == 5]
    assert len(per_row) == 24
    for c in per_row:  # splits come from min(S, W), not from the 1000-row buffer
        assert Wn.window_splits(c) == {1: 1, 2: 1, 40: 1, 64: 1, 65: 2, 257: 5}[c[6]]
        W = c[6]
        assert Wn.window_ranges(c) == [(0, 0), (0, 1), (0, W), (1, W + 1), (1000 - W, 1000)]
    assert Wn.window_ranges(cases[24]) == [(260, 300), (1, 41)]
    assert Wn.window_ranges(cases[25]) == [(660, 700)] * 2
    assert Wn.window_ranges(cases[26]) == [(217, 257)] * 2
    assert Wn.window_ranges(cases[27]) == [(0, 300)] * 2  # does not bite


def test_reference_reads_only_the_window():
    case = (64, 8, 4, 5, 1000, (0, 1, 65, 66, 1000), 65)
    inp, (ref, unit) = Wn.window_case(case)
    assert torch.isfinite(ref).all() and torch.isfinite(unit).all()
    assert not ref[0].any() and not unit[0].any()  # count 0
    for b, (f, n) in enumerate(Wn.window_ranges(case)):
        assert torch.isnan(inp["k"][b, :f].float()).all() and torch.isnan(inp["v"][b, n:].float()).all()
        assert torch.isfinite(inp["k"][b, f:n].float()).all() and torch.isfinite(inp["v"][b, f:n].float()).all()
        if n == 0:
            continue
        # an independent double-precision softmax over the slice
        q, k, v = (inp[x][b].to(F64) for x in "qkv")
        kk = k[f:n].repeat_interleave(2, dim=1)  # [n - f, H, D]
        vv = v[f:n].repeat_interleave(2, dim=1)
        p = torch.softmax(torch.einsum("hd,jhd->hj", q[0], kk) * inp["scale"], -1)
        torch.testing.assert_close(ref[b, 0], torch.einsum("hj,jhd->hd", p, vv), rtol=1e-12, atol=1e-14)


def test_decode_budget_is_unchanged_on_the_windowed_cases():
    """The smallest integer budget of the fp32 model over the windowed cases is the table's measured value, so the
    table's budget (twice that) applies to the windowed kernel as it stands."""
    worst = 0
    for case in Wn.window_cases():
        _, (ref, unit) = Wn.window_case(case)
        worst = max(worst, A.ulps_needed(Wn.window_model(case), ref, unit))
    assert worst == A.BUDGET["decode_o"][0] == 1, worst
