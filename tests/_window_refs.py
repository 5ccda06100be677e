"""Windowed ``attn_decode`` cases: a sliding window of ``W`` keys over a KV cache, where a sequence with ``n`` cached
keys reads rows ``[first, n)``, ``first = max(0, n - W)``.

Not collected by pytest.  The fp64 references and units are those of ``_attention_refs.decode_ref`` on the slice
``[first, n)`` and the budget is ``_attention_refs.BUDGET["decode_o"]``, unchanged: ``test_window_refs.py`` (CPU)
recomputes the smallest budget of the fp32 model (``_attention_refs.decode_model``) on these cases and asserts that it
is still the table's measured 1.  ``test_sliding_window_gpu.py`` runs the HIP kernel on the same cases.

Rows of the buffer below ``first`` and at or past the count are NaN, so a kernel that touches one of them fails (a NaN
key makes the score NaN; a NaN value row makes the output NaN even at weight 0)."""
from __future__ import annotations

import functools
import math

import torch

import _attention_refs as A
from _attention_refs import BF16, F64, _gen

WINDOWS = (1, 2, 40, 64, 65, 257)
NO_BITE = (300, 301, 10 ** 6)  # windows that do not bite at S = 300: bit-identical to the call without one


def window_cases():
    """(D, H, Hkv, B, S buffer rows, counts, W); counts as in ``_attention_refs.decode_cases`` (None: the host shape,
    an int: a device scalar, a tuple: one count per sequence).

    The host sizes the splits for min(S, W) keys: with B = 5 and S = 1000, W = 1, 2, 40, 64 give 1 split, 65 gives 2
    and 257 gives 5 (``window_splits``).  The counts (0, 1, W, W + 1, 1000) put ``first`` at 0, 0, 0, 1 and 1000 - W:
    aligned to nothing; count 0 gives exact zeros.  The last case's window does not bite (``NO_BITE``)."""
    out = [(D, Hq, Hkv, 5, 1000, (0, 1, W, W + 1, 1000), W) for W in WINDOWS for (D, Hq, Hkv) in A.DECODE_HEADS]
    h = A.DECODE_HEADS
    out += [h[1] + (2, 300, (300, 41), 40), h[2] + (2, 1000, 700, 40), h[3] + (2, 257, None, 40),
            h[0] + (2, 300, None, NO_BITE[0])]
    return out


def window_splits(case):
    D, Hq, Hkv, Bb, S, counts, W = case
    return A.decode_splits(Bb, Hkv, min(S, W))


def window_ranges(case):
    """[(first, n)] per sequence."""
    return [(max(0, n - case[6]), n) for n in A.decode_counts(case[:6])]


@functools.lru_cache(maxsize=None)
def window_case(case):
    D, Hq, Hkv, Bb, S, counts, W = case
    g = _gen(17, D, Hq, Hkv, Bb, S, W, *A.decode_counts(case[:6]))
    q = (0.8 * torch.randn(Bb, 1, Hq, D, generator=g)).to(BF16)
    k = (0.8 * torch.randn(Bb, S, Hkv, D, generator=g)).to(BF16)
    v = torch.randn(Bb, S, Hkv, D, generator=g).to(BF16)
    scale = 1.0 / math.sqrt(D)
    ref, unit = torch.zeros(Bb, 1, Hq, D, dtype=F64), torch.zeros(Bb, 1, Hq, D, dtype=F64)
    for b, (f, n) in enumerate(window_ranges(case)):
        k[b, :f], v[b, :f] = math.nan, math.nan
        k[b, n:], v[b, n:] = math.nan, math.nan
        ref[b:b + 1], unit[b:b + 1] = A.decode_ref(q[b:b + 1], k[b:b + 1, f:n], v[b:b + 1, f:n], scale, [n - f])
    inp = dict(q=q, k=k, v=v, scale=scale, counts=A.decode_counts(case[:6]), window=W)
    return inp, (ref, unit)


def window_model(case):
    """``_attention_refs.decode_model`` (fp32 throughout, one rounding to bf16) on each sequence's slice."""
    inp, _ = window_case(case)
    o = torch.zeros(inp["q"].shape, dtype=BF16)
    for b, (f, n) in enumerate(window_ranges(case)):
        o[b:b + 1] = A.decode_model(inp["q"][b:b + 1], inp["k"][b:b + 1, f:n], inp["v"][b:b + 1, f:n], inp["scale"],
                                    [n - f])
    return o
