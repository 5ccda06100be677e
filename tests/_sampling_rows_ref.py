"""fp64 reference of the per-row sampler's kept set (csrc/sampling_rows.hip, inference.generate.filter_logits),
written for the tests: numpy in double, a stable descending sort, value tiers and cumulative tier mass.

For one row of raw logits x and a temperature T > 0, z = double(x) * double(float32(1) / float32(T)) over the VALID
entries (not NaN, not -inf).  Every filter is a value threshold, so entries of one value (a tier) stay together:
top-k keeps z >= the k-th largest value (0 < k < #valid, else off); top-p, on the top-k survivors of mass M with
w = exp(z - z_max), keeps z >= t for the largest t with mass{z >= t} >= p * M (p >= 1 off, p clamped to [0, 1]);
min-p keeps z >= z_max + ln(min_p) (<= 0 off, >= 1 the maximum's ties).  T <= 0 keeps every valid entry."""
import functools
import math

import numpy as np
import torch


def logits_row(V, scale, dtype):
    """The row the sampling tests share: scale * randn(V) from the generator seeded with V, cast to ``dtype``."""
    g = torch.Generator().manual_seed(V)
    return (scale * torch.randn(V, generator=g)).to(dtype)


def inv_temperature(T):
    return float(np.float32(1.0) / np.float32(T))


class Tiers:
    """The valid entries of a row as value tiers in descending order."""

    def __init__(self, x, T):
        x = np.asarray(x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
        self.x = x
        self.valid = ~np.isnan(x) & (x != -np.inf)
        self.T = T
        inv = inv_temperature(T) if T > 0 else 1.0
        self.z = x * inv
        order = np.argsort(-np.where(self.valid, x, -np.inf), kind="stable")[:int(self.valid.sum())]
        xs = x[order]
        self.n = len(xs)
        if self.n == 0:
            return
        start = np.flatnonzero(np.r_[True, xs[1:] != xs[:-1]])  # first rank (0-based) of every tier
        self.raw = xs[start]                                    # the tier's raw logit
        self.count = np.diff(np.r_[start, self.n])
        self.end = start + self.count                           # entries down to the end of the tier
        self.zt = self.raw * inv
        self.zmax = self.zt[0]
        with np.errstate(invalid="ignore"):
            self.mass = self.count * np.exp(self.zt - self.zmax)
        self.cum = np.cumsum(self.mass)

    def tier_of_rank(self, r):
        """Index of the tier that holds the entry of 1-based rank r."""
        return int(np.searchsorted(self.end, r, side="left"))


def kept_set(x, T, top_k=0, top_p=1.0, min_p=0.0):
    """(mask of the kept entries, kept, min_kept) of one row; top_p / min_p as the float32 values the kernel reads."""
    t = Tiers(x, T)
    if t.n == 0:
        return np.zeros(len(t.x), bool), 0, math.inf
    thr = -np.inf
    if T > 0:
        if 0 < top_k < t.n:
            thr = t.zt[t.tier_of_rank(top_k)]
        p = float(np.float32(top_p))
        if p < 1.0:
            p = max(p, 0.0)
            surv = t.zt >= thr
            cum = np.cumsum(np.where(surv, t.mass, 0.0))
            thr = max(thr, t.zt[int(np.argmax(cum >= p * cum[-1]))])
        mp = float(np.float32(min_p))
        if mp > 0.0:
            thr = max(thr, t.zmax + math.log(min(mp, 1.0)))
    mask = t.valid & (t.z >= thr)
    return mask, int(mask.sum()), float(t.x[mask].min())


@functools.lru_cache(maxsize=None)
def tiers_of(V, scale, dtype, T):
    return Tiers(logits_row(V, scale, dtype), T)


# The boundary cases of the filter tests: (V, scale, boundary ranks)
CASES = [(7, 3.0, (1, 2)), (64, 3.0, (1, 2, 17)), (1025, 3.0, (1, 2, 17)), (16385, 3.0, (1, 2, 17, 300)),
         (50304, 3.0, (1, 2, 17, 300)), (16385, 0.5, (300, 9000)), (50304, 1.0, (300, 9000))]
MINP_RANKS = (1, 2, 17)
TOP_P_MARGIN = 1e-5   # of M: ~3x the fp32 error of exp(z - z_max) for |z - z_max| <= 20 (about |z - z_max| 2^-23 + 2 ulp)
MIN_P_MARGIN = 1e-4   # in z: ~25x the fp32 rounding of z plus logf


def boundary_params(t, r):
    """For boundary rank r of the tiers ``t``: {filter: (top_k, top_p, min_p, kept, min_kept)} with the threshold of
    each filter placed in the middle of the gap behind the tier that holds rank r.  top-p and min-p must clear a
    margin the reference alone computes; a boundary that does not moves one tier further, at most 8 times."""
    out = {}
    j = t.tier_of_rank(r)
    out["top_k"] = (int(t.end[j]), 1.0, 0.0, int(t.end[j]), float(t.raw[j]))
    M = t.cum[-1]
    for jj in range(j, j + 9):
        before = t.cum[jj - 1] if jj > 0 else 0.0
        if 0.5 * (t.cum[jj] - before) >= TOP_P_MARGIN * M:
            out["top_p"] = (0, float(np.float32(0.5 * (before + t.cum[jj]) / M)), 0.0, int(t.end[jj]), float(t.raw[jj]))
            break
    else:
        raise AssertionError(f"no top-p boundary with margin within 8 tiers of rank {r}")
    if r in MINP_RANKS:
        for jj in range(j, j + 9):
            if 0.5 * (t.zt[jj] - t.zt[jj + 1]) >= MIN_P_MARGIN:
                mp = float(np.float32(math.exp(0.5 * (t.zt[jj] + t.zt[jj + 1]) - t.zmax)))
                out["min_p"] = (0, 1.0, mp, int(t.end[jj]), float(t.raw[jj]))
                break
        else:
            raise AssertionError(f"no min-p boundary with margin within 8 tiers of rank {r}")
    return out


def filter_rows(V, scale, ranks, dtype, T):
    """The rows of one exact-filter test: [(label, top_k, top_p, min_p, kept, min_kept)] over ``logits_row``."""
    t = tiers_of(V, scale, dtype, T)
    rows = []
    for r in ranks:
        for name, prm in boundary_params(t, r).items():
            rows.append(((r, name),) + prm)
    rows += combined_rows(t, ranks[-1])
    return rows


def combined_rows(t, rk):
    """All three filters on one row, the tightest winning: top-k at the tier of rank ``rk``; top-p behind the tier
    of rank 2 -- it sees the mass M_k of the top-k survivors only, so its midpoint is taken relative to M_k, with
    the same margin --; min-p behind rank 17 (loose) or rank 1 (tight)."""
    jk, j2 = t.tier_of_rank(rk), t.tier_of_rank(2)
    if jk <= j2:
        return []
    Mk, before = t.cum[jk], t.cum[j2 - 1] if j2 > 0 else 0.0
    assert 0.5 * (t.cum[j2] - before) >= TOP_P_MARGIN * Mk
    p_k = float(np.float32(0.5 * (before + t.cum[j2]) / Mk))
    loose = boundary_params(t, 17)["min_p"] if rk > 17 else (0, 1.0, 0.0, t.n, None)
    tight = boundary_params(t, 1)["min_p"]
    assert tight[3] <= t.end[j2] <= loose[3]
    return [(("all", "top_p wins"), int(t.end[jk]), p_k, loose[2], int(t.end[j2]), float(t.raw[j2])),
            (("all", "min_p wins"), int(t.end[jk]), p_k, tight[2], tight[3], tight[4]),
            (("all", "top_k wins"), int(t.end[0]), 0.999, loose[2], int(t.end[0]), float(t.raw[0]))]


def mixed_batch(dtype, V=16385, B=8):
    """A batch in which every row has its own logits and its own sampler: (logits [B, V], T, top_k, top_p, min_p,
    kept, min_kept), every threshold with the margins of ``boundary_params``."""
    g = torch.Generator().manual_seed(11)
    lg = (3 * torch.randn(B, V, generator=g)).to(dtype)
    Ts = [1.0, 0.7, 1.3, 0.0, 0.9, 2.0, 0.5, 1.0]
    prm = []
    for b, T in enumerate(Ts):
        t = Tiers(lg[b], T)
        low = (0, 1.0, 0.0, t.n, float(t.raw[-1]))
        prm.append([low,                                   # every filter off
                    boundary_params(t, 50)["top_k"],
                    boundary_params(t, 17)["top_p"],
                    (1, 0.1, 1.0) + low[3:],               # greedy: the filters are ignored
                    boundary_params(t, 2)["min_p"],
                    boundary_params(t, 5)["top_p"],
                    combined_rows(t, 300)[0][1:],
                    combined_rows(t, 1000)[1][1:]][b])
    cols = list(zip(*prm))
    return (lg, Ts) + tuple(list(c) for c in cols)
