"""Microbenchmark: the attention kernels with per-row key bounds (document masks) against the plain causal path,
forward and backward (the backward includes the delta pre-pass and the dQ slab reduce), interleaved round by round in
one process.  One JSON line per shape: per-round us of each arm, and median ratios against the plain arm.

Arms:  plain     no bounds (the existing instantiations)
       one_doc   bounds all zero: the cost of the extra compare and the bound loads, nothing skipped
       docN      fixed-seed random document lengths of mean N (exponential, at least 1 token), per batch row
       windowW   a sliding window of W keys (ops.window_bounds), with ``--window W,...``

``--plain-only`` times the plain arm alone (it then runs on a build without the bounds, for build-to-build
comparisons: run the two builds alternately, one process each).

usage: python bench/attn_seg_bench.py [--configs BxHxTxD[xHkv],...] [--rounds 7] [--doc-len 256,512] [--window 512,...]
       [--plain-only]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


def random_docs(B, T, mean, seed):
    """Token rows whose separators (token 1) end documents of exponentially distributed length."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        t = 0
        while True:
            t += max(1, int(torch.empty(()).exponential_(1.0 / mean, generator=g)))
            if t > T:
                break
            idx[b, t - 1] = 1
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="64x12x1024x64,16x16x2048x128x16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--doc-len", default="256,512")
    ap.add_argument("--window", default="")
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    P = torch.ops.pllm
    dev = torch.device("cuda")
    for cfg in args.configs.split(","):
        dims = [int(v) for v in cfg.split("x")]
        B, H, T, D = dims[:4]
        Hkv = dims[4] if len(dims) > 4 else H
        torch.manual_seed(0)
        q = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(B, T, Hkv, D, device=dev, dtype=torch.bfloat16)
        do = torch.randn(B, T, H, D, device=dev, dtype=torch.bfloat16)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        scale = 1 / math.sqrt(D)
        arms = {"plain": None}
        if not args.plain_only:
            from pretraining_llm_amd import ops
            arms["one_doc"] = ops.doc_bounds(torch.zeros(B, T, dtype=torch.long, device=dev), 1)
            for n in (int(s) for s in args.doc_len.split(",") if s):
                arms[f"doc{n}"] = ops.doc_bounds(random_docs(B, T, n, 1234 + n).to(dev), 1)
            for w in (int(s) for s in args.window.split(",") if s):
                arms[f"window{w}"] = ops.window_bounds(B, T, w, dev)
        fns, vis = {}, {}
        for name, bnd in arms.items():
            extra_f = () if bnd is None else (bnd[0],)
            extra_b = () if bnd is None else (None, None, None, bnd[0], bnd[1])
            o, lse = P.attn_fwd(q, k, v, True, scale, *extra_f)
            fns[name] = (lambda e=extra_f: P.attn_fwd(q, k, v, True, scale, *e),
                         lambda e=extra_b, o=o, lse=lse: P.attn_bwd(do, q, k, v, o, lse, dq, dk, dv, True, scale, *e))
            if bnd is not None:  # visible (query, key) pairs over the causal triangle's
                i = torch.arange(T, device=dev)
                vis[name] = float((i[None] - bnd[0] + 1).sum()) / (B * T * (T + 1) / 2)
        res = {"cfg": cfg, "iters": args.iters, "visible_fraction": vis}
        times = {(n, p): [] for n in fns for p in ("fwd", "bwd")}
        for rnd in range(args.rounds + 1):
            for n, (f, b) in fns.items():
                tf, tb = timeit(f, args.iters), timeit(b, args.iters)
                if rnd > 0:  # round 0 is warm-up: a process's first round ran up to 20 % slow at the small shape
                    times[(n, "fwd")].append(tf)
                    times[(n, "bwd")].append(tb)
        for (n, p), ts in times.items():
            res[f"{n}_{p}_us"] = [round(t, 1) for t in ts]
            res[f"{n}_{p}_median_us"] = round(statistics.median(ts), 1)
            if n == "plain":
                res[f"plain_{p}_spread"] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
            else:
                res[f"{n}_{p}_over_plain"] = round(statistics.median(ts) / statistics.median(times[("plain", p)]), 3)
        print(json.dumps(res), flush=True)
        del q, k, v, do, dq, dk, dv, fns


if __name__ == "__main__":
    main()
