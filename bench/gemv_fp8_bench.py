"""FP8 (e4m3, per-row scale) against bf16 weights in the decode skinny GEMM, kernel level, on one MI355X.

``gemv_fp8`` against ``gemv`` of the same build at M = 1 and M = 8 token rows on the decode projections: the
50304 x 768 LM head, GPT-2 small's QKV (2304 x 768) and MLP down (768 x 3072) and llama-1.3b's QKV, gate / up and
down projections.  Each call reads another copy of the weight, out of enough copies to exceed the 256 MB Infinity
Cache several times, so that both sides stream from HBM as a decode step over a whole model does; the two sides
alternate round by round (round 0 is warm-up), device events around ``--iters`` back-to-back launches.  Prints one
JSON line per (shape, M): every round's time, the medians, the achieved weight bytes/s, each side's spread
((max - min) / median over its rounds) and the ratio of the medians.

usage: python bench/gemv_fp8_bench.py [--rounds 7] [--iters 200]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes():
    from pretraining_llm_amd.models import get_preset
    ll = get_preset("llama-1.3b")
    C, F = ll.n_embed, ll.ffn_hidden
    qkv = (ll.n_head + 2 * ll.n_kv_head) * ll.head_dim
    return [("lm_head", 50304, 768), ("gpt2_qkv", 2304, 768), ("gpt2_mlp_down", 768, 3072),
            ("llama1.3b_qkv", qkv, C), ("llama1.3b_gate_up", 2 * F, C), ("llama1.3b_down", C, F)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--cache-mb", type=int, default=768, help="bytes of weight copies to rotate over, per side")
    args = ap.parse_args()
    import torch
    from pretraining_llm_amd import ops
    ops._lib.require()
    dev = torch.device("cuda:0")
    P = torch.ops.pllm
    torch.manual_seed(0)
    for name, N, K in shapes():
        w = (torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16)
        q, sc = P.quantize_rows_fp8(w)
        n_copies = max(2, min(256, args.cache_mb * (1 << 20) // (N * K)))  # the same count on both sides
        ws = [w.clone() for _ in range(n_copies)]
        qs = [q.clone() for _ in range(n_copies)]
        for M in (1, 8):
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            err = (P.gemv_fp8(x, q, sc, None)[0].float() - P.gemv(x, w, None)[0].float()).norm() / \
                P.gemv(x, w, None)[0].float().norm()

            def run(fp8):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.iters):
                    j = i % n_copies
                    if fp8:
                        P.gemv_fp8(x, qs[j], sc, None)
                    else:
                        P.gemv(x, ws[j], None)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / args.iters  # us per call

            t = {False: [], True: []}
            for rnd in range(args.rounds + 1):
                for fp8 in (False, True):
                    us = run(fp8)
                    if rnd > 0:
                        t[fp8].append(us)
            med = {k: statistics.median(v) for k, v in t.items()}
            print(json.dumps({
                "shape": name, "N": N, "K": K, "M": M, "copies": n_copies,
                "bf16_us": [round(v, 2) for v in t[False]], "fp8_us": [round(v, 2) for v in t[True]],
                "bf16_median_us": round(med[False], 2), "fp8_median_us": round(med[True], 2),
                "bf16_weight_GBps": round(2 * N * K / med[False] / 1e3, 1),
                "fp8_weight_GBps": round(N * K / med[True] / 1e3, 1),
                "bf16_spread": round((max(t[False]) - min(t[False])) / med[False], 3),
                "fp8_spread": round((max(t[True]) - min(t[True])) / med[True], 3),
                "fp8_over_bf16_time": round(med[True] / med[False], 3),
                "quantisation_rel_err": round(float(err), 4)}), flush=True)
        del ws, qs


if __name__ == "__main__":
    main()
