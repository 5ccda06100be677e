"""KV-cache generation throughput on one MI355X (serving path).

GPT-2 small (random init, bf16): prefill a ``--prompt``-token prompt for ``B`` sequences, then
decode ``--new`` tokens greedily, eager (one launch per kernel) vs one hipGraph replay per
token (``DecodeGraph``).  Also times the decode-attention kernel alone against the flash
forward kernel run with a single query row (what decode used before the split-KV kernel), and
with a sliding window (``attn_decode(window=)``: S = 8192 cached keys, D = 128, B in {1, 64}, window 0
and 1024, interleaved round by round).  ``--kernels-only`` stops after the kernel arms.
``--softcap C`` runs every batch size twice, without and with final-logit soft-capping (``final_logit_softcap=C``:
elementwise ops on the step's [B, V] logits).  ``--sinks`` runs every batch size without and with attention sinks
(``attn_sinks=True``: a second model of the same shape, its sinks drawn from N(0, 1)).  ``--model-only`` skips the
kernel arms.  ``--fp8-weights`` runs every batch size with the bf16 weights and with FP8 decode weights
(``GPT.quantize_decode_weights``: the same model, its projections and head quantised per row), ``--rounds`` times in
alternation, and reports every round and the medians.
Prints one JSON line per configuration.

usage: python bench/decode_bench.py [--batches 1,16,64] [--prompt 128] [--new 256] [--kernels-only] [--softcap 30]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, iters=50, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--softcap", type=float, default=None)
    ap.add_argument("--model-only", action="store_true")
    ap.add_argument("--sinks", action="store_true")
    ap.add_argument("--fp8-weights", action="store_true")
    args = ap.parse_args()
    import torch
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.models import GPT, get_preset
    ops._lib.require()
    dev = torch.device("cuda:0")

    # kernel-level: split-KV decode vs flash forward with one query row
    for B, S in () if args.model_only else ((1, 1024), (16, 1024), (64, 1024), (8, 4096)):
        H, D = 12, 64
        q = torch.randn(B, 1, H, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
        sc = 1.0 / math.sqrt(D)
        t_dec = timeit(lambda: torch.ops.pllm.attn_decode(q, k, v, sc, None), iters=200)
        t_fa = timeit(lambda: torch.ops.pllm.attn_fwd(q, k, v, True, sc), iters=200)
        kv_bytes = 2 * B * S * H * D * 2
        print(json.dumps({"kernel": "attn_decode", "B": B, "S": S, "H": H, "D": D, "decode_us": round(t_dec * 1e6, 2),
                          "flash_fwd_1row_us": round(t_fa * 1e6, 2),
                          "decode_kv_GBps": round(kv_bytes / t_dec / 1e9, 1)}), flush=True)

    # sliding window: a local layer reads the last `window` rows of the count instead of all S
    import statistics
    for B in () if args.model_only else (1, 64):
        S, H, Hkv, D = 8192, 16, 16, 128
        q = torch.randn(B, 1, H, D, device=dev, dtype=torch.bfloat16)
        k = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16)
        n = torch.full((B,), S, dtype=torch.int32, device=dev)
        sc = 1.0 / math.sqrt(D)
        times = {0: [], 1024: []}
        for rnd in range(args.rounds + 1):
            for w in times:
                t = timeit(lambda w=w: torch.ops.pllm.attn_decode(q, k, v, sc, n, w), iters=200)
                if rnd > 0:  # round 0 is warm-up
                    times[w].append(t)
        med = {w: statistics.median(ts) for w, ts in times.items()}
        print(json.dumps({"kernel": "attn_decode_window", "B": B, "S": S, "H": H, "Hkv": Hkv, "D": D,
                          **{f"window{w}_us": [round(t * 1e6, 2) for t in ts] for w, ts in times.items()},
                          **{f"window{w}_median_us": round(med[w] * 1e6, 2) for w in times},
                          "window0_kv_GBps": round(2 * B * S * Hkv * D * 2 / med[0] / 1e9, 1),
                          "window1024_kv_GBps": round(2 * B * 1024 * Hkv * D * 2 / med[1024] / 1e9, 1),
                          "window1024_over_window0": round(med[1024] / med[0], 3)}), flush=True)
        del q, k, v
    if args.kernels_only:
        return

    torch.manual_seed(0)
    cfg = get_preset(args.model)
    models = {False: GPT(cfg).to(dev, torch.bfloat16).eval()}
    if args.sinks:
        models[True] = GPT(cfg.replace(attn_sinks=True)).to(dev, torch.bfloat16).eval()
        with torch.no_grad():
            for blk in models[True].attn_blocks:
                blk.attn.sinks.normal_()
    if args.fp8_weights:
        fp8_weights_arm(args, models[False], dev)
        return
    caps = [None] + ([args.softcap] if args.softcap else [])
    for B, cap, sk in ((int(b), c, s) for b in args.batches.split(",") for c in caps for s in models):
        model, cfg = models[sk], models[sk].config.replace(final_logit_softcap=None)
        idx = torch.randint(0, cfg.vocab_size, (B, args.prompt), device=dev)
        res = {"model": args.model, "batch": B, "prompt": args.prompt, "new_tokens": args.new}
        if args.sinks:
            res["attn_sinks"] = sk
        if args.softcap:
            model.config = cfg.replace(final_logit_softcap=cap)  # no parameters: the same weights
            res["final_logit_softcap"] = cap
        for mode in ("eager", "graph"):
            g = mode == "graph"
            model.generate(idx, 4, temperature=0.0, cuda_graph=g)  # warm-up (library init, graph pools)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(idx, args.new, temperature=0.0, cuda_graph=g)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[f"{mode}_s"] = round(dt, 4)
            res[f"{mode}_tok_per_s"] = round(B * args.new / dt, 1)
            res[f"{mode}_ms_per_token_step"] = round(1000 * dt / args.new, 3)
            assert out.shape == (B, args.prompt + args.new)
        print(json.dumps(res), flush=True)


def fp8_weights_arm(args, model, dev):
    """bf16 against FP8 decode weights on one model, interleaved round by round (round 0 is warm-up)."""
    import statistics
    import torch
    cfg = model.config
    for B in (int(b) for b in args.batches.split(",")):
        idx = torch.randint(0, cfg.vocab_size, (B, args.prompt), device=dev)
        tps = {(w, mode): [] for w in ("bf16", "fp8") for mode in ("eager", "graph")}
        for rnd in range(args.rounds + 1):
            for w in ("bf16", "fp8"):
                if w == "fp8":
                    model.quantize_decode_weights("fp8")
                for mode in ("eager", "graph"):
                    g = mode == "graph"
                    if rnd == 0:
                        model.generate(idx, 4, temperature=0.0, cuda_graph=g)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = model.generate(idx, args.new, temperature=0.0, cuda_graph=g)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    assert out.shape == (B, args.prompt + args.new)
                    if rnd > 0:
                        tps[(w, mode)].append(B * args.new / dt)
                model.drop_decode_weights()
        res = {"model": args.model, "batch": B, "prompt": args.prompt, "new_tokens": args.new, "rounds": args.rounds}
        for (w, mode), v in tps.items():
            res[f"{w}_{mode}_tok_per_s"] = [round(t, 1) for t in v]
            res[f"{w}_{mode}_median_tok_per_s"] = round(statistics.median(v), 1)
        for mode in ("eager", "graph"):
            res[f"fp8_over_bf16_{mode}"] = round(res[f"fp8_{mode}_median_tok_per_s"] / res[f"bf16_{mode}_median_tok_per_s"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
