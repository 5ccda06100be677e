"""Build-to-build A/B of the plain decode-attention path (``attn_decode`` without a window): two builds of the
extension (``PLLM_SO``; e.g. one made by scripts/build_variant.py from the parent commit's csrc/attn_decode.hip) run
alternately, one fresh process per build and round, in one session on one box.  GPT-2-small decode shapes: B = 1 and
B = 64, S = 1024, H = 12, D = 64.  One JSON line per shape: both builds' per-round us, their medians, build A's own
round-to-round spread, and whether build B's median lies inside it.

usage: python bench/decode_ab.py --a parent.so --b pretraining_llm_amd/_C.so [--rounds 7] [--iters 2000]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 1024, 12, 64), (64, 1024, 12, 64))


def child(iters):
    import torch
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    out = {}
    for B, S, H, D in SHAPES:
        torch.manual_seed(0)
        q = torch.randn(B, 1, H, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16)
        n = torch.full((1,), S, dtype=torch.int32, device="cuda")  # the device count, as the captured step passes it
        sc = 1.0 / math.sqrt(D)
        for _ in range(200):
            torch.ops.pllm.attn_decode(q, k, v, sc, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            torch.ops.pllm.attn_decode(q, k, v, sc, n)
        torch.cuda.synchronize()
        out[f"B{B}"] = 1e6 * (time.perf_counter() - t0) / iters
    print("AB " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", help="build A (the baseline, e.g. the parent commit's)")
    ap.add_argument("--b", help="build B")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.iters)
    times = {(s, key): [] for s in ("a", "b") for key in ("B1", "B64")}
    for rnd in range(args.rounds + 1):  # round 0 is warm-up
        for s in ("a", "b"):
            env = dict(os.environ, PLLM_SO=os.path.abspath(getattr(args, s)))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters)],
                               env=env, capture_output=True, text=True, timeout=120)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"build {s} failed in round {rnd} (exit {r.returncode})")
            line = [l for l in r.stdout.splitlines() if l.startswith("AB ")][-1]
            if rnd > 0:
                for key, t in json.loads(line[3:]).items():
                    times[(s, key)].append(t)
    for key, (B, S, H, D) in zip(("B1", "B64"), SHAPES):
        ta, tb = times[("a", key)], times[("b", key)]
        res = {"shape": f"B{B} S{S} H{H} D{D}", "iters": args.iters, "a": args.a, "b": args.b,
               "a_us": [round(t, 3) for t in ta], "b_us": [round(t, 3) for t in tb],
               "a_median_us": round(statistics.median(ta), 3), "b_median_us": round(statistics.median(tb), 3),
               "a_min_us": round(min(ta), 3), "a_max_us": round(max(ta), 3),
               "b_median_inside_a_spread": min(ta) <= statistics.median(tb) <= max(ta),
               "b_median_at_most_a_max": statistics.median(tb) <= max(ta)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
