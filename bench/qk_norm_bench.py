"""QK-norm microbench at the llama training shape (32768 rows, H = Hkv = 16, D = 128; --small adds D = 64 / 32
shapes): the fused pre-pass ``qk_norm_rope`` against the RoPE pre-pass it replaces (``rope_qk``), interleaved
round by round, and the streaming backward ``qk_norm_bwd_``.  One JSON line per shape: median / min us of each
and TB/s of the bytes each call must move --
  rope_qk       read the q / k columns of qkv, write qk                      (2 x rows (H + Hkv) D bf16)
  qk_norm_rope  the same + rstd fp32 [rows, H + Hkv]
  qk_norm_bwd_  read the q / k columns of qkv and of dqkv, write dqkv's      (3 x rows (H + Hkv) D bf16) + rstd
(the fp32 tables and gains stay in cache).  The inputs rotate over --bufs buffers so that a call does not find
its input in the 256 MB Infinity Cache.  usage: python bench/qk_norm_bench.py [--rounds 9] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timeit(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bufs", type=int, default=4)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    from pretraining_llm_amd import ops
    from pretraining_llm_amd.ops import _lib
    _lib.require()
    P = torch.ops.pllm
    shapes = [(16, 2048, 16, 16, 128)]
    if args.small:
        shapes += [(64, 1024, 12, 12, 64), (16, 2048, 32, 8, 64), (16, 2048, 16, 16, 32)]
    for B, T, H, Hkv, D in shapes:
        rows, W, NH = B * T, (H + 2 * Hkv) * D, H + Hkv
        qkvs = [torch.randn(B, T, W, device="cuda").bfloat16() for _ in range(args.bufs)]
        dqkvs = [torch.randn(B, T, W, device="cuda").bfloat16() for _ in range(args.bufs)]
        wq = (1 + 0.1 * torch.randn(D, device="cuda")).bfloat16()
        wk = (1 + 0.1 * torch.randn(D, device="cuda")).bfloat16()
        cos, sin = ops.rope_cache(T, D, 10000.0, "cuda")
        rstd = P.qk_norm_rope(qkvs[0], wq, wk, 1e-5, H, Hkv, cos, sin, T, 0)[1]
        n = args.bufs
        f_rope = lambda i: P.rope_qk(qkvs[i % n], cos, sin, H + 2 * Hkv, NH, T)  # noqa: E731
        f_qkn = lambda i: P.qk_norm_rope(qkvs[i % n], wq, wk, 1e-5, H, Hkv, cos, sin, T, 0)  # noqa: E731
        f_qkn0 = lambda i: P.qk_norm_rope(qkvs[i % n], wq, wk, 1e-5, H, Hkv, None, None, T, 0)  # noqa: E731
        f_bwd = lambda i: P.qk_norm_bwd_(dqkvs[i % n], qkvs[i % n], rstd, wq, wk, H, Hkv, None, None, False)  # noqa: E731
        fns = {"rope_qk": f_rope, "qk_norm_rope": f_qkn, "qk_norm_only": f_qkn0, "qk_norm_bwd": f_bwd}
        for f in fns.values():
            for i in range(3):
                f(i)
        ts = {k: [] for k in fns}
        for _ in range(args.rounds):  # interleaved: every round times each kernel once
            for k, f in fns.items():
                ts[k].append(timeit(f, args.reps))
        qk_bytes = rows * NH * D * 2
        nbytes = {"rope_qk": 2 * qk_bytes, "qk_norm_rope": 2 * qk_bytes + rows * NH * 4,
                  "qk_norm_only": 2 * qk_bytes + rows * NH * 4, "qk_norm_bwd": 3 * qk_bytes + rows * NH * 4}
        rec = {"rows": rows, "H": H, "Hkv": Hkv, "D": D}
        for k in fns:
            med = statistics.median(ts[k])
            rec[k] = {"us": round(med, 1), "min_us": round(min(ts[k]), 1), "max_us": round(max(ts[k]), 1),
                      "mb": round(nbytes[k] / 1e6, 1), "tbs": round(nbytes[k] / med / 1e6, 2)}
        rec["qk_norm_rope_over_rope_qk"] = round(rec["qk_norm_rope"]["us"] / rec["rope_qk"]["us"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
