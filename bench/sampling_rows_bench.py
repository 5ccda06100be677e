"""Time per call of the sampling ops on one MI355X: ``sample_rows`` (csrc/sampling_rows.hip: per-row temperature /
top-k / top-p / min-p in one launch) against ``sample`` (csrc/sampling.hip) with the truncation done in torch ops
in front of it, as ``sample_next`` does for top-k and as a sort + softmax + cumsum + mask would for top-p.

The variants alternate inside every round (device events around ``--iters`` back-to-back calls each, replayed from
one captured hipGraph per variant unless ``--eager``), and the median over ``--rounds`` rounds is printed as one
JSON line per (B, variant).  A build without ``sample_rows`` (the parent commit, loaded with ``PLLM_SO`` or from
its own tree) runs the ``sample`` variants only."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=50304)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--eager", action="store_true", help="time eager calls (host launch rate included)")
    a = ap.parse_args()
    from pretraining_llm_amd.ops import _lib
    ops = _lib.require()
    has_rows = hasattr(ops, "sample_rows")
    dev = torch.device("cuda", 0)
    T, K, P = 0.8, 50, 0.9
    for B in a.batches:
        lg = (3 * torch.randn(B, a.vocab, generator=torch.Generator().manual_seed(0))).to(dev)

        def prm(k=0, p=1.0, mp=0.0):
            def full(v, dt):
                return torch.full((B,), v, dtype=dt, device=dev)
            return (full(T, torch.float32), full(k, torch.int32), full(p, torch.float32), full(mp, torch.float32),
                    torch.arange(B, dtype=torch.long, device=dev), full(3, torch.long))

        def topk_then_sample():
            v, _ = torch.topk(lg, K)
            return ops.sample(lg.masked_fill(lg < v[:, -1:], float("-inf")), T, 1)

        def topp_then_sample():
            zs, _ = torch.sort(lg / T, dim=-1, descending=True)
            cum = torch.softmax(zs, -1).cumsum(-1)
            thr = zs.gather(-1, (cum >= P).int().argmax(-1, keepdim=True)) * T
            return ops.sample(lg.masked_fill(lg < thr, float("-inf")), T, 1)
        variants = {"sample": lambda: ops.sample(lg, T, 1), "torch.topk+masked_fill+sample k=50": topk_then_sample,
                    "torch sort+softmax+cumsum+mask+sample p=0.9": topp_then_sample}
        if has_rows:
            off, k50, p90, mp, allf = prm(), prm(k=K), prm(p=P), prm(mp=0.02), prm(k=K, p=P, mp=0.02)
            variants.update({"sample_rows filters off": lambda: ops.sample_rows(lg, *off),
                             "sample_rows k=50": lambda: ops.sample_rows(lg, *k50),
                             "sample_rows p=0.9": lambda: ops.sample_rows(lg, *p90),
                             "sample_rows min_p=0.02": lambda: ops.sample_rows(lg, *mp),
                             "sample_rows k=50 p=0.9 min_p=0.02": lambda: ops.sample_rows(lg, *allf)})
        times = {n: [] for n in variants}
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up: code objects, allocator pools
            for f in variants.values():
                for _ in range(10):
                    f()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        if not a.eager:
            # --iters calls captured as one hipGraph per variant: the replay is bound by the kernels, not by the
            # host's launch rate (a B = 1 call is a few microseconds of device work)
            graphs = {}
            for n, f in variants.items():
                graphs[n] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[n]):
                    for _ in range(a.iters):
                        f()
                graphs[n].replay()
            torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, f in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if a.eager:
                    for _ in range(a.iters):
                        f()
                else:
                    graphs[n].replay()
                e1.record()
                e1.synchronize()
                times[n].append(1e3 * e0.elapsed_time(e1) / a.iters)
        for n, ts in times.items():
            print(json.dumps({"tag": a.tag, "B": B, "V": a.vocab, "variant": n, "us_per_call_median": round(
                statistics.median(ts), 2), "us_per_row": round(statistics.median(ts) / B, 3),
                "us_per_call_min_max": [round(min(ts), 2), round(max(ts), 2)]}), flush=True)


if __name__ == "__main__":
    main()
