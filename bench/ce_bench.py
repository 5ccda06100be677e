"""Fused softmax-CE kernel alone at the GPT-2 LM-head shape (65536 x 50304 bf16 logits, dlogits in
place), median microseconds over rounds; select an A/B build with PLLM_SO.

With ``--z-loss Z`` and / or ``--softcap C`` the kernel with the options (cross_entropy_aux) is timed next to the plain
one, the two alternating round by round, at that shape and at a Llama-3 one (8192 x 128256, the CH = 32 arm), with
device events around 3 calls per round; the plain kernel's min-max spread over the rounds is printed with the ratio,
so that a difference can be read against it.  Each call reads and writes the logits once: 2 * N * V * 2 bytes."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pretraining_llm_amd.ops import _lib  # noqa: E402

SHAPES = ((65536, 50304), (8192, 128256))


def plain_only():
    N, V = SHAPES[0]
    logits = (torch.randn(N, V, device="cuda") * 2).bfloat16()
    tg = torch.randint(0, V, (N,), device="cuda")
    inv = torch.tensor([1.0 / N], device="cuda")
    for _ in range(3):
        torch.ops.pllm.cross_entropy(logits, tg, logits, -100, inv)
    ts = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            torch.ops.pllm.cross_entropy(logits, tg, logits, -100, inv)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 3 * 1e6)
    print(f"ce {os.environ.get('PLLM_SO', 'in-tree')} median_us={statistics.median(ts):.1f} min_us={min(ts):.1f} "
          f"TB/s={2 * N * V * 2 / statistics.median(ts) / 1e6:.2f}", flush=True)


def interleaved(N, V, variants, rounds, calls=3):
    """``variants``: name -> (z_loss, softcap) or None for the plain kernel.  Every call starts from the same logits
    (restored outside the timed window: the kernel overwrites them with the gradient)."""
    src = (torch.randn(N, V, device="cuda") * 4).bfloat16()
    logits = torch.empty_like(src)
    tg = torch.randint(0, V, (N,), device="cuda")
    inv = torch.tensor([1.0 / N], device="cuda")
    lse = torch.empty(N, device="cuda")

    def call(v):
        if v is None:
            torch.ops.pllm.cross_entropy(logits, tg, logits, -100, inv)
        else:
            torch.ops.pllm.cross_entropy_aux(logits, tg, logits, -100, inv, v[0], v[1], lse)

    ts = {k: [] for k in variants}
    for r in range(rounds + 1):  # round 0 warms every variant up
        for name, v in variants.items():
            us = 0.0
            for _ in range(calls):
                logits.copy_(src)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(v)
                b.record()
                torch.cuda.synchronize()
                us += a.elapsed_time(b) * 1e3
            if r:
                ts[name].append(us / calls)
    base = statistics.median(ts["plain"])
    for name, t in ts.items():
        med = statistics.median(t)
        print(f"ce {N}x{V} {name:24s} median_us={med:8.1f} min_us={min(t):8.1f} max_us={max(t):8.1f} "
              f"TB/s={2 * N * V * 2 / med / 1e6:.2f} vs_plain={med / base:.3f}", flush=True)
    print(f"ce {N}x{V} plain spread (max - min) / median = {(max(ts['plain']) - min(ts['plain'])) / base:.3%}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z-loss", type=float, default=0.0)
    ap.add_argument("--softcap", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    _lib.require()
    if not a.z_loss and not a.softcap:
        return plain_only()
    variants = {"plain": None, "aux(z=0,cap=0)": (0.0, 0.0)}
    if a.z_loss:
        variants[f"aux(z={a.z_loss:g})"] = (a.z_loss, 0.0)
    if a.softcap:
        variants[f"aux(cap={a.softcap:g})"] = (0.0, a.softcap)
    if a.z_loss and a.softcap:
        variants[f"aux(z={a.z_loss:g},cap={a.softcap:g})"] = (a.z_loss, a.softcap)
    for N, V in SHAPES:
        interleaved(N, V, variants, a.rounds)


if __name__ == "__main__":
    main()
