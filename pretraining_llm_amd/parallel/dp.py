"""Data-parallel gradient engine on RCCL (torch.distributed backend "nccl" on ROCm).

Reference: ``DDP(model, device_ids=[local_rank])`` (scripts/train_transformer.py:122-123)
with default 25 MiB buckets, a constant-buffer broadcast every other forward
 and a sync toggle that skipped the all-reduce on odd steps
while still stepping the optimizer (defect D5: replicas diverge).

This engine instead:
* works on the optimizer's flat gradient buffer (``FlatAdamW.flat_grad``), so a
  bucket is a contiguous slice -> zero packing copies, one RCCL call per bucket;
* forms buckets in REVERSE layout order (backward produces the last layers'
  gradients first) with a small first bucket so communication starts early, and
  launches each bucket from a post-accumulate-grad hook as soon as all its
  parameters are ready, strictly in bucket order (identical collective order on
  every rank), so the all-reduces run on RCCL's stream under the rest of the
  backward;
* sizes buckets for xGMI: each MI355X has 7 point-to-point links (~153 GB/s
  each); a ring all-reduce moves 2(n-1)/n * S per GPU, so buckets of 32-64 MiB
  keep per-call latency (tens of us) < 5% of transfer time while leaving
  several buckets to pipeline behind the backward;
* never reduces buffers (there are no mask buffers to broadcast), broadcasts
  parameters once at construction (one flat collective), and leaves the
  1/world averaging to the optimizer's gradient scale (no extra pass);
* ``no_sync()`` gives correct gradient accumulation (sync only on the last
  micro-step).
"""
from __future__ import annotations

import contextlib
from typing import List, Optional

import torch
import torch.distributed as dist

from .. import ops as _ops_mod
from ..ab import ab as _ab


class CommTimer:
    """Where a DP step's communication time went, from HIP events on the compute stream (no host
    sync inside the step): ``start()`` at the beginning of a step, ``launch(b)`` when bucket b's
    collective is issued (its offset into the step = how early the backward released it),
    ``backward_end()`` when ``finish_grad_sync`` is entered (the backward's last kernel is queued)
    and ``sync_end()`` once the compute stream has waited for every collective.  The exposed
    communication of a step is backward_end -> sync_end: the time the compute stream stalls on
    RCCL after the backward (the un-overlapped tail).  Read with ``report()`` after a device sync."""

    def __init__(self, enabled: bool):
        self.enabled = bool(enabled) and torch.cuda.is_available()
        self.steps = []  # per step: dict of events
        self._cur = None

    def _ev(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def start(self):
        if self.enabled:
            self._cur = {"start": self._ev(), "launch": {}}

    def launch(self, b: int):
        if self.enabled and self._cur is not None:
            self._cur["launch"][b] = self._ev()

    def backward_end(self):
        if self.enabled and self._cur is not None:
            self._cur["bwd_end"] = self._ev()

    def sync_end(self):
        if self.enabled and self._cur is not None and "bwd_end" in self._cur:
            self._cur["sync_end"] = self._ev()
            self.steps.append(self._cur)
        self._cur = None

    def reset(self):
        self.steps, self._cur = [], None

    def report(self) -> dict:
        """Mean exposed communication ms/step and, for the last step, each bucket's launch offset
        (ms after the step started) and the backward's end offset."""
        if not self.steps:
            return {"exposed_comm_ms": 0.0 if not self.enabled else None, "steps_timed": 0}
        exp = [st["bwd_end"].elapsed_time(st["sync_end"]) for st in self.steps]
        last = self.steps[-1]
        t0 = last["start"]
        return {"exposed_comm_ms": round(sum(exp) / len(exp), 3), "exposed_comm_ms_max": round(max(exp), 3),
                "steps_timed": len(exp),
                "backward_end_ms": round(t0.elapsed_time(last["bwd_end"]), 3),
                "bucket_launch_ms": [round(t0.elapsed_time(last["launch"][b]), 3) for b in sorted(last["launch"])]}


class DataParallelEngine:
    def __init__(self, optimizer, process_group=None, bucket_mb: float = 64.0, first_bucket_mb: float = 4.0,
                 broadcast_params: bool = True, overlap: bool = True, timing: bool = False):
        self.opt = optimizer
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # whether gradients are all-reduced: world > 1, or (PLLM_AB dp_world1=1, debug only) a world-1 process
        # group -- the hooks, bucket launches and waits of the world > 1 step then run over a one-rank RCCL
        # communicator, a rehearsal of the multi-GPU path on a one-GPU box (tests/test_dp_gpu.py)
        self.sync = self.world > 1 or (dist.is_initialized() and _ab("dp_world1", False))
        self.overlap = overlap
        self.timer = CommTimer(timing and optimizer.flat_grad.is_cuda)
        self.enabled = True
        self._handles = []
        self._hooks = []
        flat = optimizer.flat_grad
        esz = flat.element_size()
        params = optimizer.params
        # layout order of params by offset
        order = sorted(range(len(params)), key=lambda i: optimizer.offsets[i])
        # buckets: walk from the END of the flat buffer backwards
        self.buckets: List[dict] = []
        cap = int(first_bucket_mb * 2 ** 20)
        cur: List[int] = []
        cur_bytes = 0
        for i in reversed(order):
            nbytes = params[i].numel() * esz
            if cur and nbytes >= cap:
                # a parameter at least a bucket in size gets a bucket of its own: the tied embedding (the
                # last gradient of the backward, 154 MiB fp32 at GPT-2 small) would otherwise hold back the
                # first block's parameters in the un-overlappable tail bucket (195 MiB -> 154 MiB)
                self._close_bucket(cur)
                cur, cur_bytes = [], 0
                cap = int(bucket_mb * 2 ** 20)
            cur.append(i)
            cur_bytes += nbytes
            if cur_bytes >= cap:
                self._close_bucket(cur)
                cur, cur_bytes = [], 0
                cap = int(bucket_mb * 2 ** 20)
        if cur:
            self._close_bucket(cur)
        self.param_bucket = {}
        for b, bk in enumerate(self.buckets):
            for i in bk["params"]:
                self.param_bucket[i] = b
        # A parameter's gradient can land in several pieces (a tied embedding gets the LM-head
        # GEMM and the embedding scatter; kernels that add straight into the flat buffer signal
        # through ``p._pllm_grad_ready`` instead of autograd's post-accumulate hook).  The number
        # of pieces per parameter is learned in the first synchronised backward (which launches
        # every bucket at the end, no overlap); afterwards a parameter is ready when all its
        # pieces have arrived.
        self._expected: Optional[List[int]] = None
        self._events = [0] * len(params)
        self._reset_counters()
        if broadcast_params and self.sync:
            dist.broadcast(optimizer.flat_param, src=self._global_src(), group=process_group)
            optimizer.sync_master_from_params()
        if self.sync:
            _ops_mod.wgrad_defer_allow(False)  # gradient notifications launch the buckets: none is held back
        if self.sync and overlap:
            for i, p in enumerate(params):
                h = self._make_hook(i)
                self._hooks.append(p.register_post_accumulate_grad_hook(lambda _p, h=h: h()))
                p._pllm_grad_ready = h

    def _global_src(self):
        if self.pg is None:
            return 0
        return dist.get_global_rank(self.pg, 0)

    def _close_bucket(self, idx: List[int]):
        opt = self.opt
        starts = [opt.offsets[i] for i in idx]
        ends = [opt.offsets[i] + opt.params[i].numel() for i in idx]
        s = min(starts)
        # extend to the aligned end of the last param segment so the bucket tiles the buffer
        e = max(ends)
        self.buckets.append({"params": list(idx), "start": s, "end": e})

    def _reset_counters(self):
        if self._expected is None:
            self._pending = [len(b["params"]) for b in self.buckets]
        else:
            self._pending = [sum(1 for i in b["params"] if self._expected[i] > 0) for b in self.buckets]
        self._events = [0] * len(self._events)
        self._next_launch = 0
        self._handles = []

    def _make_hook(self, i):
        def hook():
            if not self.enabled:
                return
            self._events[i] += 1
            if self._expected is None or self._events[i] != self._expected[i]:
                return
            b = self.param_bucket[i]
            self._pending[b] -= 1
            if self._pending[b] == 0:
                self._launch_ready()
        return hook

    def _launch(self, b):
        bk = self.buckets[b]
        # lazy zeroing: a weight of this bucket that no writer touched this step (unused on this rank)
        # still holds last step's gradient -- zero it before it enters the all-reduce
        clear = getattr(self.opt, "_clear_unwritten", None)
        if clear is not None:
            clear(bk["params"])
        view = self.opt.flat_grad[bk["start"]:bk["end"]]
        self.timer.launch(b)
        self._handles.append(dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.pg, async_op=True))

    def _launch_ready(self):
        while self._next_launch < len(self.buckets) and self._pending[self._next_launch] == 0:
            self._launch(self._next_launch)
            self._next_launch += 1

    # ------------------------------------------------------------------
    @contextlib.contextmanager
    def no_sync(self):
        old = self.enabled
        self.enabled = False
        try:
            yield
        finally:
            self.enabled = old

    def finish_grad_sync(self):
        """Launch any bucket not yet launched (unused params, no-overlap mode) and wait for all.
        Returns the gradient scale the optimizer must apply (1/world)."""
        _ops_mod.wgrad_flush()
        self.timer.backward_end()
        if self.sync:
            while self._next_launch < len(self.buckets):
                self._launch(self._next_launch)
                self._next_launch += 1
            for h in self._handles:
                h.wait()
            if self._expected is None and self.enabled and any(self._events):
                self._expected = list(self._events)
        self.timer.sync_end()
        self._reset_counters()
        return 1.0 / self.world

    def bucket_sizes_mb(self):
        esz = self.opt.flat_grad.element_size()
        return [(b["end"] - b["start"]) * esz / 2 ** 20 for b in self.buckets]

    def remove_hooks(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []


def all_reduce_mean(t: torch.Tensor, group=None) -> torch.Tensor:
    """Mean of a (scalar) tensor over ranks; identity when not distributed."""
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        t = t.clone()
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        t /= dist.get_world_size(group)
    return t


@torch.no_grad()
def params_checksum(params) -> torch.Tensor:
    """fp64 checksum of all parameters (cross-rank replica-consistency check, catches SURVEY D5)."""
    s = torch.zeros((), dtype=torch.float64, device=params[0].device)
    for i, p in enumerate(params):
        s += p.double().sum() * (1.0 + 1e-3 * (i % 97))
    return s
