"""Fused ops with autograd: HIP (gfx950) kernels on GPU, PyTorch reference on CPU.

Every op here is a ``torch.autograd.Function`` whose forward/backward call
``torch.ops.pllm.*`` (hand-written HIP kernels in ``pretraining_llm_amd/csrc``)
when its inputs live on the GPU, and the reference in ``reference.py``
otherwise.  There is no third path: a GPU tensor with a missing extension
raises (see ``_lib.require``).

``set_backend("torch")`` forces stock PyTorch ops everywhere (SDPA attention,
F.layer_norm, F.cross_entropy in fp32 like the reference's autocast); it exists
only to measure the stock-PyTorch baseline on the same model and
is never selected implicitly.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from ..ab import ab as _ab
from . import _lib
from . import reference as ref

_BACKEND = "auto"   # auto -> HIP for GPU tensors, reference for CPU tensors; "torch" -> stock torch always


def set_backend(name: str):
    global _BACKEND
    assert name in ("auto", "torch"), name
    _BACKEND = name


def get_backend() -> str:
    return _BACKEND


@contextlib.contextmanager
def backend(name: str):
    old = _BACKEND
    set_backend(name)
    try:
        yield
    finally:
        set_backend(old)


def _hip(*ts) -> bool:
    return _BACKEND == "auto" and _lib.use_hip(*ts)


# Numerics bisection (diagnostic): PLLM_TORCH_OPS=attn,norm,act,ce,embed,linear runs the named op
# families through stock PyTorch ops while everything else stays on the HIP kernels
# (scripts/convergence.py compares the resulting loss curves against fp32).
_TORCH_OPS = frozenset(x for x in os.environ.get("PLLM_TORCH_OPS", "").split(",") if x)


def _hip_op(name: str, *ts) -> bool:
    return name not in _TORCH_OPS and _hip(*ts)


def _stock(name: str) -> bool:
    """True when op family ``name`` runs on stock torch ops (torch backend, or bisected out)."""
    return _BACKEND == "torch" or name in _TORCH_OPS


def _ops():
    return _lib.require()


# ---------------------------------------------------------------------------
# Direct gradient accumulation.  When the optimizer owns a flat gradient
# buffer (train/optim.py FlatAdamW marks its params ``_pllm_flat_grad``), the
# backward kernels/GEMMs ADD their weight gradients straight into
# ``p._pllm_gradbuf`` (a view of that buffer, fp32 by default: in-kernel
# read-add-write epilogues) instead of returning a fresh tensor that autograd's
# AccumulateGrad would then add in a separate pass.  The data-parallel engines
# count each parameter's notifications and the optimizer expects a slot's
# freshness flag consumed once per step, so every writer follows one sequence:
# ``_take`` the slots its kernel writes (all or none), write, ``_wrote`` -- or,
# without slots, return fresh tensors and tell nobody.  Nothing else in this
# package touches a parameter's slot attributes.
# ---------------------------------------------------------------------------
def _slot(p):
    """``p``'s slot of the flat gradient; None without one or while another writer holds it reserved."""
    free = getattr(p, "_pllm_flat_grad", False) and not getattr(p, "_pllm_grad_reserved", False)
    return getattr(p, "_pllm_gradbuf", None) if free else None


def _take(*params, whole: bool = False):
    """The flat-gradient slots of the parameters one kernel writes together, one per parameter (a None entry --
    the layer has no such parameter -- stays None), all or nothing: when one of them has no slot to give, every
    entry is None and no flag or buffer has been touched.  A slot the optimizer left uncleared (fresh: lazy
    zeroing, ``FlatAdamW(lazy_zero=True)``) is zeroed here, so an ADDING writer is right whatever ran first.
    ``whole``: the writer produces the entire gradient (the weight-gradient GEMM, ``qk_norm_bwd_``,
    ``attn_sink_bwd``) -> (slots, overwrite): with every slot fresh nothing is zeroed and the kernel stores
    instead of adding -- no zero fill, no read of zeros; else the fresh ones are zeroed and it adds."""
    if any(getattr(p, "_pllm_wgrad_queued", False) for p in params):
        wgrad_flush()  # a queued weight gradient (deferred mode of _weight_grad) lands before the next writer's
    slots, overwrite = tuple(_slot(p) for p in params), False
    if any(s is None and p is not None for s, p in zip(slots, params)):
        slots = (None,) * len(params)
    else:
        fresh = [p for p in params if getattr(p, "_pllm_grad_fresh", False)]
        overwrite = whole and len(fresh) == sum(s is not None for s in slots) > 0
        for p in fresh:
            p._pllm_grad_fresh = False
            if not overwrite:
                p._pllm_gradbuf.zero_()
    return (slots, overwrite) if whole else slots


def _wrote(*params):
    """Tell the parameters (None entries skipped), in this order, that their slots were written."""
    for cb in (getattr(p, "_pllm_grad_ready", None) for p in params):
        if cb is not None:
            cb()


def _reserve(p):
    """``p``'s slot for a writer that stores the whole gradient now and finishes it in a later call (the LM
    head: written in its forward, scaled in place in its backward); only a fresh contiguous fp32 slot.  Until
    ``_release`` every other taker finds no slot and returns a tensor, which autograd's AccumulateGrad hands
    to the optimizer's hook after the last producer: the in-place scale never covers another writer's part."""
    buf = _slot(p) if getattr(p, "_pllm_grad_fresh", False) else None
    if buf is None or buf.dtype != torch.float32 or not buf.is_contiguous():
        return None
    p._pllm_grad_fresh, p._pllm_grad_reserved = False, True
    return buf


def _release(p):
    """End ``p``'s reservation -> its slot."""
    p._pllm_grad_reserved = False
    return p._pllm_gradbuf


def _linear_param_grads(dy2, x2, w, b, need_w: bool = True, need_b: bool = True, fuse_bias: bool = True):
    """(dw, db) of y = x W^T + b from dy2 [rows, N] and x2 [rows, K]: each goes into its parameter's flat-gradient
    slot (None is returned for it and the parameter is notified, weight before bias) or comes back as a fresh
    tensor.  The weight-gradient GEMM writes the whole of dW (``_take(w, whole=True)``); with ``fuse_bias`` the bias
    gradient rides along it when both have slots (FUSED_WGRAD_BIAS), else it is a ``bias_grad`` pass of its own."""
    dw = db = None
    need_b = need_b and b is not None
    if need_w:
        (tgt,), fresh = _take(w, whole=True)
        # (no weight slot: no fused bias target either, the bias takes the separate pass below)
        (btgt,) = _take(b) if need_b and fuse_bias and tgt is not None and FUSED_WGRAD_BIAS else (None,)
        # (told of their slots' writes by _weight_grad: at once, or after the queued launch that completes them)
        dw = _weight_grad(dy2, x2, tgt, btgt, overwrite=fresh,
                          notify=(w if tgt is not None else None, b if btgt is not None else None))
        if btgt is not None:
            need_b = False
    if need_b:
        db = _bias_param_grad(dy2, b)
    return dw, db


def _bias_param_grad(dy2, b):
    """Column sums of dy2 added into ``b``'s flat-gradient slot (-> None, ``b`` notified), else returned."""
    (tgt,) = _take(b)
    if tgt is None:
        return _ops().bias_grad(dy2.contiguous())
    _ops().bias_grad(dy2.contiguous(), tgt)
    _wrote(b)
    return None


def _bias_grad_by(b, run):
    """(run(acc), db) for a kernel ``run`` that adds ``b``'s gradient into ``acc`` beside its own work (a GEMM
    epilogue's column sums): ``acc`` is b's flat-gradient slot (db None, ``b`` notified) or fresh fp32 zeros."""
    (tgt,) = _take(b)
    acc = tgt if tgt is not None else torch.zeros(b.shape[0], device=b.device, dtype=torch.float32)
    out = run(acc)
    if tgt is None:
        return out, acc.to(b.dtype)
    _wrote(b)
    return out, None


def _bias_ext(flag, b) -> bool:
    """A bias gradient is left to the consumer's backward kernel (the next norm's dx column sums, the activation
    backward) only while that consumer runs on the HIP kernels."""
    return bool(flag and b is not None and not (_TORCH_OPS & {"norm", "act"}))


def _gemm_lt(x2, w, b, epilogue: int = 0, res2=None):
    """x2 W^T + b (+ res2, added by the GEMM: one rounding) on hipBLASLt with epilogue 0 none / 2 ReLU; contiguous
    2-D operands.  Deterministic mode pins the first candidate instead of timing them."""
    return _ops().gemm_lt(x2, w, b, epilogue, not torch.are_deterministic_algorithms_enabled(), res2)[0]


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b on hipBLASLt; backward accumulates dW (beta=1 GEMM) and db in place.

    ``bias_grad_external``: the bias gradient is produced by the consumer's backward kernel
    (the next norm's dx column sums, or the activation backward), so this function leaves it
    alone instead of re-reading dy."""

    @staticmethod
    def forward(ctx, x, weight, bias, bias_grad_external, res=None):
        ctx.save_for_backward(x, weight)
        ctx.w, ctx.b = weight, bias
        ctx.bias_ext = bias_grad_external
        ctx.has_res = res is not None
        if res is not None:  # + the residual stream, added by the GEMM (resid_gemm_ok)
            N = weight.shape[0]
            # (gemm_lt takes contiguous operands only; reshape of a strided view can stay strided)
            return _gemm_lt(x.reshape(-1, x.shape[-1]).contiguous(), weight, bias, 0,
                            res.reshape(-1, N)).view(*x.shape[:-1], N)
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = _dgrad(dy, weight) if ctx.needs_input_grad[0] else None
        dw, db = _linear_param_grads(dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1]), ctx.w, ctx.b,
                                     ctx.needs_input_grad[1], ctx.needs_input_grad[2] and not ctx.bias_ext)
        ctx.w = ctx.b = None
        return dx, dw, db, None, (dy if ctx.has_res else None)


# weight-gradient GEMM engine: "hip" = hand-written split-K MFMA kernel (csrc/gemm_wgrad.hip),
# default: 824-1114 TFLOP/s at M=65536 vs 432-1003 for hipBLASLt's token-major "NT" kernels
# (bench/gemm_bench.py, profiles/r1_wgrad_v2_gemm_bench.jsonl); "blas" = hipBLASLt/rocBLAS
# through torch (beta=1 addmm into the flat gradient)
WGRAD_ENGINE = os.environ.get("PLLM_WGRAD", "hip")
# (tokens M, P, Q) weight-gradient shapes where hipBLASLt measured faster than the hand-written
# kernel on MI355X (bench/gemm_bench.py --shapes llama --M 16384, profiles/r1_wgrad_plan_ab.jsonl):
# llama-1.3B at 8 x 2048 tokens -- QKV, MLP down projection and LM head
WGRAD_BLAS_SHAPES = {(16384, 6144, 2048), (16384, 2048, 5504), (16384, 50304, 2048)}


# (Weight gradients on a side HIP stream were measured and removed: +1.5 % on one box, -0.8 % on
# another, sporadic 2.5-3x slower runs; profiles/r1_wgrad_side_stream_ab.txt.)
# A linear layer's bias gradient computed inside its weight-gradient GEMM (csrc/gemm_wgrad.hip: MFMAs
# against an all-ones operand by the first Q-tile's workgroups) instead of a separate column-sum pass
# over dy (the GPT-2 QKV projection); PLLM_AB=wgrad_bias=0 for the separate pass
FUSED_WGRAD_BIAS = _ab("wgrad_bias", True)


def _shadow(w):
    """The transposed shadow W^T the optimizer keeps of ``w`` (FlatAdamW ``transposed_shadow``), or None without
    one or when ``w`` changed since its last refresh."""
    wt = getattr(w, "_pllm_wT", None)
    return wt if wt is not None and getattr(w, "_pllm_wT_ver", None) == w._version else None


def _shadow_or_t(w):
    """W^T contiguous: the shadow when it is current, else a transposed copy."""
    wt = _shadow(w)
    return wt if wt is not None else w.t().contiguous()


def _dgrad(dy, weight):
    """dx = dy @ weight.  When the optimizer keeps a transposed shadow of the weight
    (FlatAdamW ``transposed_shadow``), the product runs as dy @ (W^T)^T: hipBLASLt's
    kernels for that operand layout are 10-15% faster at these shapes than for
    dy @ W (bench/gemm_fwd_bench.py: dgrad_nt vs dgrad_nn)."""
    wt = _shadow(weight)
    return dy @ (wt.t() if wt is not None else weight)


def _weight_grad(dy2, x2, tgt, btgt=None, overwrite: bool = False, notify=()):
    """dW = dy2^T @ x2, added into ``tgt`` (bf16 or fp32) when given (returns None) else returned;
    ``overwrite``: stored into ``tgt`` instead (its first write of the step, ``_take(.., whole=True)``).
    ``btgt`` (with ``tgt``): the bias gradient (column sums of dy2) is added into it as well -- on the
    hand-written kernel inside the GEMM (its all-ones MFMAs), else by the bias_grad kernels.
    ``notify``: the parameters whose slots ``tgt`` / ``btgt`` are, told (``_wrote``, in this order) once the
    slots hold the result -- before this returns, or, in the DEFERRED mode, later: a call with ``notify`` that
    the hand-written kernel serves with fp32 slots may be queued (``_WgradQueue``, when ``_wgrad_defer_on``)
    and run with other layers' as whole tiles of one grouped launch."""
    hip_ok = dy2.shape[1] % 8 == 0 and x2.shape[1] % 8 == 0 and dy2.shape[0] % 64 == 0
    f32_tgt = tgt is not None and tgt.dtype == torch.float32 and dy2.dtype != torch.float32
    # an fp32 gradient target always takes the hand-written kernel (fp32 read-add-write epilogue)
    use_hip = hip_ok and (f32_tgt or (WGRAD_ENGINE == "hip" and
                                      (dy2.shape[0], dy2.shape[1], x2.shape[1]) not in WGRAD_BLAS_SHAPES))
    if use_hip:
        dy2, x2 = dy2.contiguous(), x2.contiguous()
        if tgt is not None:
            out = tgt.view(dy2.shape[1], x2.shape[1])
            if (notify and f32_tgt and (btgt is None or btgt.dtype == torch.float32) and _wgrad_defer_on(dy2)
                    and _wgrad_sliced(dy2, x2, btgt) and _WGRAD_QUEUE.push(dy2, x2, out, btgt, overwrite, notify)):
                return None
            _ops().wgrad(dy2, x2, out, btgt, overwrite)
            _wrote(*notify)
            return None
        return _ops().wgrad(dy2, x2)
    if btgt is not None:
        _ops().bias_grad(dy2.contiguous(), btgt)
    if tgt is not None:
        if f32_tgt:
            dw = (torch.mm(dy2.t(), x2, out_dtype=torch.float32) if dy2.is_cuda
                  else dy2.t().float() @ x2.float())
            tgt.copy_(dw.view_as(tgt)) if overwrite else tgt.add_(dw.view_as(tgt))
        elif overwrite:
            torch.mm(dy2.t(), x2, out=tgt.view(dy2.shape[1], x2.shape[1]))
        else:
            tgt.addmm_(dy2.t(), x2)
        _wrote(*notify)
        return None
    return dy2.t() @ x2


# ---------------------------------------------------------------------------
# Deferred weight gradients.  Nothing reads a weight gradient before the optimizer, and one layer's GEMM has
# fewer 256 x 256 output tiles than the GPU has CUs (a GPT-2 small block: 27 + 9 + 36 + 36), so alone it is
# split along the tokens into fp32 slabs that a reduce pass sums.  Queued, the layers' tiles fill whole rounds
# of the grid: each tile runs over all tokens in one workgroup and is written once (the grouped arm of
# csrc/wgrad_pp.hip), with no slabs and no reduce.  Only what is left at the end of the backward -- less than
# one round -- is sliced as before.  PLLM_AB wgrad_defer=0: every weight gradient at once.
# ---------------------------------------------------------------------------
WGRAD_DEFER = _ab("wgrad_defer", True)
WGRAD_TILE = 256          # csrc/gemm_plan.h kPlanTile
WGRAD_GROUP_MAX = 16      # csrc/gemm_plan.h kWgradGroupMax
WGRAD_DEFER_MIN_SLICES = 2  # queue what the immediate plan would cut into this many token slices or more
_wgrad_defer_engine = True  # wgrad_defer_allow: off while an engine launches collectives from gradient hooks


def wgrad_defer_allow(on: bool) -> None:
    """The data-parallel engines switch deferral off when they launch collectives from the parameters'
    gradient notifications (more than one rank: a notification held back holds a bucket's all-reduce back,
    and the grouped launch takes every CU), the single-rank optimizer switches it on."""
    global _wgrad_defer_engine
    wgrad_flush()
    _wgrad_defer_engine = bool(on)


def _wgrad_defer_on(dy2) -> bool:
    """Deferred mode for this call: PLLM_AB wgrad_defer (default 1), the HIP path, one rank."""
    if not (WGRAD_DEFER and _wgrad_defer_engine and _hip(dy2)) or dy2.shape[0] < 128:
        return False
    dist = torch.distributed
    return not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)


def _wgrad_sliced(dy2, x2, btgt) -> bool:
    """Whether the immediate launch of this problem would be split along the tokens (``wgrad_plan``: at least
    WGRAD_DEFER_MIN_SLICES slices).  Only those are queued: a problem that already runs as whole tiles writes
    no slabs and has no reduce pass to save, so it runs in its layer's backward as before."""
    S = _ops().wgrad_plan(dy2.shape[0], dy2.shape[1], x2.shape[1], True, btgt is not None)[1]
    return S >= WGRAD_DEFER_MIN_SLICES


class _WgradQueue:
    """Queued weight-gradient problems (dy2, x2, out [P, Q] fp32, bias slot or None, overwrite, parameters to
    tell) in arrival order, the operands held by reference.  Their tiles form one list, a problem's tiles row
    band by row band; ``done0`` tiles of the first problem have run.  ``push`` launches the whole rounds of the
    grid the queue holds (``torch.ops.pllm.wgrad_group_plan`` cuts them, at row-band boundaries inside a
    problem) and keeps the rest; the flush at the end of the backward launches the last whole rounds and hands
    what is left -- the unfinished row bands of the first problem as a [rows, Q] problem of their own, then the
    others -- to ``torch.ops.pllm.wgrad``, sliced as an immediate call would be.  A parameter is told of its
    slot's write after the launch that ran its problem's last tile, weight before bias, in queue order."""

    def __init__(self):
        self.items, self.done0, self.armed = [], 0, False

    # the three calls into the extension (tests/test_wgrad_queue.py replaces them with recorders)
    def plan(self, tiles, tiles_q, done0):
        return _ops().wgrad_group_plan(tiles, tiles_q, done0)

    def run_group(self, items, first, last):
        empty = items[0][0].new_empty(0, dtype=torch.float32)
        _ops().wgrad_group([it[0] for it in items], [it[1] for it in items], [it[2] for it in items],
                           [empty if it[3] is None else it[3] for it in items], [int(it[4]) for it in items],
                           first, last)

    def run_single(self, dy2, x2, out, btgt, overwrite):
        _ops().wgrad(dy2, x2, out, btgt, overwrite)

    @staticmethod
    def _tiles(it):
        tq = -(-it[2].shape[1] // WGRAD_TILE)
        return -(-it[2].shape[0] // WGRAD_TILE) * tq, tq

    def push(self, dy2, x2, out, btgt, overwrite, notify) -> bool:
        """Queue one problem -> False when no flush can be registered (not inside a backward): the caller
        runs it at once."""
        if not self.armed:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(self.flush)
            except RuntimeError:
                return False
            self.armed = True
        for p in notify:
            if p is not None:
                p._pllm_wgrad_queued = True
        self.items.append((dy2, x2, out, btgt, overwrite, tuple(notify)))
        self._launch_rounds()
        return True

    def _done(self, it):
        for p in it[5]:
            if p is not None:
                p._pllm_wgrad_queued = False
        _wrote(*it[5])

    def _launch_rounds(self):
        while self.items:
            head = self.items[:WGRAD_GROUP_MAX]
            counts = [self._tiles(it) for it in head]
            take = int(self.plan([c[0] for c in counts], [c[1] for c in counts], self.done0)[0])
            if take <= 0:
                return
            first, last, n, end = self.done0, self.done0 + take, 0, 0
            while n < len(head) and end < last:  # the problems the range touches
                end += counts[n][0]
                n += 1
            self.run_group(head[:n], first, last)
            whole = n if end == last else n - 1  # the last one touched may be cut
            for it in head[:whole]:
                self._done(it)
            self.done0 = last - (end - counts[n - 1][0]) if whole < n else 0
            del self.items[:whole]

    def flush(self):
        """Everything queued lands: whole rounds grouped, the rest one problem at a time."""
        self.armed = False
        if not self.items:
            return
        self._launch_rounds()
        items, done0 = self.items, self.done0
        self.items, self.done0 = [], 0
        for i, it in enumerate(items):
            dy2, x2, out, btgt, overwrite = it[:5]
            if i == 0 and done0:  # its first row bands ran in a grouped launch: the rest as [rows, Q]
                r0 = done0 // self._tiles(it)[1] * WGRAD_TILE
                dy2, out, btgt = dy2[:, r0:], out[r0:], None if btgt is None else btgt[r0:]
            self.run_single(dy2, x2, out, btgt, overwrite)
            self._done(it)


_WGRAD_QUEUE = _WgradQueue()


def wgrad_flush() -> None:
    """Run every queued weight gradient now.  Registered for the end of each backward through the autograd
    engine's callback; every reader of the gradient slots in this package calls it first as well."""
    _WGRAD_QUEUE.flush()


# ---------------------------------------------------------------------------
# Weight-only FP8 (OCP e4m3fn) decode weights: a per-row quantised CACHE of a bf16 weight that only the
# skinny GEMM reads (csrc/gemv.hip FP8 arms, <= 8 token rows, no grad).  Everything else -- prefill,
# training, more than 8 rows -- keeps reading ``ref``, the bf16 parameter it was made from.
# ---------------------------------------------------------------------------
FP8_MAX = 448.0     # largest finite e4m3fn value
FP8_K_CHUNK = 8     # codes a lane of the FP8 skinny GEMM loads per step: K must be a multiple


class Fp8Weight:
    """``ref`` [N, K] (the bf16 parameter), ``q`` uint8 [N, K] e4m3fn codes, ``scale`` fp32 [N]:
    ref ~= dequantize_fp8(q, scale).  Accepted as ``weight`` by ``linear`` / ``norm_linear``."""
    __slots__ = ("ref", "q", "scale", "shape")

    def __init__(self, ref, q, scale):
        self.ref, self.q, self.scale, self.shape = ref, q, scale, ref.shape


def quantize_weight_fp8(w) -> Optional[Fp8Weight]:
    """Per-row e4m3fn quantisation of a weight [N, K] (csrc/quant_fp8.hip for bf16 on the GPU, ``ops.reference`` on
    the CPU); None when the FP8 skinny GEMM cannot take it (K not a multiple of 8, not contiguous, a GPU weight
    that is not on the HIP path).  Non-finite weights raise ValueError."""
    if w.dim() != 2 or w.shape[1] == 0 or w.shape[1] % FP8_K_CHUNK or not w.is_contiguous():
        return None
    if w.is_cuda and not (_lib.use_hip(w) and _lib.available()):
        return None
    wd = w.detach()
    if not bool(torch.isfinite(wd).all()):
        raise ValueError("quantize_weight_fp8: the weight holds non-finite values")
    q, scale = _ops().quantize_rows_fp8(wd) if w.is_cuda else ref.quantize_rows_fp8(wd)
    return Fp8Weight(w, q, scale)


def dequantize_fp8(q, scale):
    """fp32 [N, K] = e4m3fn value of each code times its row's scale."""
    return ref.dequantize_fp8(q, scale)


def _fp8_rows_ok(x) -> bool:
    """An inference call of at most 8 token rows: the only calls that read the quantised weight."""
    K = x.shape[-1]
    return not torch.is_grad_enabled() and K > 0 and 0 < x.numel() // K <= 8


def _linear_fp8(x, fw: Fp8Weight, bias):
    """x W^T + b from the quantised weight, or None when this call keeps the bf16 weight (more than 8 rows, grad
    mode).  HIP: the FP8 skinny GEMM; CPU / torch backend: ``ops.reference`` on the dequantised weight."""
    if not _fp8_rows_ok(x):
        return None
    if _gemv_shape_ok(x, fw.q) and x.dtype == fw.ref.dtype:
        y = _ops().gemv_fp8(x.reshape(-1, x.shape[-1]).contiguous(), fw.q, fw.scale, bias)[0]
        return y.view(*x.shape[:-1], fw.shape[0])
    if _hip(x):
        return None
    return ref.linear_fp8(x, fw.q, fw.scale, bias)


def linear(x, weight, bias=None, bias_grad_external: bool = False, residual=None):
    """``residual`` (only when resid_gemm_ok holds -- the caller checks): x W^T + b + residual.
    ``weight`` may be an ``Fp8Weight``: decode-sized inference calls read its codes, every other its ``ref``."""
    if isinstance(weight, Fp8Weight):
        y = _linear_fp8(x, weight, bias) if residual is None else None
        if y is not None:
            return y
        weight = weight.ref
    if _hip_op("linear", x) and torch.is_grad_enabled() and weight.requires_grad:
        return _LinearFn.apply(x, weight, bias, _bias_ext(bias_grad_external, bias), residual)
    if residual is not None:
        return F.linear(x, weight, bias) + residual
    # decode-sized inference projections: weight-streaming skinny GEMM (csrc/gemv.hip) instead of the
    # training-sized library tiles.  (Grad mode alone does not rule it out here as it does in _gemv_ok: a
    # frozen weight under an input that needs no gradient is still inference.)
    if not (torch.is_grad_enabled() and x.requires_grad) and _gemv_shape_ok(x, weight):
        y = _ops().gemv(x.reshape(-1, x.shape[-1]).contiguous(), weight, bias)[0]
        return y.view(*x.shape[:-1], weight.shape[0])
    return F.linear(x, weight, bias)


# ---------------------------------------------------------------------------
# MLP with the activation in the GEMM epilogues (csrc/gemm.hip)
# ---------------------------------------------------------------------------
def gemm_config(reserve_cus: Optional[int] = None, persistent: Optional[bool] = None) -> bool:
    """Configure the hand-written fused-epilogue TN GEMM (``torch.ops.pllm.gemm_tn``: the ping-pong main loop of
    csrc/gemm_pp.hip; shapes it does not take -- K < 128, the delta epilogue with T % 16 != 0 -- fall back to the
    one-barrier persistent loop of csrc/gemm.hip): ``reserve_cus``: CUs its persistent grid leaves free (RCCL
    kernels run beside the backward at world > 1); ``persistent`` False: the ping-pong GEMM and weight-gradient
    kernels launch one workgroup per tile / work item instead of one per CU, so a CU held by a concurrent RCCL
    kernel delays no tile list (the hardware deals the tiles to the free CUs).  None keeps the current
    setting; returns False without the extension (CPU)."""
    if not _lib.available():
        return False
    torch.ops.pllm.gemm_set_config(0, 0, -1, -1 if reserve_cus is None else int(reserve_cus),
                                   -1 if persistent is None else int(bool(persistent)))
    return True


# PLLM_FUSED_MLP: "bwd" (default) = forward on hipBLASLt + the activation kernel, backward through
# the fused data-gradient epilogue (act' + b1's gradient: 476-480 vs 512 us per GPT-2 layer, measured in
# round 3); "all" = the forward activation in the GEMM epilogue too (its main loop is
# still slower than hipBLASLt's: 423-440 vs 408 us with the separate GELU pass); "0" = neither
_FM = os.environ.get("PLLM_FUSED_MLP", "bwd")
FUSED_MLP = _FM in ("1", "all", "bwd")
FUSED_MLP_FWD = _FM in ("1", "all")
# PLLM_AB fused_swiglu_fwd=1|0: the llama up-projection with its SwiGLU in the GEMM epilogue (epilogue 7)
FUSED_SWIGLU_FWD = _ab("fused_swiglu_fwd", True)
# PLLM_AB lt_relu=1|0: the ReLU MLP's up-projection (reference architecture) with bias + ReLU in hipBLASLt's
# epilogue (csrc/blaslt.cpp) instead of the library GEMM + act_fwd pass (bench/gelu_epi_bench.py:
# 394 vs 494 us at the ref-3b shape).  GELU has no such path: the library build that ships with torch has
# no GELU epilogue with the pre-activation output the backward needs (HIPBLASLT_EPILOGUE_GELU_AUX*)
LT_RELU_FWD = _ab("lt_relu", True)


def fused_mlp_ok(x, w1, b1, w2, act: str) -> bool:
    """The fused path: GELU / ReLU MLPs with an up-projection bias on the HIP training path."""
    if not FUSED_MLP or act not in ("gelu", "relu") or b1 is None or not torch.is_grad_enabled():
        return False
    if not (_hip_op("linear", x) and _hip_op("act", x) and w1.requires_grad):
        return False
    C, Fh = x.shape[-1], w1.shape[0]
    return (C % 64 == 0 and Fh % 64 == 0 and x.numel() > 0 and tuple(w1.shape) == (Fh, C)
            and tuple(w2.shape) == (C, Fh) and w1.is_contiguous() and w2.is_contiguous()
            and _aligned16(w1) and _aligned16(w2) and b1.is_contiguous())


class _FusedMLPFn(torch.autograd.Function):
    """y = proj(act(hidden(x))) with the activation fused into the GEMM epilogues:

    forward   [pre,] a = act(x W1^T + b1)    one gemm_tn launch (GELU keeps the pre-activation);
                                             PLLM_FUSED_MLP=bwd: hipBLASLt + the activation kernel
              y = a W2^T + b2                hipBLASLt
    backward  dW2 += dy^T a, db2             (b2 skipped when the next norm emits it)
              da_pre = (dy W2) * act'(.)     one gemm_tn launch through W2's transposed shadow,
                                             + b1's gradient from the epilogue's column sums
              dx = da_pre W1, dW1 += da_pre^T x
    Gradient-ready notifications keep the unfused order (W2, b2, b1, W1) for the DP buckets.
    Reference: the MLP of /root/reference/src/models/mlp.py:24-26,39-41."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gelu, out_bias_ext, res=None):
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        if not FUSED_MLP_FWD and not gelu and LT_RELU_FWD:
            # ReLU in hipBLASLt's own bias epilogue: one pass writes the activation (the
            # backward needs only its sign); relu commutes with the bf16 rounding, so the result
            # equals the separate pass
            a = _gemm_lt(x2.contiguous(), w1, b1, 2)
            ctx.save_for_backward(x2, a)
        elif not FUSED_MLP_FWD:
            pre = F.linear(x2, w1, b1)
            a = _ops().act_fwd(pre, 1 if gelu else 0)
            if gelu:
                ctx.save_for_backward(x2, a, pre)
            else:
                ctx.save_for_backward(x2, a)
        elif gelu:
            a, pre = _ops().gemm_tn(x2, w1, b1, 1)
            ctx.save_for_backward(x2, a, pre)
        else:
            a, _ = _ops().gemm_tn(x2, w1, b1, 2)
            ctx.save_for_backward(x2, a)
        ctx.gelu, ctx.ext = gelu, out_bias_ext
        ctx.params = (w1, b1, w2, b2)
        ctx.xshape = x.shape
        ctx.has_res = res is not None
        if res is not None:  # the block's residual stream added in the GEMM (one rounding, see resid_gemm_ok)
            return _gemm_lt(a, w2, b2, 0, res.reshape(-1, C)).view(*x.shape[:-1], C)
        return F.linear(a, w2, b2).view(*x.shape[:-1], C)

    @staticmethod
    def backward(ctx, dy):
        if ctx.gelu:
            x2, a, pre = ctx.saved_tensors
        else:
            x2, a = ctx.saved_tensors
            pre = a
        w1, b1, w2, b2 = ctx.params
        ctx.params = None
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        # down projection: weight and bias gradients.  Two differences from _LinearFn, both kept: the weight
        # gradients are formed whatever needs_input_grad says, and b2's gradient is always a bias_grad pass of
        # its own (fused into the weight-gradient GEMM another kernel would form the sum: other bits)
        dw2, db2 = _linear_param_grads(dy2, a, w2, b2, need_b=not ctx.ext, fuse_bias=False)
        # its data gradient fused with the activation backward and b1's gradient (the epilogue's column sums)
        w2t = _shadow_or_t(w2)
        dpre, db1 = _bias_grad_by(b1, lambda acc: _ops().gemm_tn(dy2, w2t, None, 3 if ctx.gelu else 4, pre, acc)[0])
        # up projection
        dx = _dgrad(dpre, w1) if ctx.needs_input_grad[0] else None
        dw1, _ = _linear_param_grads(dpre, x2, w1, None)
        if dx is not None:
            dx = dx.view(ctx.xshape)
        return dx, dw1, db1, dw2, db2, None, None, (dy if ctx.has_res else None)


def fused_mlp(x, w1, b1, w2, b2, act: str, out_bias_ext: bool = False, residual=None):
    """``residual``: y + residual is returned (added by the down projection's GEMM, resid_gemm_ok)."""
    return _FusedMLPFn.apply(x, w1, b1, w2, b2, act == "gelu", _bias_ext(out_bias_ext, b2), residual)


# PLLM_AB resid_gemm=1|0: a block's residual add (reference: x = x + attn(ln1(x)); x = x + mlp(ln2(x)),
# /root/reference/src/models/transformer_block.py:44,46) done by its output projection's GEMM (hipBLASLt beta = 1,
# s = residual + x W^T + b in one rounding, csrc/blaslt.cpp gemm_lt) instead of by the next norm, which
# then reads one stream instead of two and writes one instead of two.  Round-4 measurement
# (profiles/r4_residual_in_gemm_negative.md): -3.9 / -15.9 us per GPT-2 layer (attention out / MLP down),
# -14.5 us at llama's attention output projection, but +105 us at its down projection (2048 x 5504: no fast
# beta = 1 solution among hipBLASLt's candidates), so weights of at most RESID_GEMM_MAX_W elements only.
# The size rule is a heuristic fitted to the measured shapes: its bound (4,194,304 = 2048 x 2048 = 1024 x 4096)
# admits exactly the measured-good ones among the presets -- GPT-2 small (768 x 768, 768 x 3072) and medium
# (1024 x 1024, 1024 x 4096) projections, llama's W_o (2048 x 2048) -- and none of the MLP downs of llama / ref-3b
# (2048 x 5504, 2048 x 8192) nor unmeasured mid-size ones (1024 x 5504, 1536 x 4096).  A new preset with a
# projection under the bound should have its beta = 1 GEMM re-measured (bench/residual_gemm_bench.py).
RESID_GEMM = _ab("resid_gemm", True)
RESID_GEMM_MAX_W = 2048 * 2048


def resid_gemm_ok(res, w) -> bool:
    return (RESID_GEMM and res is not None and torch.is_grad_enabled() and _hip(res) and not _TORCH_OPS
            and res.dtype == torch.bfloat16 and res.is_contiguous() and w.numel() <= RESID_GEMM_MAX_W
            and res.shape[-1] == w.shape[0] and w.shape[1] % 8 == 0)


def fused_swiglu_ok(x, w1, b1, w2, b2) -> bool:
    """The fused SwiGLU (llama) MLP: no biases, on the HIP training path (PLLM_FUSED_MLP != 0)."""
    if not FUSED_MLP or b1 is not None or b2 is not None or not torch.is_grad_enabled():
        return False
    if not (_hip_op("linear", x) and _hip_op("act", x) and w1.requires_grad):
        return False
    C, F2 = x.shape[-1], w1.shape[0]
    return (C % 64 == 0 and F2 % 16 == 0 and x.numel() > 0 and tuple(w1.shape) == (F2, C)
            and tuple(w2.shape) == (C, F2 // 2) and w1.is_contiguous() and w2.is_contiguous()
            and _aligned16(w1) and _aligned16(w2))


class _FusedSwiGLUMLPFn(torch.autograd.Function):
    """y = (silu(g) * u) W2^T with [g | u] = x W1^T (the llama MLP), the SwiGLU backward fused into
    the down-projection's data-gradient GEMM:

    forward   gu = x W1^T (hipBLASLt), a = swiglu(gu) (swiglu_fwd_kernel), y = a W2^T (hipBLASLt)
    backward  dW2 += dy^T a
              [dg | du] = swiglu'(gu, dy W2)   one gemm_tn launch (epilogue 5) through W2's
                                               transposed shadow: no swiglu_bwd pass over the
                                               [tokens, 2F] activations
              dx = [dg | du] W1, dW1 += [dg | du]^T x
    Same roundings as the unfused path (dy W2 rounded to bf16 before the SwiGLU backward).
    Reference MLP: /root/reference/src/models/mlp.py:24-26 (the llama preset's SwiGLU variant)."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        if FUSED_SWIGLU_FWD and _ops().gemm_uses_pp(C, 7):
            # the SwiGLU in the up-projection's epilogue (gemm_tn epilogue 7, ping-pong kernel):
            # no swiglu_fwd pass re-reading the [tokens, 2F] pre-activations
            a, gu = _ops().gemm_tn(x2, w1, None, 7)
        else:
            gu = F.linear(x2, w1)
            a = _ops().swiglu_fwd(gu)
        ctx.save_for_backward(x2, gu, a)
        ctx.params = (w1, w2)
        ctx.xshape = x.shape
        return F.linear(a, w2).view(*x.shape[:-1], C)

    @staticmethod
    def backward(ctx, dy):
        x2, gu, a = ctx.saved_tensors
        w1, w2 = ctx.params
        ctx.params = None
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        # (both weight gradients whatever needs_input_grad says, as in _FusedMLPFn)
        dw2, _ = _linear_param_grads(dy2, a, w2, None)
        dgu = _ops().gemm_tn(dy2, _shadow_or_t(w2), None, 5, gu, None)[0]
        dx = _dgrad(dgu, w1) if ctx.needs_input_grad[0] else None
        dw1, _ = _linear_param_grads(dgu, x2, w1, None)
        if dx is not None:
            dx = dx.view(ctx.xshape)
        return dx, dw1, dw2


def fused_swiglu_mlp(x, w1, w2):
    return _FusedSwiGLUMLPFn.apply(x, w1, w2)


_ACT_IDS = {None: 0, "gelu": 1, "relu": 2}


def _aligned16(t) -> bool:
    """16-byte alignment of a view, from its storage offset (allocations are 256-B aligned);
    unlike data_ptr() this is well-defined on FakeTensors (torch.compile tracing)."""
    return (t.storage_offset() * t.element_size()) % 16 == 0


def _gemv_shape_ok(x, weight) -> bool:
    """Decode-sized input (<= 8 token rows) on the HIP path whose weight the skinny GEMM (csrc/gemv.hip) takes."""
    K = x.shape[-1]
    rows = x.numel() // K if K else 0
    return _hip(x) and 0 < rows <= 8 and K % 8 == 0 and weight.is_contiguous() and _aligned16(weight)


def _gemv_ok(x, weight):
    # (the fused norm + GEMM of norm_linear has no backward at all: never under grad mode, see linear())
    return not torch.is_grad_enabled() and _gemv_shape_ok(x, weight)


def norm_linear(x, residual, norm_weight, norm_bias, eps: float, rms: bool, weight, bias=None,
                act: Optional[str] = None, kv=None):
    """Inference-only ``(act(norm(x + residual) @ weight^T + bias), x + residual)``.

    For decode-sized inputs (<= 8 token rows) on the HIP path this is ONE launch of the
    skinny-GEMM kernel with the norm as its prologue and the activation as its epilogue
    (csrc/gemv.hip): a decode block then runs no separate norm or activation kernels.
    Otherwise it is the unfused norm -> linear -> activation sequence.

    ``kv = (k_cache, v_cache, pos_t, q_cols)`` (decode QKV projection, caches [B, S_max, Hkv, D],
    ``pos_t`` int64 [1] on the device): output columns q_cols.. are also appended to the caches
    at position ``pos_t`` -- by the kernel's epilogue on the fused path.

    ``weight`` may be an ``Fp8Weight``: the fused launch is then ``gemv_fp8`` on its codes; where the fused path
    does not apply, the unfused sequence hands it to ``linear``, which reads the codes or ``ref`` by its own rule."""
    fw = weight if isinstance(weight, Fp8Weight) else None
    if fw is not None:  # the fused launch reads the codes; whatever else runs below decides in linear()
        weight = fw.ref
    fused_fp8 = fw is not None and _gemv_ok(x, fw.q) and norm_weight.dtype == x.dtype == weight.dtype
    if fused_fp8 or (_gemv_ok(x, weight) and norm_weight.dtype == x.dtype):
        K = x.shape[-1]
        rows = x.numel() // K
        x2 = x.reshape(rows, K).contiguous()
        r2 = residual.reshape(rows, K).contiguous() if residual is not None else None
        kc = vc = pos = None
        q_cols = 0
        if kv is not None:
            kc, vc, pos, q_cols = kv
        tail = (bias, r2, norm_weight, None if rms else norm_bias, eps, int(rms), _ACT_IDS[act], kc, vc, pos, q_cols)
        out = _ops().gemv_fp8(x2, fw.q, fw.scale, *tail) if fused_fp8 else _ops().gemv(x2, weight, *tail)
        y = out[0].view(*x.shape[:-1], weight.shape[0])
        s = out[1].view(x.shape) if residual is not None else x
        return y, s
    if rms:
        h, s = rms_norm(x, norm_weight, eps, residual)
    else:
        h, s = layer_norm(x, norm_weight, norm_bias, eps, residual)
    y = linear(h, fw if fw is not None else weight, bias)
    if act == "gelu":
        y = gelu(y)
    elif act == "relu":
        y = relu(y)
    if kv is not None:
        kc, vc, pos, q_cols = kv
        B, kvc = kc.shape[0], kc[0, 0].numel()
        y2 = y.reshape(B, -1)
        if pos.numel() > 1:  # one position per sequence (continuous batching)
            rows = torch.arange(B, device=pos.device)
            kc.index_put_((rows, pos), y2[:, q_cols:q_cols + kvc].reshape(B, *kc.shape[2:]))
            vc.index_put_((rows, pos), y2[:, q_cols + kvc:].reshape(B, *vc.shape[2:]))
        else:
            kc.index_copy_(1, pos, y2[:, q_cols:q_cols + kvc].reshape(B, 1, *kc.shape[2:]))
            vc.index_copy_(1, pos, y2[:, q_cols + kvc:].reshape(B, 1, *vc.shape[2:]))
    return y, s


# ---------------------------------------------------------------------------
# LayerNorm / RMSNorm with optional fused residual add
#   s = x + residual (if residual given);  y = norm(s) * w (+ b)
#   returns (y, s).  The backward adds the residual-stream gradient (ds from
#   the next layer) into dx in the same kernel.
# ---------------------------------------------------------------------------
class _NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, rms, x_bias):
        shp = x.shape
        C = shp[-1]
        x2 = x.reshape(-1, C)
        r2 = residual.reshape(-1, C) if residual is not None else None
        y, s, mean, rstd = _ops().norm_fwd(x2, r2, weight, bias, eps, rms)
        if residual is None:
            s = x2  # the op returns an empty s: the normalised stream is x itself
        ctx.save_for_backward(s, weight, mean, rstd)
        ctx.w, ctx.b, ctx.xb = weight, bias, x_bias
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        ctx.rms = rms
        ctx.shp = shp
        if residual is None:
            return y.view(shp), x  # s is x itself: hand the caller's tensor back
        return y.view(shp), s.view(shp)

    @staticmethod
    def backward(ctx, dy, ds):
        s, weight, mean, rstd = ctx.saved_tensors
        C = ctx.shp[-1]
        dy2 = dy.reshape(-1, C).contiguous()
        ds2 = ds.reshape(-1, C).contiguous() if ds is not None else None
        # (x_bias rides in the kernel only on its accumulating form: one group, all slots or none)
        tw, tb, txb = _take(ctx.w, ctx.b, ctx.xb)
        dw = db = dxb = None
        if tw is not None:
            outs = (_ops().norm_bwd_acc(dy2, s, weight, mean, rstd, ds2, ctx.has_bias, ctx.rms, tw, tb, txb),)
            _wrote(ctx.w, ctx.b, ctx.xb)
        else:
            outs = _ops().norm_bwd(dy2, s, weight, mean, rstd, ds2, ctx.has_bias, ctx.rms)
            dw, db = outs[1], (outs[2] if ctx.has_bias else None)
            if ctx.xb is not None:  # the column sums of dx as a pass of their own
                dxb = _bias_param_grad(outs[0], ctx.xb)
        ctx.w = ctx.b = ctx.xb = None
        dx = outs[0].view(ctx.shp)
        return dx, (dx if ctx.has_res else None), dw, db, None, None, dxb


def _norm_ref(x, residual, weight, bias, eps, rms):
    s = x if residual is None else x + residual
    if _stock("norm"):
        if rms:
            y = F.rms_norm(s, (s.shape[-1],), weight, eps)
        else:
            y = F.layer_norm(s, (s.shape[-1],), weight, bias, eps)
        return y, s
    if rms:
        y = ref.rms_norm(s, weight, eps)
    else:
        y = ref.layer_norm(s, weight, bias, eps)
    return y, s


def layer_norm(x, weight, bias, eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
               x_bias: Optional[torch.Tensor] = None):
    """(LayerNorm(x + residual), x + residual).  ``x_bias``: the bias of the linear layer that
    produced ``x`` (created with ``bias_grad_external=True``); its gradient is the column sum of
    dx and is produced by this norm's backward kernel (HIP path)."""
    if _hip_op("norm", x):
        return _NormFn.apply(x.contiguous(), residual.contiguous() if residual is not None else None,
                             weight, bias, eps, False, x_bias)
    return _norm_ref(x, residual, weight, bias, eps, False)


def rms_norm(x, weight, eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
             x_bias: Optional[torch.Tensor] = None):
    if _hip_op("norm", x):
        return _NormFn.apply(x.contiguous(), residual.contiguous() if residual is not None else None,
                             weight, None, eps, True, x_bias)
    return _norm_ref(x, residual, weight, None, eps, True)


# ---------------------------------------------------------------------------
# Flash attention on a packed QKV projection output.
#   qkv: [B, T, (H + 2*Hkv) * D]   ->  out [B, T, H*D]
# The HIP kernels read Q/K/V straight out of the packed GEMM output (strided
# views) and write dQ/dK/dV straight into a packed gradient buffer, so no
# split/cat copies exist on either side of the attention.
# ---------------------------------------------------------------------------
def _split_qkv(qkv, H, Hkv, D):
    B, T, _ = qkv.shape
    q = qkv[..., : H * D].view(B, T, H, D)
    k = qkv[..., H * D: (H + Hkv) * D].view(B, T, Hkv, D)
    v = qkv[..., (H + Hkv) * D:].view(B, T, Hkv, D)
    return q, k, v


def _qkv_heads(qkv, qk, H, Hkv, D):
    """q, k, v head views of the packed tensor; q / k from the rotated buffer ``qk`` when there is one."""
    B, T, _ = qkv.shape
    q, k, v = _split_qkv(qkv, H, Hkv, D)
    if qk is not None:
        q = qk[..., : H * D].view(B, T, H, D)
        k = qk[..., H * D:].view(B, T, Hkv, D)
    return q, k, v


def doc_bounds(idx, sep_token: int):
    """Per-row key bounds of a packed token window ``idx`` [B, T] whose documents end with ``sep_token``:
    (kv_start, q_last), int32 [B, T] each -- position i sees keys kv_start[b, i] <= j <= i, key j is seen by
    queries j <= i <= q_last[b, j].  A separator is the last token of the document it ends; the first document
    starts at 0 and the last ends at T - 1.  Fixed-shape device ops only (no sync, no data-dependent shape),
    so it can sit inside a captured step."""
    B, T = idx.shape
    pos = torch.arange(T, device=idx.device, dtype=torch.int32).expand(B, T)
    sep = idx == sep_token
    # a document starts right after a separator: position i starts one iff token i - 1 is a separator
    starts = torch.zeros_like(sep)
    starts[:, 1:] = sep[:, :-1]
    kv_start = torch.cummax(torch.where(starts, pos, torch.zeros_like(pos)), dim=1).values
    # it ends at the next separator at or after i (T - 1 without one): a reversed running minimum
    ends = torch.where(sep, pos, torch.full_like(pos, T - 1))
    q_last = -torch.cummax(-ends.flip(1), dim=1).values.flip(1)
    return kv_start.to(torch.int32).contiguous(), q_last.to(torch.int32).contiguous()


def bounds_from_start(kv_start):
    """q_last [B, T] int32 for any valid ``kv_start`` [B, T] (non-decreasing, 0 <= kv_start[i] <= i): the last
    query i with kv_start[i] <= j, i.e. searchsorted(kv_start[b], j, right=True) - 1."""
    B, T = kv_start.shape
    j = torch.arange(T, device=kv_start.device, dtype=kv_start.dtype).expand(B, T).contiguous()
    return (torch.searchsorted(kv_start.contiguous(), j, right=True) - 1).to(torch.int32)


def window_bounds(B: int, T: int, window: int, device, doc=None):
    """Per-row key bounds (kv_start, q_last), int32 [B, T] each, of a sliding window of ``window`` keys (the query
    included): kv_start[i] = max(0, i - window + 1), q_last[j] = min(T - 1, j + window - 1).  With ``doc`` (the
    bounds of ``doc_bounds``) the intersection of window and document: kv_start = max(doc_start, i - window + 1),
    q_last = min(doc_q_last, j + window - 1).  Closed form in fixed-shape device ops, so it can sit inside a
    captured step; nothing is kept between calls."""
    if window < 1:
        raise ValueError(f"window_bounds: window={window} must be >= 1")
    w = min(int(window), T) - 1
    pos = torch.arange(T, device=device, dtype=torch.int32).expand(B, T)
    kv_start = (pos - w).clamp_min(0)
    q_last = (pos + w).clamp_max(T - 1)
    if doc is not None:
        kv_start = torch.maximum(kv_start, doc[0].to(torch.int32))
        q_last = torch.minimum(q_last, doc[1].to(torch.int32))
    return kv_start.contiguous(), q_last.contiguous()


def _bounds_mask(kv_start):
    """Boolean visibility [B, 1, T, T] of the bounds (query i, key j): kv_start[b, i] <= j <= i."""
    T = kv_start.shape[1]
    j = torch.arange(T, device=kv_start.device)
    return ((j[None, None, :] >= kv_start[:, :, None]) & (j[None, None, :] <= j[None, :, None])).unsqueeze(1)


def _attn_packed_fwd(qkv, H, Hkv, causal, scale, cos, sin, qkn=None, kv_start=None, sinks=None):
    """Forward attention over packed qkv -> (qk, o, lse, rstd); ``qk`` is the q / k buffer of the
    pre-pass ([B, T, (H + Hkv) D], None without one), which the backward reads again: rotated (RoPE,
    rope_qk) or, with ``qkn`` = (wq, wk, eps) (QK-norm), normalised per head and then rotated when
    there are tables (qk_norm_rope, which also returns the heads' ``rstd``; else None).  ``sinks``: bf16 [H]
    attention sinks, folded into the forward kernel's epilogue (``lse`` then includes them)."""
    T = qkv.shape[1]
    D = qkv.shape[2] // (H + 2 * Hkv)
    rstd = None
    if qkn is not None:
        qk, rstd = _ops().qk_norm_rope(qkv, qkn[0], qkn[1], qkn[2], H, Hkv, cos, sin, T, 0)
    else:
        qk = _ops().rope_qk(qkv, cos, sin, H + 2 * Hkv, H + Hkv, T) if cos is not None else None
    q, k, v = _qkv_heads(qkv, qk, H, Hkv, D)
    o, lse = _ops().attn_fwd(q, k, v, causal, scale, kv_start, sinks)
    return qk, o, lse, rstd


def _qk_norm_bwd(dqkv, qkv, rstd, wq, wk, H, Hkv):
    """QK-norm backward in place on the q / k columns of ``dqkv`` -> (dwq, dwk): None when the gain
    gradients went straight into the flat-gradient slots, else fresh tensors."""
    (tq, tk), overwrite = _take(wq, wk, whole=True)
    out = _ops().qk_norm_bwd_(dqkv, qkv, rstd, wq, wk, H, Hkv, tq, tk, overwrite)
    if tq is None:
        return out
    _wrote(wq, wk)
    return None, None


def _sinks_kw(sinks) -> dict:
    """The reference's ``sinks`` argument, only when there are sinks (without them the call is the plain one)."""
    return {} if sinks is None else {"sinks": sinks}


def _sink_bwd(lse, delta, sinks):
    """Gradient of the attention sinks, ds[h] = -sum_{b,i} exp(s[h] - lse[b,h,i]) delta[b,h,i] (csrc/attn_sink.hip):
    None when it went straight into the flat-gradient slot (the whole gradient at once), else a fresh tensor."""
    (tgt,), overwrite = _take(sinks, whole=True)
    out = _ops().attn_sink_bwd(lse, delta, sinks, tgt, overwrite)
    if tgt is None:
        return out
    _wrote(sinks)
    return None


def _attn_packed_bwd(do, qkv, qk, o, lse, cfg, cos, sin, delta=None, qkn=None, rstd=None, kv_start=None, q_last=None,
                     sinks=None):
    """Backward attention -> packed dqkv (for the unrotated qkv: the kernels rotate dq / dk back).
    ``do``: [B, T, H, D] contiguous; ``delta``: rowsum(dO * O) when the caller already holds it.
    Returns (dqkv, dwq, dwk, dsinks): with ``qkn`` = (wq, wk, eps) one streaming post-pass takes the q / k
    columns back through the QK-norm and yields the gain gradients (see _qk_norm_bwd), else None.  With ``sinks``
    (``lse`` includes them) the backward kernels run as they are -- the sink has a zero value row, so
    delta = rowsum(dO O) already is the sum of P dP over keys and sink -- and the sink gradient is one
    reduction over lse and delta (see _sink_bwd), delta kept from the kernels' pre-pass when none came in."""
    H, Hkv, D, causal, scale = cfg
    q, k, v = _qkv_heads(qkv, qk, H, Hkv, D)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = _split_qkv(dqkv, H, Hkv, D)
    _attn_ws(qkv.device)
    if sinks is not None and delta is None:
        delta = torch.empty_like(lse)
        _ops().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, scale, cos, sin, None, kv_start, q_last, delta)
    else:
        _ops().attn_bwd(do, q, k, v, o, lse, dq, dk, dv, causal, scale, cos, sin, delta, kv_start, q_last)
    dwq = dwk = None
    if qkn is not None:
        dwq, dwk = _qk_norm_bwd(dqkv, qkv, rstd, qkn[0], qkn[1], H, Hkv)
    dsinks = _sink_bwd(lse, delta, sinks) if sinks is not None else None
    return dqkv, dwq, dwk, dsinks


class _FlashAttnPacked(torch.autograd.Function):
    """Attention over the packed QKV projection.  With ``cos``/``sin`` (RoPE) one pre-pass
    writes the rotated q and k heads to a [B, T, (H + Hkv) D] buffer that both the forward and
    the backward kernels read (kept for the backward: 2/3 of qkv for MHA); the backward kernels
    rotate dq / dk back while storing them, so the gradient comes back for the unrotated packed
    tensor.  (Rotating inside the kernels' tile loops instead measured +22 % forward / +25 %
    backward at the llama shape -- the round-2 RoPE A/B record under profiles/ -- and was removed.)"""

    @staticmethod
    def forward(ctx, qkv, H, Hkv, causal, scale, cos, sin, wq=None, wk=None, qk_eps=1e-5, kv_start=None, q_last=None,
                sinks=None):
        B, T, W = qkv.shape
        ctx.qkn = (wq, wk, qk_eps) if wq is not None else None  # QK-norm gains (the parameters themselves)
        ctx.sinks = sinks  # attention sinks (the parameter itself)
        qk, o, lse, rstd = _attn_packed_fwd(qkv, H, Hkv, causal, scale, cos, sin, ctx.qkn, kv_start, sinks)
        ctx.save_for_backward(qkv, qk, o, lse, cos, sin, rstd, kv_start, q_last)
        ctx.cfg = (H, Hkv, W // (H + 2 * Hkv), causal, scale)
        return o.view(B, T, -1)

    @staticmethod
    def backward(ctx, do):
        qkv, qk, o, lse, cos, sin, rstd, kv_start, q_last = ctx.saved_tensors
        dqkv, dwq, dwk, dsinks = _attn_packed_bwd(do.contiguous().view(o.shape), qkv, qk, o, lse, ctx.cfg, cos, sin,
                                                  qkn=ctx.qkn, rstd=rstd, kv_start=kv_start, q_last=q_last,
                                                  sinks=ctx.sinks)
        ctx.qkn = ctx.sinks = None
        return dqkv, None, None, None, None, None, None, dwq, dwk, None, None, None, dsinks


class _AttnProjFn(torch.autograd.Function):
    """``attention_packed`` followed by the output projection y = O W_o^T (+ b_o).  The backward runs
    the projection's data gradient through the fused-epilogue GEMM (csrc/gemm.hip epilogue 6), which
    also emits the attention backward's row constants delta = rowsum(dO * O) per (batch, head,
    query) while dO is in registers, so the attn_bwd_pre_kernel pass over dO and O is gone.  Head
    dim 64 (a wave's 64 output columns are one head).  Same math as _FlashAttnPacked + _LinearFn."""

    @staticmethod
    def forward(ctx, qkv, H, Hkv, causal, scale, cos, sin, w, b, bias_ext, res=None, wq=None, wk=None, qk_eps=1e-5,
                kv_start=None, q_last=None, sinks=None):
        B, T, W = qkv.shape
        D = W // (H + 2 * Hkv)
        ctx.qkn = (wq, wk, qk_eps) if wq is not None else None  # QK-norm gains (the parameters themselves)
        ctx.sinks = sinks  # attention sinks (the parameter itself)
        qk, o, lse, rstd = _attn_packed_fwd(qkv, H, Hkv, causal, scale, cos, sin, ctx.qkn, kv_start, sinks)
        ctx.save_for_backward(qkv, qk, o, lse, cos, sin, rstd, kv_start, q_last)
        ctx.cfg = (H, Hkv, D, causal, scale)
        ctx.w, ctx.b, ctx.bias_ext = w, b, bias_ext
        ctx.has_res = res is not None
        if res is not None:  # the block's residual stream added in the GEMM (resid_gemm_ok)
            C = w.shape[0]
            return _gemm_lt(o.view(B * T, H * D), w, b, 0, res.reshape(-1, C)).view(B, T, C)
        return F.linear(o.view(B, T, H * D), w, b)

    @staticmethod
    def backward(ctx, dy):
        qkv, qk, o, lse, cos, sin, rstd, kv_start, q_last = ctx.saved_tensors
        H, Hkv, D, causal, scale = ctx.cfg
        w, b, qkn, sinks = ctx.w, ctx.b, ctx.qkn, ctx.sinks
        ctx.w = ctx.b = ctx.qkn = ctx.sinks = None
        B, T, _ = qkv.shape
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        o2 = o.view(B * T, H * D)
        # projection weight / bias gradients (as _LinearFn.backward)
        dw, db = _linear_param_grads(dy2, o2, w, b, ctx.needs_input_grad[7],
                                     ctx.needs_input_grad[8] and not ctx.bias_ext)
        # dO and delta from one GEMM through W_o's transposed shadow
        do2, delta = _ops().gemm_tn(dy2, _shadow_or_t(w), None, 6, o2, None, T)
        dqkv, dwq, dwk, dsinks = _attn_packed_bwd(do2.view(B, T, H, D), qkv, qk, o, lse, ctx.cfg, cos, sin, delta,
                                                  qkn=qkn, rstd=rstd, kv_start=kv_start, q_last=q_last, sinks=sinks)
        return (dqkv, None, None, None, None, None, None, dw, db, None, (dy if ctx.has_res else None), dwq, dwk,
                None, None, None, dsinks)


# PLLM_AB attn_proj_fused=0: the output projection's backward on hipBLASLt + the attention's delta pre-pass
FUSED_ATTN_PROJ = _ab("attn_proj_fused", True)
# head dims served by it: 64.  (D = 128 -- two 64-column delta halves per head -- measured 0.5 % slower on
# llama-1.3B, profiles/r4_attn_experiments.md, and was removed: the D = 128 backward, csrc/attn_bwd_ks.hip,
# forms delta itself)
ATTN_PROJ_HEAD_DIMS = (64,)


def attn_proj_ok(qkv, n_head: int, n_kv_head: int, w, b) -> bool:
    """The fused attention + output projection path (_AttnProjFn): HIP training path, head dim 64."""
    if not FUSED_ATTN_PROJ or not torch.is_grad_enabled() or not (_hip_op("attn", qkv) and _hip_op("linear", qkv)):
        return False
    B, T, W = qkv.shape
    D = W // (n_head + 2 * n_kv_head)
    C_out = w.shape[0]
    return (D in ATTN_PROJ_HEAD_DIMS and B * T > 0 and tuple(w.shape) == (C_out, n_head * D) and C_out % 64 == 0
            and w.is_contiguous() and _aligned16(w) and (b is None or b.is_contiguous()))


def attention_proj(qkv, n_head: int, n_kv_head: int, w, b, causal: bool = True, scale: Optional[float] = None,
                   rope_cos=None, rope_sin=None, bias_grad_external: bool = False, residual=None,
                   q_norm_weight=None, k_norm_weight=None, qk_norm_eps: float = 1e-5, bounds=None, sinks=None):
    """``linear(attention_packed(qkv, ...), w, b)`` (+ ``residual``, added by the GEMM) with the fused
    backward (see _AttnProjFn).  ``bounds``, ``sinks``: see attention_packed."""
    D = qkv.shape[-1] // (n_head + 2 * n_kv_head)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    kv_start, q_last = bounds if bounds is not None else (None, None)
    if q_norm_weight is None:
        k_norm_weight = None
    else:  # the QK-norm pre- and post-pass take the packed tensor contiguous
        qkv = qkv.contiguous()
    return _AttnProjFn.apply(qkv, n_head, n_kv_head, causal, scale, rope_cos, rope_sin, w, b,
                             _bias_ext(bias_grad_external, b), residual, q_norm_weight, k_norm_weight, qk_norm_eps,
                             kv_start, q_last, sinks)


_ATTN_WS_MB = [None]


def _attn_ws(device):
    """Attention-backward dQ slab budget from the HBM still free (utils/memory.py: a quarter of
    it, capped at the 4 GiB that keeps every shipped config in one pass, floored at 64 MiB),
    quantised to 256 MiB steps so it is re-sent to the extension only when it moves;
    PLLM_ATTN_BWD_WS_MB fixes it instead."""
    if "PLLM_ATTN_BWD_WS_MB" in os.environ:
        return
    from ..utils import memory as _mem
    b = _mem.workspace_budget(device, _mem.ATTN_WS_CAP, _mem.ATTN_WS_FRACTION, _mem.ATTN_WS_FLOOR)
    mb = max(64.0, float(b // (256 * _mem.MiB) * 256))
    if mb != _ATTN_WS_MB[0]:
        _ops().attn_bwd_set_workspace_mb(mb)
        _ATTN_WS_MB[0] = mb


class _RopePackedFn(torch.autograd.Function):
    """Rotate the q and k heads of a packed qkv tensor (rotate-half convention)."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, H, Hkv):
        B, T, W = qkv.shape
        out = _ops().rope(qkv.contiguous(), cos, sin, H + 2 * Hkv, H + Hkv, T, 0, False)
        ctx.save_for_backward(cos, sin)
        ctx.cfg = (H, Hkv, T)
        return out

    @staticmethod
    def backward(ctx, dout):
        cos, sin = ctx.saved_tensors
        H, Hkv, T = ctx.cfg
        d = _ops().rope(dout.contiguous(), cos, sin, H + 2 * Hkv, H + Hkv, T, 0, True)
        return d, None, None, None, None


def rope_packed(qkv, cos, sin, n_head: int, n_kv_head: int):
    if _hip(qkv):
        return _RopePackedFn.apply(qkv, cos, sin, n_head, n_kv_head)
    B, T, W = qkv.shape
    D = W // (n_head + 2 * n_kv_head)
    q, k, v = _split_qkv(qkv, n_head, n_kv_head, D)
    q = ref.rope(q, cos[:T], sin[:T])
    k = ref.rope(k, cos[:T], sin[:T])
    return torch.cat([q.reshape(B, T, -1), k.reshape(B, T, -1), v.reshape(B, T, -1)], -1)


class _QKNormPackedFn(torch.autograd.Function):
    """QK-norm (+ RoPE) of the q and k heads of a packed qkv tensor -> [B, T, (H + Hkv) D]: the attention
    pre-pass on its own (csrc/qk_norm.hip), for decode and direct use."""

    @staticmethod
    def forward(ctx, qkv, wq, wk, eps, H, Hkv, cos, sin, pos_offset):
        qk, rstd = _ops().qk_norm_rope(qkv, wq, wk, eps, H, Hkv, cos, sin, qkv.shape[1], pos_offset)
        ctx.save_for_backward(qkv, rstd, cos, sin)
        ctx.wq, ctx.wk = wq, wk
        ctx.cfg = (H, Hkv, pos_offset)
        return qk

    @staticmethod
    def backward(ctx, dqk):
        qkv, rstd, cos, sin = ctx.saved_tensors
        H, Hkv, pos_offset = ctx.cfg
        wq, wk = ctx.wq, ctx.wk
        ctx.wq = ctx.wk = None
        d = dqk.contiguous()
        if cos is not None:  # back through the rotation
            d = _ops().rope(d, cos, sin, H + Hkv, H + Hkv, qkv.shape[1], pos_offset, True)
        dqkv = torch.zeros_like(qkv)  # v takes no part
        dqkv[..., : d.shape[-1]] = d
        dwq, dwk = _qk_norm_bwd(dqkv, qkv, rstd, wq, wk, H, Hkv)
        return dqkv, dwq, dwk, None, None, None, None, None, None


def qk_norm_packed(qkv, wq, wk, eps: float, n_head: int, n_kv_head: int, cos=None, sin=None, pos_offset: int = 0):
    """QK-norm of a packed qkv tensor [B, T, (H + 2 Hkv) D]: (q [B,T,H,D], k [B,T,Hkv,D]), each head RMS-normalised
    over D with the gains ``wq`` / ``wk`` [D] and then rotated when ``cos`` / ``sin`` are given (row t at position
    t + pos_offset).  Differentiable; the HIP kernels on the GPU, ``reference.qk_norm`` elsewhere."""
    B, T, W = qkv.shape
    H, Hkv = n_head, n_kv_head
    D = W // (H + 2 * Hkv)
    if _hip_op("attn", qkv):
        qk = _QKNormPackedFn.apply(qkv.contiguous(), wq, wk, eps, H, Hkv, cos, sin, pos_offset)
        return qk[..., : H * D].view(B, T, H, D), qk[..., H * D:].view(B, T, Hkv, D)
    q, k, _ = _split_qkv(qkv, H, Hkv, D)
    q, k = ref.qk_norm(q, wq, eps), ref.qk_norm(k, wk, eps)
    if cos is not None:
        c, s = cos[pos_offset:pos_offset + T], sin[pos_offset:pos_offset + T]
        q, k = ref.rope(q, c, s), ref.rope(k, c, s)
    return q, k


def attention_packed(qkv, n_head: int, n_kv_head: int, causal: bool = True, scale: Optional[float] = None,
                     rope_cos: Optional[torch.Tensor] = None, rope_sin: Optional[torch.Tensor] = None,
                     q_norm_weight=None, k_norm_weight=None, qk_norm_eps: float = 1e-5, bounds=None, sinks=None):
    """Causal self-attention over a packed qkv tensor. RoPE (if cos/sin given) is
    applied to the q and k heads first (rotate-half convention); with ``q_norm_weight`` /
    ``k_norm_weight`` (QK-norm) every q and k head is RMS-normalised over D before that.
    ``bounds`` = (kv_start, q_last) (int32 [B, T] each, from ``doc_bounds`` / ``bounds_from_start``; needs
    ``causal``): position i attends to keys kv_start[b, i] <= j <= i only (document / window masks).
    ``sinks`` [n_head] (attention sinks): one learned logit per query head that joins every row's softmax
    denominator -- unscaled, visible whatever the bounds -- and carries no value; differentiable."""
    B, T, W = qkv.shape
    D = W // (n_head + 2 * n_kv_head)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    kv_start, q_last = bounds if bounds is not None else (None, None)
    if bounds is not None and not causal:
        raise ValueError("attention bounds need causal attention")
    if _hip_op("attn", qkv):
        # RoPE: one rope_qk pre-pass rotates q / k, the backward kernels rotate dq / dk back
        if q_norm_weight is None:
            k_norm_weight = None
        else:  # QK-norm: qk_norm_rope is that pre-pass, qk_norm_bwd_ a post-pass over dqkv, both on contiguous qkv
            qkv = qkv.contiguous()
        return _FlashAttnPacked.apply(qkv, n_head, n_kv_head, causal, scale, rope_cos, rope_sin,
                                      q_norm_weight, k_norm_weight, qk_norm_eps, kv_start, q_last, sinks)
    if q_norm_weight is not None:
        q, k = qk_norm_packed(qkv, q_norm_weight, k_norm_weight, qk_norm_eps, n_head, n_kv_head, rope_cos, rope_sin)
        v = _split_qkv(qkv, n_head, n_kv_head, D)[2]
    else:
        if rope_cos is not None:
            qkv = rope_packed(qkv, rope_cos, rope_sin, n_head, n_kv_head)
        q, k, v = _split_qkv(qkv, n_head, n_kv_head, D)
    if _stock("attn") and qkv.is_cuda and sinks is None:  # (SDPA has no sink: those go through the reference)
        # stock-PyTorch baseline path (SDPA), used only by the explicit torch backend
        qh, kh, vh = (t.transpose(1, 2) for t in (q, k, v))
        if bounds is not None:  # the bounds as a boolean mask (it includes the causal triangle)
            o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=_bounds_mask(kv_start), scale=scale,
                                               enable_gqa=(n_kv_head != n_head))
        else:
            o = F.scaled_dot_product_attention(qh, kh, vh, is_causal=causal, scale=scale,
                                               enable_gqa=(n_kv_head != n_head))
        return o.transpose(1, 2).reshape(B, T, n_head * D)
    o, _ = ref.attention(q, k, v, causal=causal, scale=scale, bounds=bounds, **_sinks_kw(sinks))
    return o.reshape(B, T, n_head * D)


def attention(q, k, v, causal: bool = True, scale: Optional[float] = None, return_lse: bool = False,
              kv_start: Optional[torch.Tensor] = None, sinks: Optional[torch.Tensor] = None):
    """Unpacked attention q [B,T,H,D], k/v [B,S,Hkv,D] (forward only; used by the
    KV-cache decode and context-parallel paths).  Queries are aligned to the end
    of the key sequence.  ``kv_start`` (int32 [B, T], see ``window_bounds``; needs ``causal`` and S == T, a
    prefill from position 0): query i sees keys kv_start[b, i] <= j <= i only.  ``sinks`` [H]: attention sinks
    (see ``attention_packed``); the returned lse includes them."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if kv_start is not None:
        if not causal or k.shape[1] != q.shape[1]:
            raise ValueError(f"attention: kv_start needs causal attention over as many keys as queries "
                             f"(causal={causal}, T={q.shape[1]}, S={k.shape[1]})")
        if _hip(q):
            o, lse = _ops().attn_fwd(q, k, v, causal, scale, kv_start, sinks)
        else:
            o, lse = ref.attention(q, k, v, causal=True, scale=scale, bounds=(kv_start, None), **_sinks_kw(sinks))
        return (o, lse) if return_lse else o
    if _hip(q) and q.shape[1] == 1 and not return_lse and q.shape[2] // k.shape[2] in (1, 2, 4, 8):
        # one query per sequence (KV-cache decode): split-KV streaming kernel (csrc/attn_decode.hip)
        return _ops().attn_decode(q, k, v, scale, None, 0, sinks)
    if _hip(q):
        o, lse = _ops().attn_fwd(q, k, v, causal, scale, None, sinks)
    else:
        o, lse = ref.attention(q, k, v, causal=causal, scale=scale, **_sinks_kw(sinks))
    return (o, lse) if return_lse else o


def attention_decode(q, k, v, seqlen: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                     window: Optional[int] = None, sinks: Optional[torch.Tensor] = None):
    """Single-query attention q [B,1,H,D] over cached k/v [B,S,Hkv,D]; ``seqlen`` (int32 [1]
    device tensor) optionally limits the keys to the first ``seqlen`` rows, read on the
    device so a captured decode step (hipGraph) replays at every position.  ``window`` (sliding-window
    attention, a host constant): only the last ``window`` of those keys, [max(0, n - window), n), are seen.
    ``sinks`` [H]: attention sinks (see ``attention_packed``), in the denominator whatever the count or window."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if window is not None and window < 1:
        raise ValueError(f"attention_decode: window={window} must be >= 1 (None: no window)")
    if _hip(q):
        return _ops().attn_decode(q, k, v, scale, seqlen, int(window or 0), sinks)
    W = window if window is not None else k.shape[1]
    if seqlen is not None and seqlen.numel() > 1:  # one key count per sequence
        return torch.cat([ref.attention(q[b:b + 1], k[b:b + 1, max(0, int(n) - W):int(n)],
                                        v[b:b + 1, max(0, int(n) - W):int(n)], causal=False,
                                        scale=scale, **_sinks_kw(sinks))[0] for b, n in enumerate(seqlen.tolist())])
    n = int(seqlen.item()) if seqlen is not None else k.shape[1]
    k, v = k[:, max(0, n - W):n], v[:, max(0, n - W):n]
    o, _ = ref.attention(q, k, v, causal=False, scale=scale, **_sinks_kw(sinks))
    return o


def attention_block_bwd(do, q, k, v, o, lse, causal: bool = True, scale: Optional[float] = None):
    """Backward of one (query block, key block) attention product given the final output
    ``o`` and the log-sum-exp ``lse`` [B,H,T] of the WHOLE softmax row (context-parallel
    building block).  Returns (dq, dk, dv) in the dtype of q (HIP) or fp32 (CPU oracle)."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if _hip(q):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _attn_ws(q.device)
        _ops().attn_bwd(do, q, k, v, o, lse.contiguous(), dq, dk, dv, causal, scale)
        return dq, dk, dv
    return ref.attention_bwd(do, q, k, v, o, lse, causal=causal, scale=scale)


# ---------------------------------------------------------------------------
# activations (op ids of the HIP act kernels: 0 relu, 1 gelu-tanh)
# ---------------------------------------------------------------------------
class _ActFn(torch.autograd.Function):
    """GELU(tanh) (``kind`` 1) / ReLU (0, the reference MLP's activation); with ``bias`` (the producing linear's
    bias, created with bias_grad_external=True) the backward kernel also emits that bias's gradient."""

    @staticmethod
    def forward(ctx, x, bias, kind):
        y = _ops().act_fwd(x, kind)
        ctx.save_for_backward(x if kind == 1 else y)  # GELU's derivative needs its input, ReLU's only the sign of y
        ctx.b, ctx.kind = bias, kind
        return y

    @staticmethod
    def backward(ctx, dy):
        (t,) = ctx.saved_tensors
        dy = dy.contiguous()
        b, ctx.b = ctx.b, None
        if b is None:
            return _ops().act_bwd(dy, t, ctx.kind), None, None
        (tgt,) = _take(b)  # (not _bias_grad_by: without a slot it is another kernel pair, not fresh zeros)
        if tgt is not None:
            dx = _ops().act_bwd_bias(dy, t, ctx.kind, tgt)
            _wrote(b)
            return dx, None, None
        dx = _ops().act_bwd(dy, t, ctx.kind)
        return dx, _ops().bias_grad(dx), None


class _SwigluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        return _ops().swiglu_fwd(gu)

    @staticmethod
    def backward(ctx, dy):
        (gu,) = ctx.saved_tensors
        return _ops().swiglu_bwd(dy.contiguous(), gu)


def gelu(x, bias: Optional[torch.Tensor] = None):
    if _hip_op("act", x):
        return _ActFn.apply(x.contiguous(), bias, 1)
    if _stock("act"):
        return F.gelu(x, approximate="tanh")
    return ref.gelu_tanh(x)


def swiglu(gate_up):
    if _hip_op("act", gate_up):
        return _SwigluFn.apply(gate_up.contiguous())
    return ref.swiglu(gate_up)


def relu(x, bias: Optional[torch.Tensor] = None):
    if _hip_op("act", x):
        return _ActFn.apply(x.contiguous(), bias, 0)
    return ref.relu(x)


# ---------------------------------------------------------------------------
# Embedding (token + optional learned position), deterministic backward
# ---------------------------------------------------------------------------
class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, wte, wpe):
        x = _ops().embedding_fwd(idx, wte, wpe, 0)
        ctx.save_for_backward(idx)
        ctx.V = wte.shape[0]
        ctx.n_pos = 0 if wpe is None else wpe.shape[0]
        ctx.wte, ctx.wpe = wte, wpe
        return x

    @staticmethod
    def backward(ctx, dx):
        (idx,) = ctx.saved_tensors
        has_pos = ctx.n_pos > 0
        wte, wpe = ctx.wte, ctx.wpe
        ctx.wte = ctx.wpe = None
        tt, tp = _take(wte, wpe)
        if tt is not None:
            _ops().embedding_bwd_acc(dx.contiguous(), idx, ctx.V, ctx.n_pos, has_pos, tt, tp)
            _wrote(wte, wpe)
            return None, None, None
        outs = _ops().embedding_bwd(dx.contiguous(), idx, ctx.V, ctx.n_pos, has_pos)
        return None, outs[0], (outs[1] if has_pos else None)


def embedding(idx, wte, wpe=None, pos_offset: int = 0):
    if _hip_op("embed", wte):
        if pos_offset:
            return _ops().embedding_fwd(idx.contiguous(), wte, wpe, pos_offset)
        return _EmbeddingFn.apply(idx.contiguous(), wte, wpe)
    return ref.embedding(idx, wte, wpe, pos_offset)


# ---------------------------------------------------------------------------
# LM head + fused cross entropy, chunked over rows.
# The reference materialises [B*T, V] fp32 logits and a softmax (transformer.py:71-77:
# 3+ GiB at its own config).  Here the rows are processed in chunks of CE_CHUNK_ROWS:
# per chunk the LM-head GEMM writes bf16 logits into ONE reused [rows, V] workspace, the
# HIP CE kernel turns them in place into dlogits (never storing probabilities), and the
# two backward GEMMs (dh = dlogits W, dW += dlogits^T h) plus the head-bias column sums
# run right away on the same workspace while it is hot.  Nothing logits-sized outlives a
# chunk; the backward only scales the saved dh / fp32 dW / db by the upstream gradient.
# ---------------------------------------------------------------------------
# Chunk size: the fewest equal chunks (multiples of 64 rows) whose bf16 logits workspace fits
# CE_WORKSPACE_MB, or exactly CE_CHUNK_ROWS rows when that is set.  Measured on MI355X
# (GPT-2 small, 65,536 rows x 50,304, profiles/r2_ce_chunk_sweep.jsonl): 63.4 ms/step unchunked
# (29.9 GB peak) vs 64.5 / 65.3 / 70.6 / 73.8 ms at 16K / 8K / 4K / 2K rows (24.8-23.1 GB): the
# backward GEMMs lose efficiency at small M, so the default budget (8 GiB) keeps every shipped
# config in one chunk and only bounds the workspace when batch x vocab grows past it.  Also
# measured slower: sub-chunks of 1K / 2K / 4K rows for GEMM -> CE -> dgrad (logits kept in the
# Infinity Cache between them) with one weight-gradient GEMM over the whole dlogits afterwards:
# 75.7 / 68.5 / 66.6 ms vs 60.5 ms per step (scripts/gpu/r2_cesub.sh, profiles/r2_ce_subchunk_negative.txt).
# The workspace budget is a quarter of the HBM the device can still give (utils/memory.py),
# capped at those 8 GiB and floored at 256 MiB; PLLM_CE_WORKSPACE_MB fixes it instead.
CE_CHUNK_ROWS = _ab("ce_chunk_rows", 0)
CE_WORKSPACE_MB = float(os.environ["PLLM_CE_WORKSPACE_MB"]) if "PLLM_CE_WORKSPACE_MB" in os.environ else None


def _ce_budget_bytes(device) -> int:
    if CE_WORKSPACE_MB is not None:
        return int(CE_WORKSPACE_MB * 2 ** 20)
    from ..utils import memory as _mem
    return _mem.workspace_budget(device, _mem.CE_CAP, _mem.CE_FRACTION, _mem.CE_FLOOR)


def _ce_chunk_rows(N: int, V: int = 50304, budget_bytes: Optional[int] = None) -> int:
    if CE_CHUNK_ROWS > 0:
        r = max(64, CE_CHUNK_ROWS // 64 * 64)
        return N if N <= r else r
    per_row = 2 * V
    budget = budget_bytes if budget_bytes is not None else 8192 * 2 ** 20
    n_chunks = max(1, math.ceil(N * per_row / budget))
    if n_chunks == 1:
        return N
    return max(64, (math.ceil(N / n_chunks) + 63) // 64 * 64)


def _logits_into(ws, hc, weight, bias):
    """One chunk's logits hc W^T (+ bias) written into the head rows of the workspace ``ws``; returns those rows."""
    lg = ws[:hc.shape[0]]
    if bias is not None:
        torch.addmm(bias, hc, weight.t(), out=lg)
    else:
        torch.mm(hc, weight.t(), out=lg)
    return lg


def _ce_rows(lg, targets, dlogits, ignore_index, inv_n, z_loss, cap, lse):
    """Per-row losses of one block of logits: the plain kernel with both options off, else cross_entropy_aux
    (z term included; ``lse``: the rows of the log-sum-exp buffer to fill, or None)."""
    if not z_loss and not cap:
        return _ops().cross_entropy(lg, targets, dlogits, ignore_index, inv_n)
    return _ops().cross_entropy_aux(lg, targets, dlogits, ignore_index, inv_n, float(z_loss), float(cap or 0.0), lse)


def _z_term(lse, z_loss, inv_n, z_out):
    """z_loss * mean over the valid rows of lse^2 (ignored rows hold 0) into the 1-element ``z_out``."""
    if z_out is not None and lse is not None:
        z_out.copy_((lse.square().sum() * inv_n * z_loss).reshape(1))


def _scaled_param_grad(p, t, g, dtype, whole: bool = False):
    """g * t (``t``: the fp32 gradient the forward left) into ``p``'s slot (-> None, ``p`` notified; ``whole``: stored
    over a fresh slot), else returned as ``dtype``."""
    (tgt,), overwrite = _take(p, whole=True) if whole else (_take(p), False)
    if tgt is None:
        return t.mul_(g).to(dtype)
    if overwrite:
        torch.mul(t.view(-1), g, out=tgt.view(-1))
    else:
        tgt.view(-1).addcmul_(t.view(-1), g)
    _wrote(p)
    return None


class _LMHeadCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias, targets, ignore_index, z_loss=0.0, cap=None, z_out=None):
        N, C = h.shape
        V = weight.shape[0]
        n_valid = (targets != ignore_index).sum().clamp_min(1)
        inv_n = n_valid.to(torch.float32).reciprocal().reshape(1)
        need_h = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1]
        need_b = bias is not None and ctx.needs_input_grad[2]
        R = _ce_chunk_rows(N, V, _ce_budget_bytes(h.device))
        ws = torch.empty(R, V, dtype=h.dtype, device=h.device)
        dh = torch.empty_like(h) if need_h else None
        # the first chunk's weight gradient stores into dw (no zero fill, no read of zeros), later ones add.
        # When the weight's flat-gradient slot is untouched this step (lazy zeroing: the first writer
        # overwrites) the chunks write straight into that slot and the backward only scales it in place by
        # the upstream gradient -- a no-op launch when that is 1 -- instead of a 154 MB fp32 buffer copied and
        # scaled into the slot (GPT-2 small: ~55 us per step).  A slot already holding gradient (accumulation
        # micro-steps) keeps the separate buffer, and a taken one stays reserved until the backward (_reserve):
        # the scale applies to this call's part only.
        direct = _reserve(weight) if need_w else None
        dw = (direct.view(V, C) if direct is not None else
              torch.empty(V, C, dtype=torch.float32, device=h.device)) if need_w else None
        db = torch.zeros(V, dtype=torch.float32, device=h.device) if need_b else None
        rows = torch.empty(N, dtype=torch.float32, device=h.device)
        lse = torch.empty(N, dtype=torch.float32, device=h.device) if (z_loss or cap) else None
        wt = _shadow(weight)
        for r0 in range(0, N, R):
            r1 = min(N, r0 + R)
            hc = h[r0:r1]
            lg = _logits_into(ws, hc, weight, bias)
            rows[r0:r1] = _ce_rows(lg, targets[r0:r1], lg, ignore_index, inv_n, z_loss, cap,
                                   None if lse is None else lse[r0:r1])
            if need_h:  # dh = dlogits @ W (through the W^T shadow when present, see _dgrad)
                torch.mm(lg, wt.t() if wt is not None else weight, out=dh[r0:r1])
            if need_w:
                _weight_grad(lg, hc, dw, overwrite=r0 == 0)
            if need_b:
                _ops().bias_grad(lg, db)
        ctx.direct = direct is not None
        ctx.save_for_backward(dh, None if ctx.direct else dw, db)
        ctx.w, ctx.b = weight, bias
        ctx.wdtype = weight.dtype
        if z_loss:
            _z_term(lse, z_loss, inv_n[0], z_out)
        return rows.sum() * inv_n[0]

    @staticmethod
    def backward(ctx, dloss):
        dh, dw, db = ctx.saved_tensors
        g = dloss.to(torch.float32).reshape(())
        gh = None
        if dh is not None:
            if dh.is_cuda and dh.numel() % 8 == 0 and _lib.available():
                _ops().scale_(dh, g.reshape(1))  # (no pass when g == 1)
                gh = dh
            else:
                gh = dh.mul_(g.to(dh.dtype))
        gw = gb = None
        if ctx.direct:  # the weight gradient is already in its flat slot: scale it there (no-op when g == 1)
            _ops().scale_(_release(ctx.w).view(-1), g.reshape(1))
            _wrote(ctx.w)
        elif dw is not None:
            gw = _scaled_param_grad(ctx.w, dw, g, ctx.wdtype, whole=True)
        if db is not None:  # (the forward's column sums scaled by g, not a bias_grad pass: no _bias_param_grad)
            gb = _scaled_param_grad(ctx.b, db, g, ctx.wdtype)
        ctx.w = ctx.b = None
        return gh, gw, gb, None, None, None, None, None


def _check_ce_options(z_loss, softcap):
    if not z_loss >= 0:
        raise ValueError(f"z_loss={z_loss}: must be >= 0")
    if softcap is not None and not softcap > 0:
        raise ValueError(f"softcap={softcap}: must be > 0 (None: off)")


def softcap(logits, cap: Optional[float]):
    """Final-logit soft-capping ``cap * tanh(logits / cap)`` of a logits tensor that is handed out (``cap`` None:
    the tensor itself).  Plain elementwise torch ops of fixed shape, so it captures into the decode hipGraph; tanh is
    monotone, so greedy decoding does not change."""
    return ref.softcap(logits, cap)


def lm_head_cross_entropy(h, weight, bias, targets, ignore_index: int = -100, z_loss: float = 0.0,
                          softcap: Optional[float] = None, z_out=None):
    """mean CE of ``h @ weight^T + bias`` against ``targets`` without returning logits
    (chunked over rows on the HIP path: no [N, V] buffer in training or evaluation).
    ``softcap``: the logits pass through ``softcap * tanh(. / softcap)`` first; ``z_loss``: adds
    ``z_loss * logsumexp(logits)^2`` per token, both inside the CE kernel; ``z_out``: a 1-element fp32 tensor that
    receives the z term of the returned loss."""
    _check_ce_options(z_loss, softcap)
    targets = targets.reshape(-1)
    h = h.reshape(-1, h.shape[-1])
    if _hip_op("ce", h) and torch.is_grad_enabled() and (h.requires_grad or weight.requires_grad):
        if not z_loss and softcap is None:
            return _LMHeadCEFn.apply(h, weight, bias, targets, ignore_index)
        return _LMHeadCEFn.apply(h, weight, bias, targets, ignore_index, z_loss, softcap, z_out)
    if _hip_op("ce", h):
        N, V = h.shape[0], weight.shape[0]
        R = _ce_chunk_rows(N, V, _ce_budget_bytes(h.device))
        ws = torch.empty(R, V, dtype=h.dtype, device=h.device)
        rows = torch.empty(N, dtype=torch.float32, device=h.device)
        lse = torch.empty(N, dtype=torch.float32, device=h.device) if z_loss and z_out is not None else None
        for r0 in range(0, N, R):
            r1 = min(N, r0 + R)
            lg = _logits_into(ws, h[r0:r1], weight, bias)
            rows[r0:r1] = _ce_rows(lg, targets[r0:r1], None, ignore_index, None, z_loss, softcap,
                                   None if lse is None else lse[r0:r1])
        n_valid = (targets != ignore_index).sum().clamp_min(1)
        _z_term(lse, z_loss, n_valid.to(torch.float32).reciprocal(), z_out)
        return rows.sum() / n_valid
    logits = F.linear(h, weight, bias)
    return cross_entropy(logits, targets, ignore_index, z_loss, softcap, z_out)


def cross_entropy(logits, targets, ignore_index: int = -100, z_loss: float = 0.0, softcap: Optional[float] = None,
                  z_out=None):
    """Mean token cross-entropy over ``logits [N, V]`` (no in-place tricks); ``z_loss`` / ``softcap`` / ``z_out`` as
    in lm_head_cross_entropy."""
    _check_ce_options(z_loss, softcap)
    targets = targets.reshape(-1)
    if _hip(logits) and not (torch.is_grad_enabled() and logits.requires_grad):
        lse = torch.empty(targets.shape[0], dtype=torch.float32, device=logits.device) \
            if z_loss and z_out is not None else None
        rows = _ce_rows(logits.contiguous(), targets, None, ignore_index, None, z_loss, softcap, lse)
        n_valid = (targets != ignore_index).sum().clamp_min(1)
        _z_term(lse, z_loss, n_valid.to(torch.float32).reciprocal(), z_out)
        return rows.sum() / n_valid
    if not z_loss and softcap is None:
        return ref.cross_entropy(logits, targets, ignore_index)
    return ref.cross_entropy(logits, targets, ignore_index, z_loss, softcap, z_out)


# ---------------------------------------------------------------------------
# misc
# ---------------------------------------------------------------------------
def rope_cache(seq_len: int, head_dim: int, theta: float, device):
    cos, sin = ref.rope_cos_sin(seq_len, head_dim, theta, device=device)
    return cos.contiguous(), sin.contiguous()


def apply_rope(x, cos, sin, pos_offset: int = 0):
    """x [B,T,H,D] -> rotated copy (no autograd; used by decode). cos/sin index from pos_offset."""
    if _hip(x):
        B, T, H, D = x.shape
        y = _ops().rope(x.contiguous().view(B, T, H * D), cos, sin, H, H, T, pos_offset, False)
        return y.view(B, T, H, D)
    T = x.shape[1]
    return ref.rope(x, cos[pos_offset:pos_offset + T], sin[pos_offset:pos_offset + T])
