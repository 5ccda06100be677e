"""The flat-gradient helpers of ops (``_linear_param_grads``, ``_bias_param_grad``, ``_bias_grad_by``,
``_shadow`` / ``_shadow_or_t``) driven directly on the CPU: parameters dressed by hand the way FlatAdamW and the
data-parallel engine dress them, the two kernels behind them (``wgrad``, ``bias_grad``) replaced by torch
stand-ins that also record how they were called.  All values are small integers, so every sum is exact in bf16
and fp32 alike and the slots are compared with ``torch.equal``."""
import pytest
import torch
import torch.nn as nn

from pretraining_llm_amd import ops

N, K = 16, 24  # dy [rows, N], x [rows, K]


class _Kernels:
    """Stand-in for ``torch.ops.pllm``: the weight-gradient GEMM (optionally with the bias gradient riding on it)
    and the column-sum kernel, computed in fp32 by torch; ``calls`` records (kernel, took a fused bias target)."""

    def __init__(self):
        self.calls = []

    def wgrad(self, dy, x, out_acc=None, bias_acc=None, overwrite=False):
        self.calls.append(("wgrad", bias_acc is not None))
        dw = dy.t().float() @ x.float()
        if bias_acc is not None:
            bias_acc.add_(dy.float().sum(0).to(bias_acc.dtype))
        if out_acc is None:
            return dw.to(dy.dtype)
        out_acc.copy_(dw) if overwrite else out_acc.add_(dw.to(out_acc.dtype))
        return out_acc

    def bias_grad(self, dy, out_acc=None):
        self.calls.append(("bias_grad", False))
        assert dy.is_contiguous()
        s = dy.float().sum(0)
        if out_acc is None:
            return s.to(dy.dtype)
        out_acc.add_(s.to(out_acc.dtype))
        return out_acc


@pytest.fixture
def kernels(monkeypatch):
    k = _Kernels()
    monkeypatch.setattr(ops, "_ops", lambda: k)
    return k


def _ints(*shape, lo=-1, hi=2):
    return torch.randint(lo, hi, shape).to(torch.bfloat16)


def _param(shape, slot_dtype, fresh, log, name):
    """An nn.Parameter with (``slot_dtype`` given) a flat-gradient slot: NaN-filled when ``fresh`` (the optimizer
    left it uncleared: the first writer must overwrite), small integers otherwise; notifications go to ``log``."""
    p = nn.Parameter(_ints(*shape))
    p._pllm_grad_ready = lambda: log.append(name)
    if slot_dtype is None:
        return p, None
    old = torch.randint(-3, 4, shape).to(slot_dtype)
    p._pllm_flat_grad = True
    p._pllm_gradbuf = torch.full(shape, float("nan"), dtype=slot_dtype) if fresh else old.clone()
    p._pllm_grad_fresh = fresh
    return p, (torch.zeros_like(old) if fresh else old)


# rows 64: the shape the hand-written kernel takes (the stand-in's wgrad); 48: the torch arm of ops._weight_grad
@pytest.mark.parametrize("rows", [64, 48])
@pytest.mark.parametrize("w_slot,w_fresh", [(torch.float32, True), (torch.float32, False), (torch.bfloat16, True),
                                            (torch.bfloat16, False), (None, False)])
@pytest.mark.parametrize("bias", ["none", "slot", "noslot", "unneeded"])
@pytest.mark.parametrize("fuse_bias", [True, False])
def test_linear_param_grads(kernels, rows, w_slot, w_fresh, bias, fuse_bias):
    torch.manual_seed(rows + 7 * (bias == "slot") + fuse_bias)
    log = []
    dy, x = _ints(rows, N), _ints(rows, K)
    w, w_old = _param((N, K), w_slot, w_fresh, log, "w")
    b, b_old = (None, None) if bias == "none" else _param((N,), w_slot if bias in ("slot", "unneeded") else None,
                                                          False, log, "b")
    if w_slot is None and bias in ("slot", "unneeded"):  # a bias slot without a weight slot
        b, b_old = _param((N,), torch.float32, False, log, "b")
    dw_ref = dy.t().float() @ x.float()
    db_ref = dy.float().sum(0)

    dw, db = ops._linear_param_grads(dy, x, w, b, True, bias != "unneeded", fuse_bias)

    if w_slot is None:
        assert torch.equal(dw.float(), dw_ref) and not hasattr(w, "_pllm_gradbuf")
    else:  # overwritten over the NaNs when fresh, added onto the old contents otherwise
        assert dw is None
        assert torch.equal(w._pllm_gradbuf.float(), w_old.float() + dw_ref)
        assert w._pllm_grad_fresh is False
    b_written = bias in ("slot",)
    if bias in ("slot", "unneeded"):
        assert torch.equal(b._pllm_gradbuf.float(), b_old.float() + (db_ref if b_written else 0))
    if bias == "noslot":
        assert torch.equal(db.float(), db_ref)
    else:
        assert db is None
    assert log == (["w"] if w_slot is not None else []) + (["b"] if b_written else [])  # weight before bias
    # the bias gradient rides on the weight-gradient GEMM only with fuse_bias and both slots
    fused = fuse_bias and b_written and w_slot is not None
    if rows == 64:
        assert ("wgrad", fused) in kernels.calls and ("wgrad", not fused) not in kernels.calls
    assert kernels.calls.count(("bias_grad", False)) == int(bias in ("slot", "noslot") and not (fused and rows == 64))


def test_linear_param_grads_weight_not_needed(kernels):
    """needs_input_grad[1] False: the weight's slot stays untouched and fresh, the bias takes its own pass."""
    log = []
    dy, x = _ints(64, N), _ints(64, K)
    w, _ = _param((N, K), torch.float32, True, log, "w")
    b, b_old = _param((N,), torch.float32, False, log, "b")
    dw, db = ops._linear_param_grads(dy, x, w, b, False, True)
    assert dw is None and db is None and log == ["b"]
    assert w._pllm_grad_fresh is True and torch.isnan(w._pllm_gradbuf).all()
    assert torch.equal(b._pllm_gradbuf, b_old + dy.float().sum(0))
    assert kernels.calls == [("bias_grad", False)]


def test_fused_bias_switch_off(kernels, monkeypatch):
    """FUSED_WGRAD_BIAS off: the same slots and notifications through the separate pass."""
    monkeypatch.setattr(ops, "FUSED_WGRAD_BIAS", False)
    log = []
    dy, x = _ints(64, N), _ints(64, K)
    w, _ = _param((N, K), torch.float32, True, log, "w")
    b, b_old = _param((N,), torch.float32, False, log, "b")
    assert ops._linear_param_grads(dy, x, w, b) == (None, None)
    assert log == ["w", "b"] and kernels.calls == [("wgrad", False), ("bias_grad", False)]
    assert torch.equal(w._pllm_gradbuf, dy.t().float() @ x.float())
    assert torch.equal(b._pllm_gradbuf, b_old + dy.float().sum(0))


@pytest.mark.parametrize("slot,fresh", [(torch.float32, False), (torch.float32, True), (torch.bfloat16, False),
                                        (None, False)])
def test_bias_writers(kernels, slot, fresh):
    """The adding bias writers: ``_bias_param_grad`` (a bias_grad pass) and ``_bias_grad_by`` (a kernel that adds
    the sums beside its own work).  A fresh slot is zeroed before it is added into."""
    for helper in ("param", "by"):
        log = []
        dy = _ints(48, N)
        b, b_old = _param((N,), slot, fresh, log, "b")
        if helper == "param":
            out, db = "ran", ops._bias_param_grad(dy.t().contiguous().t(), b)  # a strided dy is made contiguous
        else:
            out, db = ops._bias_grad_by(b, lambda acc: (acc.add_(dy.float().sum(0).to(acc.dtype)), "ran")[1])
        assert out == "ran"
        if slot is None:
            assert torch.equal(db.float(), dy.float().sum(0)) and db.dtype == b.dtype and log == []
        else:
            assert db is None and log == ["b"] and b._pllm_grad_fresh is False
            assert torch.equal(b._pllm_gradbuf.float(), b_old.float() + dy.float().sum(0))


def test_shadow_lookup():
    w = nn.Parameter(_ints(N, K))
    assert ops._shadow(w) is None  # no shadow at all
    assert torch.equal(ops._shadow_or_t(w), w.t()) and ops._shadow_or_t(w).is_contiguous()
    w._pllm_wT = w.detach().t().contiguous()
    w._pllm_wT_ver = w._version
    assert ops._shadow(w) is w._pllm_wT and ops._shadow_or_t(w) is w._pllm_wT
    dy = _ints(8, N)
    assert torch.equal(ops._dgrad(dy, w), dy @ w)
    with torch.no_grad():
        w.add_(1)  # the weight moved on (an optimizer step before refresh_shadows): the shadow is stale
    assert w._pllm_wT_ver != w._version
    assert ops._shadow(w) is None
    wt = ops._shadow_or_t(w)
    assert wt is not w._pllm_wT and wt.is_contiguous() and torch.equal(wt, w.t())
    assert torch.equal(ops._dgrad(dy, w), dy @ w)  # through the weight itself, not the stale shadow
