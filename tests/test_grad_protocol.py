"""The flat-gradient helpers of ops (the slot protocol itself: ``_take`` / ``_wrote`` / ``_reserve`` / ``_release``;
``_linear_param_grads``, ``_bias_param_grad``, ``_bias_grad_by``, ``_qk_norm_bwd``, ``_sink_bwd``; ``_shadow`` /
``_shadow_or_t``) driven directly on the CPU: parameters dressed by hand the way FlatAdamW and the data-parallel
engine dress them, the kernels behind them (``wgrad``, ``bias_grad``, ``qk_norm_bwd_``, ``attn_sink_bwd``) replaced
by torch stand-ins that also record how they were called.  All values are small integers, so every sum is exact in
bf16 and fp32 alike and the slots are compared with ``torch.equal``."""
import itertools

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

    # the two whole-gradient reductions of the attention path.  Stand-in math: the q / k gain gradients are the column
    # sums of the two halves of dqkv, the sink gradient is minus the column sums of delta
    def qk_norm_bwd_(self, dqkv, qkv, rstd, wq, wk, H, Hkv, acc_q, acc_k, overwrite):
        self.calls.append(("qk_norm_bwd_", overwrite))
        assert (acc_q is None) == (acc_k is None)
        D = wq.shape[0]
        gq, gk = dqkv[:, :D].float().sum(0), dqkv[:, D:].float().sum(0)
        if acc_q is None:
            assert overwrite is False
            return gq.to(wq.dtype), gk.to(wk.dtype)
        for acc, g in ((acc_q, gq), (acc_k, gk)):
            acc.copy_(g) if overwrite else acc.add_(g.to(acc.dtype))
        return acc_q, acc_k

    def attn_sink_bwd(self, lse, delta, sinks, acc, overwrite):
        self.calls.append(("attn_sink_bwd", overwrite))
        g = -delta.float().sum(0)
        if acc is None:
            assert overwrite is False
            return g.to(sinks.dtype)
        acc.copy_(g) if overwrite else acc.add_(g.to(acc.dtype))
        return acc


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


def _same(a, b):
    """Bitwise-equal contents, NaNs included."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


# a group member: no such parameter (None entry), a parameter without a slot, or (slot dtype, fresh)
_MEMBERS = ["absent", "noslot", (torch.float32, True), (torch.float32, False), (torch.bfloat16, True),
            (torch.bfloat16, False)]


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("size", [1, 2, 3])
def test_take_groups(size, whole):
    """``_take`` over every group of ``size`` members: all slots or none, and on "none" nothing is touched -- not a
    flag, not a buffer (the fresh ones keep their NaNs).  An adding group zeroes exactly its fresh members; a
    ``whole`` group overwrites only when every member is fresh, else it zeroes the fresh ones.  Nobody is notified."""
    torch.manual_seed(size)
    for kinds in itertools.product(_MEMBERS, repeat=size):
        log, params, olds = [], [], []
        for i, kind in enumerate(kinds):
            p, old = (None, None) if kind == "absent" else _param((N,), *((None, False) if kind == "noslot" else kind),
                                                                  log, str(i))
            params.append(p)
            olds.append(old)
        before = [None if getattr(p, "_pllm_gradbuf", None) is None else p._pllm_gradbuf.clone() for p in params]
        out = ops._take(*params, whole=whole)
        slots, overwrite = out if whole else (out, False)
        assert isinstance(slots, tuple) and len(slots) == size and log == []
        present = [k for k in kinds if k != "absent"]
        if not present or "noslot" in present:  # incomplete: no slots, everything as it was found
            assert slots == (None,) * size and overwrite is False
            for p, kind, b in zip(params, kinds, before):
                if b is not None:
                    assert p._pllm_grad_fresh is kind[1] and _same(p._pllm_gradbuf, b)
            continue
        assert overwrite is (whole and all(k[1] for k in present))
        for p, kind, slot, b, old in zip(params, kinds, slots, before, olds):
            if p is None:
                assert slot is None
                continue
            assert slot is p._pllm_gradbuf and p._pllm_grad_fresh is False
            if kind[1] and overwrite:  # left for the kernel to store over
                assert _same(slot, b)
            else:  # a fresh slot zeroed, a written one kept
                assert torch.equal(slot, old)


def test_wrote_order():
    log = []
    a, b = _param((N,), torch.float32, False, log, "a")[0], _param((N,), None, False, log, "b")[0]
    ops._wrote(a, None, b, a)
    assert log == ["a", "b", "a"]
    ops._wrote(nn.Parameter(_ints(N)), None)  # nobody listens


def test_reservation():
    """A reserved slot (the LM head between its forward and its backward) is no slot to anyone else, alone or in
    a group, and nothing of the group is touched; releasing gives it back as a written slot."""
    log = []
    p, _ = _param((N, K), torch.float32, True, log, "p")
    q, _ = _param((N,), torch.float32, True, log, "q")
    buf = ops._reserve(p)
    assert buf is p._pllm_gradbuf and p._pllm_grad_fresh is False and torch.isnan(buf).all()  # its to store over
    assert ops._reserve(p) is None
    assert ops._take(p) == (None,) and ops._take(p, whole=True) == ((None,), False)
    assert ops._take(q, p) == (None, None) and ops._take(None, p, q, whole=True) == ((None, None, None), False)
    assert q._pllm_grad_fresh is True and torch.isnan(q._pllm_gradbuf).all()
    assert p._pllm_grad_fresh is False and torch.isnan(buf).all() and log == []
    buf.fill_(2.0)  # the reserving writer's part
    assert ops._release(p) is buf
    (got,), overwrite = ops._take(p, whole=True)
    assert got is buf and overwrite is False and torch.equal(buf, torch.full((N, K), 2.0))
    (gq, gp) = ops._take(q, p)
    assert gq is q._pllm_gradbuf and gp is buf and torch.equal(gq, torch.zeros(N)) and q._pllm_grad_fresh is False
    # only a fresh fp32 slot can be reserved; a refusal touches nothing
    for dtype, fresh in [(torch.float32, False), (torch.bfloat16, True), (None, False)]:
        r, _ = _param((N, K), dtype, fresh, log, "r")
        b0 = None if dtype is None else r._pllm_gradbuf.clone()
        assert ops._reserve(r) is None
        if dtype is not None:
            assert r._pllm_grad_fresh is fresh and _same(r._pllm_gradbuf, b0)
            assert ops._take(r)[0] is r._pllm_gradbuf  # and it is still there to take


_QK_CASES = [((torch.float32, True), (torch.float32, True)), ((torch.float32, True), (torch.float32, False)),
             ((torch.float32, False), (torch.float32, True)), ((torch.float32, False), (torch.float32, False)),
             ((torch.bfloat16, True), (torch.bfloat16, False)), ((None, False), (None, False)),
             ((torch.float32, True), (None, False)), ((None, False), (torch.float32, True))]


@pytest.mark.parametrize("q_kind,k_kind", _QK_CASES)
def test_qk_norm_bwd_slots(kernels, q_kind, k_kind):
    """The two gain gradients go into their slots together or come back together: stored when both slots are
    fresh, added otherwise (a fresh one zeroed first), ``wq`` notified before ``wk``; with a slot missing both
    come back as tensors, nobody is notified and the other slot stays as it was found, flag included."""
    torch.manual_seed(3)
    log, D = [], 8
    dqkv = _ints(32, 2 * D)
    wq, q_old = _param((D,), *q_kind, log, "wq")
    wk, k_old = _param((D,), *k_kind, log, "wk")
    before = [None if old is None else p._pllm_gradbuf.clone() for p, old in ((wq, q_old), (wk, k_old))]
    gq, gk = dqkv[:, :D].float().sum(0), dqkv[:, D:].float().sum(0)
    dwq, dwk = ops._qk_norm_bwd(dqkv, dqkv, None, wq, wk, 1, 1)
    if q_old is None or k_old is None:
        assert torch.equal(dwq.float(), gq) and torch.equal(dwk.float(), gk) and log == []
        assert kernels.calls == [("qk_norm_bwd_", False)]
        for p, kind, b in ((wq, q_kind, before[0]), (wk, k_kind, before[1])):
            if b is not None:
                assert p._pllm_grad_fresh is kind[1] and _same(p._pllm_gradbuf, b)
        return
    assert dwq is None and dwk is None and log == ["wq", "wk"]
    assert kernels.calls == [("qk_norm_bwd_", q_kind[1] and k_kind[1])]
    assert wq._pllm_grad_fresh is False and wk._pllm_grad_fresh is False
    assert torch.equal(wq._pllm_gradbuf.float(), q_old.float() + gq)
    assert torch.equal(wk._pllm_gradbuf.float(), k_old.float() + gk)


@pytest.mark.parametrize("slot,fresh", [(torch.float32, True), (torch.float32, False), (torch.bfloat16, False),
                                        (None, False)])
def test_sink_bwd_slot(kernels, slot, fresh):
    torch.manual_seed(4)
    log, H = [], 4
    delta = _ints(32, H)
    s, old = _param((H,), slot, fresh, log, "sinks")
    ds = ops._sink_bwd(None, delta, s)
    g = -delta.float().sum(0)
    assert kernels.calls == [("attn_sink_bwd", fresh)]
    if slot is None:
        assert torch.equal(ds.float(), g) and log == []
    else:
        assert ds is None and log == ["sinks"] and s._pllm_grad_fresh is False
        assert torch.equal(s._pllm_gradbuf.float(), old.float() + g)


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
