"""The deferred weight-gradient queue of ``ops`` (``_WgradQueue``) with its three calls into the extension
replaced by stand-ins that record the call and do the same arithmetic in torch on the CPU: when rounds are
launched, what is carried over, the order in which parameters are told, the flush at the end of a backward
(autograd engine callback), the safety-net flushes, and when deferral is off."""
import pytest
import torch

from pretraining_llm_amd import ops

T = ops.WGRAD_TILE


def plan_rule(tiles, tiles_q, done0, ctas, group_max=ops.WGRAD_GROUP_MAX):
    """csrc/gemm_plan.h wgrad_group_plan, restated: whole rounds of ``ctas`` tiles from the head of the queue,
    a cut inside a problem moved down to its last row-band boundary, at most ``group_max`` problems."""
    total = sum(tiles) - done0
    if total < ctas:
        return 0
    want, take = total // ctas * ctas, 0
    for i, (n, q) in enumerate(zip(tiles, tiles_q)):
        if i >= group_max or take >= want:
            break
        have = n - (done0 if i == 0 else 0)
        if take + have <= want:
            take += have
        else:
            take += (want - take) // q * q
            break
    return take


class RecQueue(ops._WgradQueue):
    def __init__(self, ctas):
        super().__init__()
        self.ctas, self.log = ctas, []

    def plan(self, tiles, tiles_q, done0):
        return [plan_rule(tiles, tiles_q, done0, self.ctas), 0]

    def run_group(self, items, first, last):
        self.log.append(("group", [it[5][0].tag for it in items], first, last))
        t0 = 0
        for dy, x, out, b, ow, _ in items:
            tq = -(-out.shape[1] // T)
            n = -(-out.shape[0] // T) * tq
            for t in range(max(first, t0), min(last, t0 + n)):
                r, c = (t - t0) // tq * T, (t - t0) % tq * T
                v = dy[:, r:r + T].float().t() @ x[:, c:c + T].float()
                out[r:r + T, c:c + T] = v if ow else out[r:r + T, c:c + T] + v
                if b is not None and c == 0:
                    b[r:r + T] += dy[:, r:r + T].float().sum(0)
            t0 += n

    def run_single(self, dy, x, out, b, ow):
        self.log.append(("single", tuple(out.shape)))
        v = dy.float().t() @ x.float()
        out.copy_(v if ow else out + v)
        if b is not None:
            b += dy.float().sum(0)


class P:
    """A parameter stand-in: a named slot whose notification goes into the queue's log."""

    def __init__(self, name, log, n):
        self.tag = name
        self.buf = torch.zeros(n)
        self._pllm_grad_ready = lambda: log.append(("told", name))


def problem(q, name, M, Pd, Qd, bias=False, overwrite=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(M, Pd, generator=g).bfloat16()
    x = torch.randn(M, Qd, generator=g).bfloat16()
    w, b = P(name, q.log, Pd * Qd), (P(name + ".b", q.log, Pd) if bias else None)
    if not overwrite:
        w.buf.fill_(1.0)
    q.armed = True  # as inside a backward whose end-of-backward flush is registered
    q.push(dy, x, w.buf.view(Pd, Qd), None if b is None else b.buf, overwrite, (w, b))
    ref = dy.float().t() @ x.float() + (0.0 if overwrite else 1.0)
    return w, b, ref, dy.float().sum(0)


def launches(q):
    return [e for e in q.log if e[0] != "told"]


def test_threshold_leftover_and_order():
    q = RecQueue(ctas=8)
    a = problem(q, "a", 128, 256, 256)                 # 1 tile
    b = problem(q, "b", 128, 264, 72, seed=1)          # 2 tiles, 1 per row band
    c = problem(q, "c", 128, 8, 520, seed=2)           # 3 tiles, one band of 3
    assert q.log == [] and len(q.items) == 3           # 6 tiles < 8: nothing launched, nobody told
    d = problem(q, "d", 128, 768, 256, bias=True, overwrite=False, seed=3)  # 3 tiles, 1 per band -> 9 >= 8
    # one round of 8: a, b, c whole and d's first two row bands; d stays queued with 2 tiles done, not told
    assert q.log == [("group", ["a", "b", "c", "d"], 0, 8), ("told", "a"), ("told", "b"), ("told", "c")]
    assert q.done0 == 2 and [it[5][0].tag for it in q.items] == ["d"]
    e = problem(q, "e", 128, 8, 2056, seed=4)          # 9 tiles in one band: 1 + 9 = 10 >= 8, but the cut
    # 8 falls inside e's only band -> down to the band boundary: d's last tile alone
    assert q.log[4:] == [("group", ["d"], 2, 3), ("told", "d"), ("told", "d.b")]
    assert q.done0 == 0 and [it[5][0].tag for it in q.items] == ["e"]
    q.flush()                                          # 9 >= 8, cut at 8 -> band boundary 0: e runs sliced
    assert q.log[7:] == [("single", (8, 2056)), ("told", "e")]
    assert not q.items and not q.armed
    for w, bb, ref, bref in (a, b, c, d, e):
        torch.testing.assert_close(w.buf.view_as(ref), ref, rtol=0, atol=0)
        assert not getattr(w, "_pllm_wgrad_queued", True)
        if bb is not None:
            torch.testing.assert_close(bb.buf, bref, rtol=0, atol=0)


def test_cut_problem_finishes_as_row_bands():
    """A problem cut by the last whole round: its remaining row bands go to the single-problem call as a
    [rows, Q] problem with the matching slices of dy, the slot and the bias slot."""
    q = RecQueue(ctas=4)
    a = problem(q, "a", 128, 768, 520, bias=True)      # 3 bands of 3 tiles: cut 8 -> 6 = two bands
    assert launches(q) == [("group", ["a"], 0, 6)] and q.done0 == 6 and ("told", "a") not in q.log
    q.flush()
    assert q.log == [("group", ["a"], 0, 6), ("single", (256, 520)), ("told", "a"), ("told", "a.b")]
    torch.testing.assert_close(a[0].buf.view_as(a[2]), a[2], rtol=0, atol=0)
    torch.testing.assert_close(a[1].buf, a[3], rtol=0, atol=0)


def test_one_launch_covers_several_rounds_and_group_max():
    q = RecQueue(ctas=2)
    q.ctas = 10 ** 6
    ps = [problem(q, f"p{i}", 128, 256, 256, seed=i) for i in range(ops.WGRAD_GROUP_MAX + 3)]
    q.ctas = 2
    q.flush()  # 19 tiles, rounds of 2: 16 problems per launch at the most, the odd one out runs alone
    assert launches(q) == [("group", [f"p{i}" for i in range(16)], 0, 16), ("group", ["p16", "p17"], 0, 2),
                           ("single", (256, 256))]
    assert [e[1] for e in q.log if e[0] == "told"] == [f"p{i}" for i in range(19)]
    for w, _, ref, _ in ps:
        torch.testing.assert_close(w.buf.view_as(ref), ref, rtol=0, atol=0)


class _Lin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x)
        ctx.w = w
        return x @ w.t()

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        (tgt,), fresh = ops._take(ctx.w, whole=True)
        ops._weight_grad(dy.bfloat16(), x.bfloat16(), tgt, None, overwrite=fresh, notify=(ctx.w, None))
        return dy @ ctx.w, None


def _slotted(n, log, name="w"):
    w = torch.nn.Parameter(torch.randn(n, n) * 0.1)
    w.tag = name
    w._pllm_flat_grad, w._pllm_gradbuf, w._pllm_grad_fresh = True, torch.zeros(n * n), True
    w._pllm_grad_ready = lambda: log.append(("told", w.tag))
    return w


@pytest.fixture
def rec(monkeypatch):
    q = RecQueue(ctas=4)
    monkeypatch.setattr(ops, "_WGRAD_QUEUE", q)
    monkeypatch.setattr(ops, "_wgrad_defer_on", lambda dy2: True)
    monkeypatch.setattr(ops, "_wgrad_sliced", lambda dy2, x2, btgt: True)
    return q


def test_flush_at_end_of_backward(rec):
    ws = [_slotted(256, rec.log, f"w{i}") for i in range(3)]
    x = torch.randn(128, 256, requires_grad=True)
    h = x
    for w in ws:
        h = _Lin.apply(h, w)
    h.sum().backward(inputs=[x])
    # 3 tiles < 4: nothing ran inside the backward; the engine's callback flushed them one by one, in the
    # backward's order, and the queue is disarmed for the next backward
    assert launches(rec) == [("single", (256, 256))] * 3
    assert [e[1] for e in rec.log if e[0] == "told"] == [w.tag for w in reversed(ws)]
    assert not rec.items and not rec.armed
    assert all(not w._pllm_grad_fresh and not w._pllm_wgrad_queued for w in ws)
    assert all(float(w._pllm_gradbuf.abs().sum()) > 0 for w in ws)
    first = [w._pllm_gradbuf.clone() for w in ws]
    h = x
    for w in ws:
        h = _Lin.apply(h, w)
    h.sum().backward(inputs=[x])  # no zero_grad in between: the second backward adds
    for w, f in zip(ws, first):
        torch.testing.assert_close(w._pllm_gradbuf, 2 * f, rtol=1e-6, atol=1e-6)


def test_outside_a_backward_nothing_is_queued(rec):
    w = _slotted(256, rec.log)
    dy, x = torch.randn(128, 256).bfloat16(), torch.randn(128, 256).bfloat16()
    assert rec.push(dy, x, w._pllm_gradbuf.view(256, 256), None, True, (w, None)) is False
    assert not rec.items and not getattr(w, "_pllm_wgrad_queued", False)


def test_safety_net_flushes(rec):
    w = _slotted(256, rec.log)
    w._pllm_grad_fresh = False  # (as after the _take of the queued write)
    dy, x = torch.randn(128, 256).bfloat16(), torch.randn(128, 256).bfloat16()
    rec.armed = True
    assert rec.push(dy, x, w._pllm_gradbuf.view(256, 256), None, True, (w, None)) and w._pllm_wgrad_queued
    (slot,) = ops._take(w)  # another writer of the same slot: the queued gradient lands first
    assert slot is w._pllm_gradbuf and launches(rec) == [("single", (256, 256))] and not w._pllm_wgrad_queued
    rec.armed = True
    rec.push(dy, x, w._pllm_gradbuf.view(256, 256), None, False, (w, None))
    ops.wgrad_flush()  # what FlatAdamW.step / grad_norm and the engines' finish_grad_sync call first
    assert len(launches(rec)) == 2 and not rec.items
    torch.testing.assert_close(w._pllm_gradbuf.view(256, 256), 2 * (dy.float().t() @ x.float()), rtol=0, atol=0)
    rec.armed = True
    rec.push(dy, x, w._pllm_gradbuf.view(256, 256), None, False, (w, None))
    ops.wgrad_defer_allow(True)  # changing the switch flushes too
    assert len(launches(rec)) == 3


def test_optimizer_and_engine_flush_first(monkeypatch):
    from pretraining_llm_amd.parallel.dp import DataParallelEngine
    from pretraining_llm_amd.train.optim import FlatAdamW
    calls = []
    monkeypatch.setattr(ops, "wgrad_flush", lambda: calls.append(1))
    opt = FlatAdamW(torch.nn.Linear(8, 8), lr=1e-3)
    n = len(calls)
    opt.grad_norm()
    assert len(calls) == n + 1
    opt.step()
    assert len(calls) == n + 2
    DataParallelEngine(opt).finish_grad_sync()
    assert len(calls) == n + 3


def test_deferral_off(monkeypatch):
    bf = torch.zeros(128, 8, dtype=torch.bfloat16)
    assert not ops._wgrad_defer_on(bf)  # a CPU tensor: not the HIP path
    monkeypatch.setattr(ops._lib, "use_hip", lambda *ts: True)
    assert ops._wgrad_defer_on(bf)
    assert not ops._wgrad_defer_on(bf[:64])  # a single K-tile: the grouped kernel peels the first of >= 2
    with ops.backend("torch"):
        assert not ops._wgrad_defer_on(bf)
    monkeypatch.setattr(ops, "WGRAD_DEFER", False)  # PLLM_AB wgrad_defer=0
    assert not ops._wgrad_defer_on(bf)
    monkeypatch.setattr(ops, "WGRAD_DEFER", True)
    ops.wgrad_defer_allow(False)  # an engine that launches collectives from the notifications
    assert not ops._wgrad_defer_on(bf)
    ops.wgrad_defer_allow(True)
    dist = torch.distributed
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    assert not ops._wgrad_defer_on(bf)  # more than one rank


def test_only_sliced_problems_are_queued(monkeypatch):
    """A problem the immediate plan runs as whole tiles (S = 1) has no slab and no reduce to save: it is not
    queued, so small models keep today's launch and notification order."""
    plans = {128: [2, 1, 128, 0, 0, 0, 0], 65536: [2, 7, 9408, 0, 0, 0, 0]}
    asked = []
    fake = type("O", (), {"wgrad_plan": staticmethod(lambda M, P, Q, f32, bias: (asked.append((M, P, Q, f32, bias)),
                                                                                 plans[M])[1])})
    monkeypatch.setattr(ops, "_ops", lambda: fake)
    x = torch.zeros(1, 768, dtype=torch.bfloat16)
    assert not ops._wgrad_sliced(x.expand(128, 768), x.expand(128, 768), None)
    assert ops._wgrad_sliced(x.expand(65536, 768), x.expand(65536, 768), torch.zeros(768))
    assert asked == [(128, 768, 768, True, False), (65536, 768, 768, True, True)]
    monkeypatch.setattr(ops, "WGRAD_DEFER_MIN_SLICES", 1)
    assert ops._wgrad_sliced(x.expand(128, 768), x.expand(128, 768), None)


def test_direct_and_reserved_calls_are_not_queued(rec, monkeypatch):
    ran = []
    monkeypatch.setattr(ops, "_ops", lambda: type("O", (), {"wgrad": staticmethod(lambda *a: ran.append(a))}))
    w = _slotted(256, rec.log)
    dy, x = torch.randn(128, 256).bfloat16(), torch.randn(128, 256).bfloat16()
    rec.armed = True
    ops._weight_grad(dy, x, w._pllm_gradbuf, overwrite=True)  # no ``notify``: the LM head's chunked calls
    assert len(ran) == 1 and not rec.items
    assert ops._reserve(w) is w._pllm_gradbuf
    dw, _ = ops._linear_param_grads(dy, x, w, None)  # a reserved slot gives no target: a returned tensor
    assert len(ran) == 2 and not rec.items and len(ran[1]) == 2


def test_plan_rule_matches_the_extension():
    """``plan_rule`` above is what csrc/gemm_plan.h computes (the stand-in tests test the real policy)."""
    if not ops._lib.available():
        pytest.skip("extension not built")
    plan = torch.ops.pllm.wgrad_group_plan
    ctas = next(c for c in range(1, 4097) if plan([c], [1], 0)[0] > 0)  # the round: the grid's workgroups
    blocks = ([36, 36, 9, 27] * 3, [12, 3, 3, 3] * 3)
    for tiles, tq, done0 in [(*blocks, 0), (*blocks, 24), ([3 * ctas + 5], [7], 0), ([5 * ctas], [12], 36),
                             ([ctas - 1, ctas - 1], [3, 3], 0), ([1] * 40, [1] * 40, 0), ([ctas - 1], [1], 0)]:
        assert plan(tiles, tq, done0)[0] == plan_rule(tiles, tq, done0, ctas), (tiles, tq, done0)
