"""CPU checks of ``_qk_norm_refs``: the fp64 references against autograd in double precision (``F.rms_norm`` and
an independent form of the rotation) to 1e-12 relative, and the calibration of the budgets against a plain fp32
evaluation of the cases that ``test_qk_norm_gpu.py`` runs on the HIP kernels."""
import pytest
import torch
import torch.nn.functional as F

import _qk_norm_refs as Q
import _streaming_refs as R
from pretraining_llm_amd.ops import reference as ref

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32


def _same(a, b, what, tol=1e-12):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert float((a - b).abs().max()) <= tol * scale, f"{what}: {float((a - b).abs().max())} vs scale {scale}"


SUBSET = [c for c in Q.cases() if (c["B"], c["T"]) == (1, 67) and (c["H"], c["Hkv"]) == (4, 2)]


@pytest.mark.parametrize("case", SUBSET, ids=Q.case_id)
def test_refs_match_torch_double(case):
    inp = Q.inputs(**case)
    D, H, Hkv, T, pos = inp["D"], inp["H"], inp["Hkv"], inp["T"], inp["pos"]
    rows = inp["qkv"].shape[0]
    x = inp["qkv"].to(F64).requires_grad_()
    wq, wk = inp["wq"].to(F64).requires_grad_(), inp["wk"].to(F64).requires_grad_()
    eps = R.f32r(inp["eps"])
    q = F.rms_norm(x[:, : H * D].view(rows, H, D), (D,), wq, eps)
    k = F.rms_norm(x[:, H * D:(H + Hkv) * D].view(rows, Hkv, D), (D,), wk, eps)
    yn = torch.cat([q.reshape(rows, -1), k.reshape(rows, -1)], -1)  # normalised, un-rotated
    y = yn
    if inp["cos"] is not None:  # y cos + rotate_half(y) sin with the tables repeated over both halves
        c = inp["cos"][pos:pos + T].to(F64).repeat(1, 2)[:, None, :]
        s = inp["sin"][pos:pos + T].to(F64).repeat(1, 2)[:, None, :]
        rot = lambda t: t * c + torch.cat([-t[..., D // 2:], t[..., : D // 2]], -1) * s  # noqa: E731
        y = torch.cat([rot(q).reshape(rows, -1), rot(k).reshape(rows, -1)], -1)
    fw = Q.fwd_ref(**inp)
    # the package's own fp32 oracle agrees with the reference to fp32 precision
    o32 = ref.qk_norm(inp["qkv"][:, : H * D].float().view(1, rows, H, D), inp["wq"].float(), inp["eps"])
    if inp["cos"] is not None:
        o32 = ref.rope(o32, inp["cos"][pos:pos + T], inp["sin"][pos:pos + T])
    _same(o32.reshape(rows, -1), fw["y"][0][:, : H * D], "ops.reference.qk_norm", tol=1e-5)
    _same(fw["y"][0], y.detach(), "y")
    xh = Q._heads(inp["qkv"], H, Hkv, D, F64)
    _same(fw["rstd"][0], (xh.pow(2).mean(-1) + eps).rsqrt(), "rstd")
    # the backward takes the gradient of the normalised, un-rotated heads, from the exact statistics here
    dy = inp["dqkv"][:, : (H + Hkv) * D].to(F64)
    dx, dwq, dwk = torch.autograd.grad(yn, [x, wq, wk], dy)
    bw = Q.bwd_ref(inp["dqkv"], inp["qkv"], fw["rstd"][0], inp["wq"], inp["wk"], D, H, Hkv)
    _same(bw["dx"][0], dx[:, : (H + Hkv) * D], "dx")
    assert not dx[:, (H + Hkv) * D:].any()
    _same(bw["dwq"][0], dwq, "dwq")
    _same(bw["dwk"][0], dwk, "dwk")


def test_case_list_covers_the_issue():
    cs = Q.cases()
    assert {c["D"] for c in cs} == {32, 64, 128}
    assert {(c["H"], c["Hkv"]) for c in cs} == {(4, 4), (4, 2), (8, 1)}
    assert {(c["B"], c["T"]) for c in cs} == {(2, 5), (1, 67), (3, 128)}
    assert {(c["rope"], c["pos"]) for c in cs} == {(0, 0), (1, 0), (1, 9)}
    assert {c["scale"] for c in cs} == {1.0, 2.0 ** -40, 2.0 ** 20}
    inp = Q.inputs(**cs[0])
    heads = Q._heads(inp["qkv"], inp["H"], inp["Hkv"], inp["D"], F32)
    zero = ~heads.any(-1)
    assert zero[:, : inp["H"]].any() and zero[:, inp["H"]:].any()  # an all-zero q head and k head
    assert torch.allclose(Q.fwd_ref(**inp)["rstd"][0][zero], torch.tensor(R.f32r(Q.EPS), dtype=F64) ** -0.5)
    for w in (inp["wq"], inp["wk"]):
        assert (w == 0).any() and (w < 0).any()
    # the big backward case: >= 8 passes of the backward's capped grid
    per_row = (Q.BIG["H"] + Q.BIG["Hkv"]) * (Q.BIG["D"] // 16)
    assert Q.BIG_ROWS * per_row >= 8 * Q.BWD_PASS_THREADS
    assert Q.BIG_ROWS * (Q.BIG["H"] + 2 * Q.BIG["Hkv"]) * Q.BIG["D"] * 2 < 64 * 2 ** 20  # bf16 bytes of qkv


def _model_items():
    for c in Q.cases():
        inp = Q.inputs(**c)
        out = Q.model_f32(inp)
        yield from Q.fwd_checks(inp, out)
        yield from Q.bwd_checks(inp, out)
    inp = Q.inputs(**Q.BIG)
    yield from Q.bwd_checks(inp, Q.model_f32(inp, forward=False))


def test_budgets_are_calibrated_on_the_fp32_model():
    measured = {}
    for op, name, out, (r, unit) in _model_items():
        measured[op] = max(measured.get(op, 0), R.ulps_needed(out, r, unit))
    print("measured smallest budgets:", measured)
    assert measured == {op: b[0] for op, b in Q.BUDGET.items()}, "the table in _qk_norm_refs.py is stale"
    for m, b in Q.BUDGET.values():
        assert b == 2 * m
