"""CPU checks of the FP8 decode references (tests/_fp8_refs.py): the quantiser's definition on ``quant_ref``
itself, the calibration of the gemv_fp8 budgets on fp32 CPU models, and the defects that the checks reject."""
import pytest
import torch

import _fp8_refs as R
import _gemm_refs as G
import _streaming_refs as S
from _streaming_refs import BF16, F32, F64


def _rejected(items):
    with pytest.raises(AssertionError):
        R.check_all(items)


# ------------------------------------------------------------------------------------------------ codes, quantiser
def test_code_table_is_ocp_e4m3fn():
    v = R.code_values()
    assert len(R.FINITE_CODES) == 254 and torch.isnan(v[0x7f]) and torch.isnan(v[0xff])
    assert v[0x7e] == 448.0 and v[0xfe] == -448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6
    assert v[0x38] == 1.0 and v[0x00] == 0.0  # (fnuz: 0x38 is 0.5, 0x7f is 240)
    assert torch.equal(v[list(R.FINITE_CODES)].to(BF16).float(), v[list(R.FINITE_CODES)])  # exact in bf16


@pytest.mark.parametrize("N,K", R.QUANT_SHAPES)
def test_quant_ref_gives_nearest_codes_ties_to_even(N, K):
    w = R.quant_inputs(N, K)
    q, scale = R.quant_ref(w)
    rep = R.nearest_code_report(w, q, scale)
    print(rep)
    assert rep["violations"] == rep["odd_ties"] == rep["nan_codes"] == rep["sign_flips"] == rep["bad_scales"] == 0
    if N >= 4:
        # the planted row (when it fits) and those of the random rows: tie handling matters
        assert rep["ties"] >= min(K - 2, 2 * 126)
        assert scale[1] == 1.0 and (q[1] == 0).all()                     # the all-zero row
        assert q[2, -1] == 0x7e and q[2, -2] == 0xfe                     # +-amax -> +-448
        assert scale[3] == 2.0 ** -7 and q[3, 0] == 0x7e and q[3, 1] == 0xfe
        assert int((q[3] & 1).sum()) == 0                                # every planted tie took the even code
    # the ops layer's CPU quantiser is the same function
    from pretraining_llm_amd.ops import reference as ref
    q2, s2 = ref.quantize_rows_fp8(w)
    assert torch.equal(q2, q) and torch.equal(s2, scale)
    assert torch.equal(ref.dequantize_fp8(q, scale).to(F64), R.dq64(q, scale).to(F32).to(F64))


def test_quantiser_defects_are_rejected():
    w = R.quant_inputs(300, 520)
    q, scale = R.quant_ref(w)
    qt, st = R.quant_trunc(w)
    rep = R.nearest_code_report(w, qt, st)
    assert rep["violations"] > 1000 and not torch.equal(qt, q)
    q240, s240 = R.quant_amax240(w)
    rep = R.nearest_code_report(w, q240, s240)
    assert rep["bad_scales"] == 299 and rep["violations"] > 1000  # (the all-zero row keeps scale 1)


# ------------------------------------------------------------------------------------------------ gemv_fp8 budgets
def _cases():
    return [c for c in G.gemv_cases() if c[0] in (1, 8)]


def _model_items():
    for M, N, K, bias in _cases():
        inp = R.fp8_inputs(M, N, K)
        for chain in (False, True):
            yield ("gemv_fp8_y", f"y {M}x{N}x{K}", R.gemv_fp8_model(inp, N, K, bias=bias, chain=chain)["y"],
                   R.gemv_fp8_ref(inp, bias))
    for M, N, K, norm, wr in G.gemv_norm_cases():
        inp = R.fp8_inputs(M, N, K, norm)
        ref = R.gemv_fp8_norm_ref(inp, norm == 2, wr)
        for chain in (False, True):
            out = R.gemv_fp8_model(inp, N, K, norm, wr, chain=chain)
            yield ("gemv_fp8_norm_y", f"y {M}x{N}x{K}", out["y"], ref["y"])
            if wr:
                yield ("exact", "s", out["s"], ref["s"])


def test_fp8_budgets_are_calibrated_on_the_fp32_models():
    measured, worst = {}, {}
    for it in _model_items():
        op, name, out, (ref, unit) = it
        u = S.ulps_needed(out, ref, unit)
        if u >= measured.get(op, -1):
            measured[op], worst[op] = u, it
    print("measured smallest budgets:", measured)
    assert {op: m for op, m in measured.items() if op in R.BUDGET} == {op: b[0] for op, b in R.BUDGET.items()}, \
        "the table in _fp8_refs.py is stale"
    assert measured["exact"] == 0
    for op, (m, b) in R.BUDGET.items():
        assert b == 2 * m and m > 0
        R.check_all([worst[op]])
        with pytest.raises(AssertionError):
            S.assert_close_ulps(worst[op][2], worst[op][3][0], 0, 0.0)


def test_fp8_reference_matches_the_dequantised_double_product():
    M, N, K = 3, 1032, 520
    inp = R.fp8_inputs(M, N, K)
    ref, unit = R.gemv_fp8_ref(inp)
    dq = R.dq64(inp["q"], inp["scale"])
    alt = inp["x"].to(F64) @ dq.t() + inp["bias"].to(F64)
    assert ((ref - alt).abs() <= 1e-12 * (unit / S.E32)).all()
    # quantisation error itself is far outside the bound: the reference is the QUANTISED product, not x w^T
    _rejected([("gemv_fp8_y", "bf16 weights", G.gemv_model_outputs(inp, N, K)["y"], (ref, unit))])


# ------------------------------------------------------------------------------------------------ defects
@pytest.mark.parametrize("M,N,K", [(1, 1032, 520), (8, 8197, 768)])
def test_gemv_fp8_defects_are_rejected(M, N, K):
    inp = R.fp8_inputs(M, N, K)
    ref = R.gemv_fp8_ref(inp)
    good = R.gemv_fp8_model(inp, N, K, chain=True)
    R.check_all([("gemv_fp8_y", "y", good["y"], ref)])
    acc, scale, b = good["acc"], inp["scale"], inp["bias"].float()
    x, codes = inp["x"].float(), R.values_of(inp["q"])

    def y_of(v):
        return [("gemv_fp8_y", "y", v.to(BF16), ref)]

    _rejected(y_of(0.5 * acc * scale + b))                       # codes decoded as e4m3 fnuz: every value halved
    _rejected(y_of(acc + b))                                     # the scale dropped
    _rejected(y_of((acc + b) * scale))                           # the scale applied after the bias
    _rejected(y_of((x[:, :K - 8] @ codes[:, :K - 8].t()) * scale + b))  # the last K chunk skipped
    _rejected(y_of(acc * scale.roll(1) + b))                     # the scale of the neighbouring column
    qt, _ = R.quant_trunc(inp["w"])                              # a truncating quantiser's codes
    _rejected(y_of((x @ R.values_of(qt).t()) * scale + b))
    q240, s240 = R.quant_amax240(inp["w"])                       # scale = amax / 240 with the codes of amax / 448
    _rejected(y_of(acc * s240 + b))


def test_scale_seam_case_has_neighbouring_scales_2_20_apart():
    inp = R.fp8_inputs(3, 2056, 520, seam=True)
    r = inp["scale"][1:] / inp["scale"][:-1]
    assert ((r > 2.0 ** 17) | (r < 2.0 ** -17)).all()
    good = R.gemv_fp8_model(inp, 2056, 520, chain=True)
    R.check_all([("gemv_fp8_y", "y", good["y"], R.gemv_fp8_ref(inp))])
    wg = good["acc"] * inp["scale"].view(-1, 4)[:, :1].expand(-1, 4).reshape(-1) + inp["bias"].float()
    _rejected([("gemv_fp8_y", "scale per workgroup", wg.to(BF16), R.gemv_fp8_ref(inp))])


def test_snap_to_fp8_grid_makes_quantisation_lossless():
    from pretraining_llm_amd.models import GPT, get_preset
    torch.manual_seed(0)
    model = GPT(get_preset("gpt2-tiny").replace(vocab_size=512, context_length=64)).to(BF16).eval()
    assert R.snap_to_fp8_grid(model) == len(model._decode_weight_params())
    for _, p in model._decode_weight_params():
        q, scale = R.quant_ref(p)
        assert torch.equal(torch.exp2(torch.log2(scale).round()), scale)        # powers of two
        assert torch.equal(R.dq64(q, scale).to(BF16), p.detach())               # the round trip is bitwise
