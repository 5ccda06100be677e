"""The host dispatch of ``gemm_tn`` and ``wgrad`` (csrc/gemm_plan.h) on the CPU, through the stand-alone program
csrc/host/selftest/gemm_plan_selftest.cpp built plain and under AddressSanitizer + UBSan:

* the pinned rows of ``_gemm_refs`` (WGRAD_CASES / WGRAD_HYBRID, the GEMM edge shapes) under the rules the GPU edge
  tests assert through ``torch.ops.pllm.gemm_plan`` / ``wgrad_plan``;
* tests/fixtures/gemm_plans.json: what those two ops returned on an MI355X before the dispatch moved into
  gemm_plan.h, under the default settings and every A/B setting -- every field must still be equal;
* the program's own sweep of the invariants a plan must satisfy (workspace sizes, slice cover, grids)."""
import json
import os
import shutil
import subprocess

import pytest

import _gemm_refs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pretraining_llm_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "fixtures", "gemm_plans.json")
CUS = 256
GRID8 = CUS - 8                   # reserve_cus that leaves the persistent grids 8 workgroups
DEFAULT = (4, 0, 1, 0, 1, 1)      # phased, reserve_cus, persistent, wgrad_set_mfma, wgrad_set_hy, wgrad_hy_cost
ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:verify_asan_link_order=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    san = request.param
    out = tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_selftest"
    flags = ["-O2"] if san == "plain" else ["-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
    src = os.path.join(CSRC, "host", "selftest", "gemm_plan_selftest.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-Wall", *flags, src, "-o", str(out)], capture_output=True, text=True,
                           timeout=240)
    if build.returncode != 0 and "cannot find" in build.stderr and "san" in build.stderr:
        pytest.skip(f"sanitizer runtime for {san} not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    return str(out)


def _clean(stderr):
    return "ERROR: AddressSanitizer" not in stderr and "runtime error" not in stderr and "violated" not in stderr


def _plans(exe, rows):
    """rows: (kind, settings, cus, shape and flags) -> one list of ints per row."""
    text = "".join(" ".join(map(str, [kind, *st, cus, *args])) + "\n" for kind, st, cus, args in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and _clean(r.stderr), (r.returncode, r.stderr[-4000:])
    out = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(out) == len(rows)
    return out


def _settings(**kw):
    s = dict(zip(("phased", "reserve", "persistent", "wmfma", "hy", "hy_cost"), DEFAULT))
    s.update(kw)
    return tuple(s.values())


def test_header_is_plain_cxx():
    """No HIP, torch or environment access in the plan header."""
    src = open(os.path.join(CSRC, "gemm_plan.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ["<algorithm>", "<cstdint>"], includes
    assert "getenv" not in src


def test_wgrad_pinned_cases(exe):
    rows, want = [], []
    for name, (M, P, Q, S, slice_rows, grid8) in G.WGRAD_CASES.items():
        for mf in (0, 16, 32):
            for of32 in (False, True):
                for bias in (False, True):
                    rows.append(("wgrad", _settings(reserve=GRID8 if grid8 else 0, wmfma=mf), CUS,
                                 (M, P, Q, int(of32), int(bias))))
                    want.append((name, mf, of32, bias, G.expect_wgrad_plan(name, mf, of32, bias)))
    for (kind, st, cus, (M, P, Q, of32, bias)), plan, (name, mf, _, _, exp) in zip(rows, _plans(exe, rows), want):
        assert plan[:7] == exp, (name, mf, of32, bias, plan)
        arm, S = plan[0], plan[1]
        grid, bias_rows, fused, ws = plan[7:]
        tiles = -(-P // 256) * -(-Q // 256)
        if arm == 3:
            full, rem, hs, _ = plan[3:7]
            assert (grid, bias_rows, fused, ws) == (min(full + rem * hs, 8), 0, 0, rem * hs * 256 * 256), (name, plan)
        else:
            assert grid == (min(tiles * S, 8 if st[1] else CUS) if arm == 2 else tiles * S), (name, plan)
            assert (bias_rows, fused, ws) == (S * bias, int(bias and arm != 1), S * P * Q if S > 1 else 0), (name, plan)


@pytest.mark.parametrize("phased", [4, 0])
def test_gemm_pinned_cases(exe, phased):
    cases = [(M, N, K, e, 0) for (M, N, K) in G.GEMM_SHAPES for e in range(6)]
    if phased == 4:  # epilogue 7 runs on the ping-pong kernel only
        cases += [(M, N, K, 7, 0) for (M, N, K) in G.GEMM_SHAPES + (G.SWIGLU_F136,) if K >= 128]
    cases += [(B * T, N, K, 6, T) for (B, T, N, K) in G.DELTA_CASES]
    for reserve, cap in ((0, CUS), (GRID8, 8)):
        rows = [("gemm", _settings(phased=phased, reserve=reserve), CUS, c) for c in cases]
        for (M, N, K, epi, T), plan in zip(cases, _plans(exe, rows)):
            head, tail = G.expect_gemm_plan(M, N, K, epi, phased, T)
            assert plan[:2] == head and plan[3:] == tail, (plan, (M, N, K, epi, T))
            assert plan[2] == min(tail[0] * tail[1], cap), (plan, (M, N, K, epi, T))
    tiled = [("gemm", _settings(phased=phased, reserve=r), CUS, (*G.GEMM_TILED[0], 0, 0)) for r in (0, GRID8)]
    assert [p[2] for p in _plans(exe, tiled)] == [12, 8]  # the grids test_gemm_tn_grids_agree_bitwise runs on


def test_same_plans_as_recorded(exe):
    """Every field the ops returned before the refactor, on the recorded CU count."""
    with open(FIXTURE) as f:
        rec = json.load(f)
    assert 200 <= len(rec["rows"]) <= 1000
    recorded_under = {tuple(r[1]) for r in rec["rows"]}
    assert recorded_under >= {DEFAULT, _settings(phased=0), _settings(wmfma=16), _settings(wmfma=32),
                              _settings(wmfma=100), _settings(hy=0), _settings(persistent=0),
                              _settings(reserve=rec["cus"] - 8), _settings(hy_cost=0)}
    rows = [(kind, st, rec["cus"], args) for kind, st, args, _ in rec["rows"]]
    bad = [(r, got) for r, got in zip(rec["rows"], _plans(exe, rows)) if got[:len(r[3])] != r[3]]
    assert not bad, (len(bad), bad[:5])


def test_sweep_invariants(exe):
    r = subprocess.run([exe, "--sweep"], capture_output=True, text=True, timeout=240, env=ENV)
    assert r.returncode == 0 and "sweep ok" in r.stdout and _clean(r.stderr), (r.stdout[-500:], r.stderr[-4000:])
