// Stand-alone driver of csrc/gemm_plan.h (the host dispatch of gemm_tn and wgrad), for CPU tests and sanitizer
// builds: tests/test_gemm_plan.py.
//
//   gemm_plan_selftest < rows     one plan per input row, fields in the order the torch ops return them:
//     gemm  <settings> <cus> M N K epi T          -> pp quad grid tiles_m tiles_n colsum_groups
//     wgrad <settings> <cus> M P Q out_f32 bias   -> arm S slice hy_full hy_rem hy_s hy_slice_kt
//                                                    grid bias_rows fused_bias ws_floats
//     <settings> = phased reserve_cus persistent wgrad_set_mfma wgrad_set_hy wgrad_hy_cost, applied through
//     the setters to the defaults (negative: keep, as gemm_set_config does)
//   gemm_plan_selftest --sweep    checks the invariants every plan must satisfy over a sweep of shapes, grid
//                                 caps and settings; exits 1 at the first violation, naming the shape
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../gemm_plan.h"

using namespace pllm;

namespace {

GemmSettings settings(int phased, int reserve, int persistent, int wmfma, int hy, int hy_cost) {
  GemmSettings s;
  s.set_config(0, 0, phased, reserve, persistent);
  s.set_wgrad_mfma(wmfma);
  s.wgrad_hy = hy;
  s.wgrad_hy_cost = hy_cost;
  return s;
}

int rows() {
  char kind[16];
  int st[6], cus, n = 0;
  while (std::scanf("%15s %d %d %d %d %d %d %d", kind, &st[0], &st[1], &st[2], &st[3], &st[4], &st[5], &cus) == 8) {
    const GemmSettings s = settings(st[0], st[1], st[2], st[3], st[4], st[5]);
    int a[5];
    if (std::scanf("%d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4]) != 5) break;
    if (std::strcmp(kind, "gemm") == 0) {
      const GemmPlan p = gemm_plan(s, cus, a[0], a[1], a[2], a[3], a[4]);
      std::printf("%d %d %d %d %d %d\n", (int)p.pp, (int)p.quad, p.grid, p.tiles_m, p.tiles_n, p.colsum_groups);
    } else if (std::strcmp(kind, "wgrad") == 0) {
      const WgradPlan p = wgrad_plan(s, cus, a[0], a[1], a[2], a[3] != 0, a[4] != 0);
      std::printf("%d %d %d %d %d %d %d %d %d %d %" PRId64 "\n", p.arm, p.S, p.slice, p.hy_full, p.hy_rem, p.hy_s,
                  p.hy_slice_kt, p.grid, p.bias_rows, (int)p.fused_bias, p.ws_floats);
    } else {
      std::fprintf(stderr, "unknown row kind %s\n", kind);
      return 2;
    }
    ++n;
  }
  if (!std::feof(stdin)) {
    std::fprintf(stderr, "malformed row after %d rows\n", n);
    return 2;
  }
  return 0;
}

#define REQUIRE(cond)                                                                                  \
  do {                                                                                                   \
    if (!(cond)) {                                                                                       \
      std::fprintf(stderr, "violated: %s\n  %s\n", #cond, what);                                         \
      return false;                                                                                      \
    }                                                                                                    \
  } while (0)

// slices of `per` K-tiles cover kst K-tiles with a non-empty last one
bool covers(int n, int per, int kst) { return (int64_t)(n - 1) * per < kst && kst <= (int64_t)n * per; }

bool check_wgrad(const GemmSettings& s, int cus, int M, int P, int Q, bool of32, bool bias) {
  const WgradPlan p = wgrad_plan(s, cus, M, P, Q, of32, bias);
  char what[256];
  std::snprintf(what, sizeof what,
                "wgrad M %d P %d Q %d out_f32 %d bias %d | reserve %d persistent %d set_mfma (%d, pp %d) hy %d "
                "hy_cost %d -> arm %d S %d slice %d hy %d %d %d %d grid %d",
                M, P, Q, (int)of32, (int)bias, s.reserve_cus, s.persistent, s.wgrad_mfma, (int)s.wgrad_pp, s.wgrad_hy,
                s.wgrad_hy_cost, p.arm, p.S, p.slice, p.hy_full, p.hy_rem, p.hy_s, p.hy_slice_kt, p.grid);
  const int cap = grid_cap(s, cus), kst = M / 64;
  const int64_t ntiles = (int64_t)((P + 255) / 256) * ((Q + 255) / 256);
  REQUIRE(p.S >= 1);
  REQUIRE(p.slice > 0 && p.slice % 64 == 0);
  REQUIRE(covers(p.S, p.slice / 64, kst));
  REQUIRE(p.arm >= 0 && p.arm <= 3);
  if (p.arm == 2) REQUIRE(of32 && p.slice / 64 >= 2 && s.wgrad_pp);
  if (p.arm == 3) REQUIRE(of32 && !bias && s.wgrad_hy && s.wgrad_pp && ntiles > cap);
  if (s.wgrad_mfma == 16) REQUIRE(p.arm == 0);
  if (s.wgrad_mfma == 32) REQUIRE(p.arm == 1);
  if (!s.wgrad_pp) REQUIRE(p.arm <= 1);
  int64_t items;
  if (p.arm != 3) {
    REQUIRE(p.ws_floats == (p.S > 1 ? (int64_t)p.S * P * Q : 0));
    REQUIRE(p.bias_rows == (bias ? p.S : 0));
    REQUIRE(p.fused_bias == (bias && (p.arm == 0 || p.arm == 2)));
    REQUIRE(p.hy_full == 0 && p.hy_rem == 0 && p.hy_s == 0 && p.hy_slice_kt == 0);
    items = ntiles * p.S;
  } else {
    REQUIRE(p.hy_full + p.hy_rem == ntiles);
    REQUIRE(p.hy_full > 0 && p.hy_full % cap == 0);
    REQUIRE(p.hy_rem >= 0 && p.hy_rem < cap);
    REQUIRE(!p.fused_bias && p.bias_rows == 0);
    REQUIRE(p.hy_slice_kt >= 1);
    if (p.hy_rem == 0) {
      REQUIRE(p.hy_s == 0 && p.ws_floats == 0);
    } else {
      REQUIRE(p.hy_s >= 1 && covers(p.hy_s, p.hy_slice_kt, kst));
      REQUIRE(p.hy_s == 1 || p.hy_slice_kt >= 2);  // the kernel peels the first K-tile of a slice
      REQUIRE(p.ws_floats == (int64_t)p.hy_rem * p.hy_s * 256 * 256);
    }
    items = p.hy_full + (int64_t)p.hy_rem * p.hy_s;
  }
  // the one-barrier kernel (arms 0 / 1) is not persistent: one workgroup per work item, whatever the cap
  REQUIRE(p.grid == (p.arm <= 1 ? items : std::min<int64_t>(items, cap)));
  return true;
}

bool check_gemm(const GemmSettings& s, int cus, int M, int N, int K, int epi, int T) {
  const GemmPlan p = gemm_plan(s, cus, M, N, K, epi, T);
  char what[256];
  std::snprintf(what, sizeof what,
                "gemm M %d N %d K %d epi %d T %d | phased %d reserve %d persistent %d -> pp %d quad %d grid %d tiles "
                "%d x %d colsum %d",
                M, N, K, epi, T, s.phased, s.reserve_cus, s.persistent, (int)p.pp, (int)p.quad, p.grid, p.tiles_m,
                p.tiles_n, p.colsum_groups);
  const bool pp = s.phased == 4 && K >= 128 && (epi != 6 || T % 16 == 0);
  const bool quad = pp && K >= 2048 && (epi == 0 || epi == 2 || epi == 3 || epi == 4 || epi == 6);
  REQUIRE(p.pp == pp && p.quad == quad);
  REQUIRE(p.tiles_m == (M + 255) / 256);
  REQUIRE(p.tiles_n == (pp && epi == 7 ? (N + 127) / 128 : (N + 255) / 256));
  REQUIRE(p.colsum_groups == (s.phased == 4 && K >= 2048 ? 4 : 2) * p.tiles_m);
  REQUIRE(p.grid == std::min<int64_t>((int64_t)p.tiles_m * p.tiles_n, grid_cap(s, cus)));
  return true;
}

int sweep() {
  const int cus = 256;
  // grid caps 256, 248, 8 and (not persistent) 2^30
  const int caps[4][2] = {{0, 1}, {8, 1}, {248, 1}, {0, 0}};
  const int Ms[] = {64, 128, 192, 256, 512, 576, 1024, 1216, 2048, 4672, 8192, 16384, 32768, 65536};
  const int PQs[] = {8, 136, 200, 256, 264, 520, 768, 776, 2048, 2304, 3072, 5504, 6144, 11008, 16384, 50304};
  long plans = 0;
  for (const auto& c : caps)
    for (int wmfma : {0, 16, 32, 100})
      for (int hy = 0; hy <= 1; ++hy)
        for (int hy_cost = 0; hy_cost <= 1; ++hy_cost) {
          const GemmSettings s = settings(4, c[0], c[1], wmfma, hy, hy_cost);
          for (int M : Ms)
            for (int P : PQs)
              for (int Q : PQs)
                for (int flags = 0; flags < 4; ++flags, ++plans)
                  if (!check_wgrad(s, cus, M, P, Q, (flags & 1) != 0, (flags & 2) != 0)) return 1;
        }
  const int GMs[] = {1, 17, 129, 256, 257, 520, 32768, 65536};
  const int GNs[] = {8, 72, 136, 264, 520, 776, 2304, 5504, 11008};
  for (const auto& c : caps)
    for (int phased : {4, 0, 2}) {
      const GemmSettings s = settings(phased, c[0], c[1], 0, 1, 1);
      for (int M : GMs)
        for (int N : GNs)
          for (int K : {64, 128, 192, 768, 2048, 2112})
            for (int epi = 0; epi <= 7; ++epi)
              for (int T : {0, 16, 24}) {
                ++plans;
                if (!check_gemm(s, cus, M, N, K, epi, T)) return 1;
              }
    }
  std::printf("gemm_plan_selftest sweep ok: %ld plans\n", plans);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--sweep") == 0) return sweep();
  return rows();
}
