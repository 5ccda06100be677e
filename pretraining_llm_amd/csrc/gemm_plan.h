// Host dispatch of the fused-epilogue GEMM (gemm.hip, gemm_pp.hip) and the weight-gradient GEMM
// (gemm_wgrad.hip, wgrad_pp.hip): which kernel serves a call, on what grid, with what workspace.
// One plan per launch, computed here from the settings and the shape; the bindings size their
// buffers from it and the launchers run it.  Plain C++17 integer logic, no HIP and no torch header,
// so it also builds as a stand-alone host program (host/selftest/gemm_plan_selftest.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

#ifndef PL_GEMM_GROUP_M
#define PL_GEMM_GROUP_M 4  // m-tiles per tile group (L2 reuse of the B panels; A/B builds)
#endif

namespace pllm {

// tile geometry the plans count in; each kernel file static_asserts its own constants against these
constexpr int kPlanTile = 256;       // output tile rows and columns (GT / PT / BT / WT)
constexpr int kPlanKTile = 64;       // tokens per K-tile of the weight-gradient kernels (BKM / WBK)
constexpr int kPlanTileNSwiglu = 128;  // output tile columns of epilogue 7 on the ping-pong kernel

struct GemmSettings {
  int mfma = 16;  // fallback TN kernel's MFMA shape (16: 16x16x32, 32: 32x32x16; tests only)
  int group_m = PL_GEMM_GROUP_M;
  // 0: every wave issues its DMA pieces; 2: the asymmetric DMA (waves 0-3 issue all).  Measured and
  // removed (profiles/r3_gemm_tn.md): 1 = two k32 phases per K-tile with counted vmcnt across raw
  // barriers (3-12 % slower), 3 = one wave per SIMD with 128x128 per wave and the DMA pinned between
  // MFMA groups (hipBLASLt's geometry; 4-18 % slower, its fused epilogues up to 40 % slower)
  // 4 (default): the ping-pong kernel of gemm_pp.hip (two wave groups one barrier apart, counted
  // waits): 4-6 % faster than gemm.hip's kernel on every fused epilogue measured (GELU' / SwiGLU' /
  // attention delta; profiles/r4_gemm_pp.md), whole GPT-2 step +0.5 %.
  // gemm.hip's kernel is the FALLBACK for what the ping-pong loop does not take (a single K-tile,
  // K < 128; the delta epilogue with T % 16 != 0); 0 / 2 select it for every shape (tests only).  Its
  // 32x32x16 and asymmetric-DMA instantiations run only under gemm_set_config from the tests.
  int phased = 4;
  // CUs the persistent grids leave free, for RCCL kernels overlapping the backward (world > 1)
  int reserve_cus = 0;
  // 0: the persistent kernels (gemm_pp / wgrad_pp / gemm.hip's) launch one workgroup per tile instead
  // of one per CU, so the hardware deals tiles to whichever CUs are free (e.g. beside RCCL kernels)
  int persistent = 1;
  // Weight-gradient variant (set_wgrad_mfma): 0 = default -- the ping-pong kernel of wgrad_pp.hip where it
  // applies (fp32 gradient target), else gemm_wgrad.hip's kernel per shape; 100 = gemm_wgrad.hip's kernel per
  // shape (as does any other non-zero value); 16 / 32 = that kernel with that MFMA shape.
  // Same-box A/B of the MFMA shapes (profiles/r3_wgrad_asym_ab.md): 16x16x32 wins everywhere except the
  // LM-head shapes (P = vocabulary), where 32x32x16 does (+0.5-4 %)
  int wgrad_mfma = 0;  // 0: per shape
  bool wgrad_pp = true;
  // hybrid weight gradients, default on: with more tiles than CUs, whole tiles for the whole
  // rounds and slices only for the last one -- LM head 65536 x 50304 x 768 3,984 vs 4,081 us, 32768 x 50304 x
  // 2048 5,190 vs 5,721 us, GPT-2 step +0.3 %, llama +0.2-0.3 % (profiles/r4_wgrad_hybrid.md).  On the
  // persistent grid only (whole rounds of one tile per CU); with a grid per tile the hardware deals the tiles
  // anyway.  (Full stream-K -- equal K-tile runs per workgroup -- lost 13-47 %: r4_wgrad_stream_k_negative.md)
  int wgrad_hy = 1;
  int wgrad_hy_cost = 1;  // PLLM_AB key wgrad_hy_cost: the hybrid remainder sliced by the cost model

  // negative values (mfma: any but 16 / 32; group_m: any but > 0) keep the current setting
  void set_config(int mfma_, int group_m_, int phased_, int reserve_cus_, int persistent_) {
    if (mfma_ == 16 || mfma_ == 32) mfma = mfma_;
    if (group_m_ > 0) group_m = group_m_;
    if (phased_ >= 0) phased = phased_;
    if (reserve_cus_ >= 0) reserve_cus = reserve_cus_;
    if (persistent_ >= 0) persistent = persistent_;
  }
  void set_wgrad_mfma(int mf) {
    wgrad_pp = mf == 0;
    wgrad_mfma = (mf == 16 || mf == 32) ? mf : 0;
  }
};

// persistent grid: one workgroup per CU, minus the CUs reserved for concurrent collectives;
// non-persistent: no cap (one workgroup per tile / work item)
inline int grid_cap(const GemmSettings& s, int cus) {
  if (!s.persistent) return 1 << 30;
  return cus - s.reserve_cus > 8 ? cus - s.reserve_cus : 8;
}

inline int plan_tiles(int n, int tile) { return (int)(((int64_t)n + tile - 1) / tile); }
inline int plan_grid(int64_t items, int cap) { return (int)std::min<int64_t>(items, cap); }

// ---------------------------------------------------------------- gemm_tn
struct GemmPlan {
  bool pp;    // the ping-pong kernel (gemm_pp.hip); else the fallback (gemm.hip)
  bool quad;  // ping-pong kernel: quadrant epilogues
  int tiles_m, tiles_n;
  int grid;           // workgroups
  int colsum_groups;  // column-sum partial rows of the EPI 3 / 4 bias gradient
};

inline GemmPlan gemm_plan(const GemmSettings& s, int cus, int M, int N, int K, int epi, int T) {
  GemmPlan p;
  // the ping-pong kernel serves a call when selected, with >= 2 K-tiles and (epilogue 6) 16 | T
  const bool pp_k = s.phased == 4 && K >= 128;
  p.pp = pp_k && (epi != 6 || T % 16 == 0);
  // quadrant epilogues at K >= 2048, except EPI 5 (aux too large for the LDS) and EPI 1 (the GELU's
  // VALU work in the LOAD segments: 1410 vs 1344 us for the end-of-tile form + hipBLASLt at the llama
  // shape 32768 x 11008 x 2048, profiles/r4_gemm_pp.md)
  // (EPI 7 has no quadrant form either: its instantiation is always the end-of-tile one)
  p.quad = p.pp && K >= 2048 && epi != 5 && epi != 1 && epi != 7;
  p.tiles_m = plan_tiles(M, kPlanTile);
  p.tiles_n = plan_tiles(N, p.pp && epi == 7 ? kPlanTileNSwiglu : kPlanTile);
  p.grid = plan_grid((int64_t)p.tiles_m * p.tiles_n, grid_cap(s, cus));
  // 2 per tile row in the fallback kernel, 4 (one per accumulator quadrant row half and wave row) in
  // the ping-pong kernel's quadrant epilogues, 2 otherwise -- decided as for epilogue 3 whatever epi is
  p.colsum_groups = (pp_k && K >= 2048 ? 4 : 2) * p.tiles_m;
  return p;
}

// ---------------------------------------------------------------- wgrad
struct WgradPlan {
  // 0 / 1: gemm_wgrad.hip's kernel with 16x16x32 / 32x32x16 MFMAs, 2: the ping-pong kernel, 3: its hybrid form
  int arm;
  int S, slice;   // split-K slices and tokens per slice (arms 0-2; reported on arm 3 too)
  int hy_full, hy_rem, hy_s, hy_slice_kt;  // arm 3: whole tiles, sliced tiles, their slice count, K-tiles per slice
  int grid;       // workgroups: one per work item on arms 0 / 1, min(work items, cap) on the persistent arms
  int bias_rows;  // rows [P] of the bias-gradient workspace the caller allocates when it passes a bias target
  bool fused_bias;  // the launch also produces the bias gradient (else the caller runs bias_grad)
  int64_t ws_floats;  // fp32 workspace: S slabs [P, Q] when S > 1, or the hybrid form's tile pieces
};

inline WgradPlan wgrad_plan(const GemmSettings& s, int cus, int M, int P, int Q, bool out_f32, bool bias) {
  WgradPlan p{};
  const int ntiles = plan_tiles(P, kPlanTile) * plan_tiles(Q, kPlanTile);
  const int kst = M / kPlanKTile;
  const int ctas = grid_cap(s, cus);
  {
    // Split-K slice count from a cost model: rounds of 256 workgroups (one per CU) x stages per
    // slice x ~2.0 us per 256x256x64 stage, plus -- for S > 1 -- the fp32 slab traffic (S slabs
    // written by the main kernel and read back by the reduce) at ~4 TB/s.  The slab term is what
    // keeps S small when P x Q is large (llama MLP: 11008 x 2048 at 16K tokens -> S = 2, not 11).
    // >= 8 stages per slice; near-ties (< 2 %) go to fewer slices.
    int best = 1;
    double best_t = 1e30;
    for (int c = 1; c <= 64; ++c) {
      if (c > 1 && kst / c < 8) break;
      const int n = ntiles * c;
      const int rounds = (n + 255) / 256;
      const int st_per = (kst + c - 1) / c;
      double t = rounds * (double)st_per * 2.0e-6;
      if (c > 1) t += (double)P * Q * 4.0 * (2 * c + 1) / 4.0e12;
      if (t < best_t * 0.98) {
        best_t = t;
        best = c;
      }
    }
    const int st_per = std::max((kst + best - 1) / best, 1);  // (M = 0: no slice, nothing to launch)
    p.slice = st_per * kPlanKTile;
    p.S = (kst + st_per - 1) / st_per;
  }
  // hybrid plan: with more tiles than workgroups, whole tiles for the whole rounds of the grid and the
  // remaining tiles as slices (>= 2 K-tiles each); it does not apply with no more tiles than
  // workgroups (the uniform slices above).  The remainder's slice count comes from the cost model above
  // (rounds x K-tiles per slice x ~2 us, plus the tile pieces written and read back at ~4 TB/s) instead of
  // "one round of slices" (ctas / rem): llama's gate/up projection (344 tiles on 256 CUs, 88 left) takes 5
  // slices in 2 rounds (1.4 tile times) instead of 2 slices in 1 round (1.5) (profiles/r6_wgrad_hy_cost.log)
  if (s.wgrad_hy && s.wgrad_pp && out_f32 && !bias && ctas < (1 << 29) && M % kPlanKTile == 0 && kst >= 2 &&
      ntiles > ctas) {
    p.arm = 3;
    p.hy_full = ntiles / ctas * ctas;
    p.hy_rem = ntiles - p.hy_full;
    int c_best = p.hy_rem > 0 ? std::max(1, std::min(ctas / p.hy_rem, kst / 2)) : 1;
    if (p.hy_rem > 0 && s.wgrad_hy_cost) {
      double best_t = 1e30;
      for (int c = 1; c <= 16 && (c == 1 || kst / c >= 8); ++c) {
        const int per = (kst + c - 1) / c;
        const int rounds = (p.hy_rem * c + ctas - 1) / ctas;
        const double t = rounds * (double)per * 2.0e-6 +
                         (c > 1 ? (double)p.hy_rem * c * kPlanTile * kPlanTile * 4.0 * 2 / 4.0e12 : 0.0);
        if (t < best_t * 0.98) {
          best_t = t;
          c_best = c;
        }
      }
    }
    p.hy_slice_kt = (kst + c_best - 1) / c_best;
    p.hy_s = p.hy_rem > 0 ? (kst + p.hy_slice_kt - 1) / p.hy_slice_kt : 0;
    p.ws_floats = (int64_t)p.hy_rem * p.hy_s * kPlanTile * kPlanTile;
    p.grid = plan_grid(p.hy_full + (int64_t)p.hy_rem * p.hy_s, ctas);
    return p;
  }
  // the ping-pong kernel: fp32 targets, whole K-tiles, >= 2 K-tiles per slice (the first K-tile is peeled)
  const bool pp_ok = M % kPlanKTile == 0 && p.slice % kPlanKTile == 0 && p.slice / kPlanKTile >= 2 && p.S >= 1;
  if (s.wgrad_pp && out_f32 && pp_ok) p.arm = 2;
  else p.arm = (s.wgrad_mfma != 0 ? s.wgrad_mfma : (P >= 16384 ? 32 : 16)) == 16 ? 0 : 1;
  const int64_t items = (int64_t)ntiles * p.S;
  p.grid = p.arm == 2 ? plan_grid(items, ctas) : (int)items;
  p.ws_floats = p.S > 1 ? (int64_t)p.S * P * Q : 0;
  p.bias_rows = bias ? p.S : 0;
  // the bias gradient rides along on the ping-pong kernel and the 16x16x32 one-barrier kernel (see wgrad_kernel)
  p.fused_bias = bias && p.arm != 1;
  return p;
}

// ---------------------------------------------------------------- grouped wgrad
// Whole tiles of several queued weight gradients in one launch of the ping-pong kernel (wgrad_pp.hip's
// grouped arm).  The queue is a list of problems in arrival order; its global tile list numbers every
// problem's tiles row band by row band.  One launch runs a contiguous range of that list; what it leaves
// stays queued for the next launch, or -- at the end of a backward -- goes to wgrad_plan one problem at a
// time (slices, slabs and reduces as for an immediate call).
constexpr int kWgradGroupMax = 16;  // problems one launch carries in its kernel argument

struct WgradGroupPlan {
  int take;  // tiles to launch now, counted from the head of the queue (0: keep waiting)
  int grid;  // workgroups of that launch
};

// tiles[i] / tiles_q[i]: tile count and tiles per row band of queued problem i (n problems); done0: tiles of
// problem 0 that an earlier launch ran (a multiple of tiles_q[0]).  The launch takes the whole rounds of the
// grid -- ctas workgroups, the CUs less reserve_cus whether the grid is persistent or one workgroup per tile --
// that the queue holds.  A cut inside a problem moves down to its last row-band boundary, so the part left
// over is a [rows, Q] problem of its own for wgrad_plan (and a row band's bias column sums are complete in the
// launch that runs it); a launch carries at most kWgradGroupMax problems.
inline WgradGroupPlan wgrad_group_plan(const GemmSettings& s, int cus, const int* tiles, const int* tiles_q, int n,
                                       int done0) {
  WgradGroupPlan g{0, 0};
  const int ctas = cus - s.reserve_cus > 8 ? cus - s.reserve_cus : 8;
  int64_t total = -(int64_t)done0;
  for (int i = 0; i < n; ++i) total += tiles[i];
  if (!s.wgrad_pp || total < ctas) return g;
  const int64_t want = total / ctas * ctas;
  int64_t take = 0;
  for (int i = 0; i < n && i < kWgradGroupMax && take < want; ++i) {
    const int off = i == 0 ? done0 : 0;
    const int64_t have = tiles[i] - off;
    if (take + have <= want) {
      take += have;
    } else {
      take += (want - take) / tiles_q[i] * tiles_q[i];
      break;
    }
  }
  g.take = (int)take;
  g.grid = s.persistent ? (int)std::min<int64_t>(take, ctas) : (int)take;
  return g;
}

}  // namespace pllm
