// Gradient of the attention sinks (gfx950).
//
// A sink is one learned logit s[h] per query head that joins every softmax row's denominator and carries no
// value.  Its probability in row (b, h, t) is p = exp(s[h] - lse[b, h, t]); with a zero value row its dP is 0,
// so dS_sink = p (0 - delta) with delta = rowsum(dO O), the row constant the backward kernels already use:
//   ds[h] = - sum_{b, t} exp(s[h] - lse[b, h, t]) delta[b, h, t].
// The flash backward kernels therefore run unchanged on the sink-inclusive lse; this file is the only new
// backward work: a streaming reduction over two fp32 [B, H, T] tensors.
//  * grid (G, H): the G workgroups of head h stride over the head's B x ceil((T + 3) / 4) 16-byte groups.  A row
//    [b, h, :] starts at element (b H + h) T, 16-B aligned only when that is a multiple of 4, so the groups are
//    laid on the aligned grid around the row: whole groups inside the row are one 16-B load each of lse and
//    delta, the (at most two) ragged groups at a row's ends go element by element;
//  * every thread sums its groups in fp32 in a fixed order, the workgroup combines its 4 waves through LDS in a
//    fixed order and writes one partial to part[g][h]; col_reduce (norm.hip) sums the G partials in a fixed
//    order into the bf16 / fp32 gradient (stored or added).  No float atomics: bitwise reproducible.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NT = 256;
constexpr int kMaxGrid = 32;  // workgroups per head

__global__ __launch_bounds__(NT) void attn_sink_bwd_kernel(const float* __restrict__ lse,
                                                           const float* __restrict__ delta,
                                                           const uint16_t* __restrict__ sinks, int B, int H, int T,
                                                           float* __restrict__ part) {
  __shared__ float scratch[NT / 64];
  const int h = blockIdx.y;
  constexpr float kLog2e = 1.4426950408889634f;
  const float s = bf2f(sinks[h]);
  const int nv = (T + 6) / 4;  // 16-B groups that can touch a row (misalignment up to 3 elements)
  const int64_t items = (int64_t)B * nv;
  float acc = 0.f;
  for (int64_t it = (int64_t)blockIdx.x * NT + threadIdx.x; it < items; it += (int64_t)gridDim.x * NT) {
    const int b = (int)(it / nv), v = (int)(it % nv);
    const int64_t e0 = ((int64_t)b * H + h) * T;  // first element of the row
    const int mis = (int)(e0 & 3);
    const int t0 = 4 * v - mis;  // the group's first row index (may be < 0 or reach past T)
    if (t0 >= 0 && t0 + 4 <= T) {
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse + e0 + t0);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta + e0 + t0);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc += fast_exp2((s - l4[i]) * kLog2e) * d4[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + i;
        if (t >= 0 && t < T) acc += fast_exp2((s - lse[e0 + t]) * kLog2e) * delta[e0 + t];
      }
    }
  }
  const float tot = block_sum<NT / 64>(acc, scratch);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.x * H + h] = -tot;
}

}  // namespace

namespace pllm {

int attn_sink_bwd_grid(int B, int T) {
  const int64_t items = (int64_t)B * ((T + 6) / 4);
  const int64_t g = (items + NT - 1) / NT;
  return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

void attn_sink_bwd(const float* lse, const float* delta, const void* sinks, int B, int H, int T, float* part,
                   void* out, bool out_f32, bool accumulate, hipStream_t st) {
  const int G = attn_sink_bwd_grid(B, T);
  hipLaunchKernelGGL(attn_sink_bwd_kernel, dim3(G, H), dim3(NT), 0, st, lse, delta, (const uint16_t*)sinks, B, H, T,
                     part);
  col_reduce(part, G, H, out, out_f32, accumulate, st);
  PL_CHECK_LAUNCH();
}

}  // namespace pllm
