// Per-row FP8 (OCP e4m3fn) weight quantiser of the weight-only FP8 decode path (gfx950).
//
// For every row n of a bf16 matrix w[N, K]:
//   amax_n  = max_k |w_nk|                        (exact: bf16 is exact in fp32)
//   scale_n = amax_n / 448, or 1 when amax_n == 0 (one IEEE fp32 division)
//   q_nk    = e4m3fn(w_nk / scale_n)              (a true division, then v_cvt_pk_fp8_f32: nearest, ties to even)
// |w_nk / scale_n| <= 448 (1 + 2^-23), which rounds to 448, so the NaN codes 0x7f / 0xff never appear.
// It runs once when decode weights are prepared: one workgroup per row, two passes over the row (the second
// hits L2), element-wise loads so that any K and any 2-B aligned row stride is accepted.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int QT = 256;

__global__ __launch_bounds__(QT) void quantize_rows_fp8_kernel(const uint16_t* __restrict__ w, int64_t ldw,
                                                               uint8_t* __restrict__ q, float* __restrict__ scale,
                                                               int K) {
  __shared__ float red[QT / 64];
  const int n = blockIdx.x;
  const uint16_t* __restrict__ row = w + (int64_t)n * ldw;
  uint8_t* __restrict__ out = q + (int64_t)n * K;
  float amax = 0.f;
  for (int k = threadIdx.x; k < K; k += QT) amax = fmaxf(amax, fabsf(bf2f(row[k])));
  amax = block_max<QT / 64>(amax, red);
  const float sc = amax == 0.f ? 1.f : amax / 448.f;
  if (threadIdx.x == 0) scale[n] = sc;
  for (int k = threadIdx.x; k < K; k += QT) {
    const float t = bf2f(row[k]) / sc;
    out[k] = (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(t, 0.f, 0, false) & 0xff);
  }
}

}  // namespace

namespace pllm {

void quantize_rows_fp8(const uint16_t* w, int64_t ldw, uint8_t* q, float* scale, int N, int K, hipStream_t st) {
  if (N <= 0) return;
  hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3(N), dim3(QT), 0, st, w, ldw, q, scale, K);
  PL_CHECK_LAUNCH();
}

}  // namespace pllm
