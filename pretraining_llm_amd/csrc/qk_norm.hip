// QK-norm (gfx950): RMSNorm over the head dimension of every query and key head of a packed qkv row
// [rows, (H + 2 Hkv) D], one learned gain vector of D for q and one for k, applied before RoPE.
//
// * forward  -- replaces the attention's RoPE pre-pass (rope_kernel, elementwise.hip): reads the q / k heads,
//               normalises (fp32: r = rsqrt(mean(x^2) + eps), y = x r gamma), optionally rotates (rotate-half,
//               position row % T + pos_offset) and writes the [rows, (H + Hkv) D] buffer the attention kernels
//               read, rounding to bf16 once; r goes to rstd fp32 [rows, H + Hkv].  v is not copied.
// * backward -- one streaming post-pass over the q / k columns of the packed dqkv, in place: the attention
//               backward left dy there (gradient of the normalised, un-rotated heads);
//               x_hat = x r, g = dy gamma, c = mean(g x_hat), dx = r (g - x_hat c); dgamma = sum dy x_hat.
//
// Work mapping of both (as rope_kernel): one thread holds a 16-B chunk of the low half of a head and the
// matching chunk of the high half -- the RoPE partners -- so a head is D/16 = 2 / 4 / 8 neighbouring lanes of
// one wave and the row sums finish with 1 / 2 / 3 cross-lane adds (head_sum).  The forward runs a full grid (one chunk
// pair per thread, see the grid note in elementwise.hip).  The backward needs per-workgroup gain partials,
// so its grid is capped (qk_norm_bwd_grid) and every workgroup walks its items in a fixed order; the
// partials [G, D] per gain are reduced in fixed order by col_reduce (norm.hip): no float atomics, two calls
// on the same inputs give the same bits.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kBwdGridCap = 512;  // as the norm backward for rows <= 1,024 elements (norm_bwd_grid)

// sum over the HV = D/16 lanes of a head (aligned groups of 2 / 4 / 8 lanes of one wave), every lane getting
// the total: the xor-butterfly (lane ^ 1, lane ^ 2, then the group's other quad -- whose four lanes all hold
// the same quad sum) as DPP moves inside the VALU instead of __shfl_xor's ds_bpermute round trips through the
// LDS crossbar, which sit between a thread's only loads and its only stores
template <int CTRL>
PL_DEV float dpp_move(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int HV>
PL_DEV float head_sum(float v) {
  v += dpp_move<0xB1>(v);                          // quad_perm [1, 0, 3, 2]: lane ^ 1
  if constexpr (HV >= 4) v += dpp_move<0x4E>(v);   // quad_perm [2, 3, 0, 1]: lane ^ 2
  if constexpr (HV >= 8) v += dpp_move<0x141>(v);  // row_half_mirror: lane 7 - i of the 8, in the other quad
  return v;
}

template <int HV, bool ROPE>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(const uint16_t* __restrict__ qkv,
                                                           const uint16_t* __restrict__ wq,
                                                           const uint16_t* __restrict__ wk, uint16_t* __restrict__ qk,
                                                           float* __restrict__ rstd, const float* __restrict__ cosb,
                                                           const float* __restrict__ sinb, size_t rows, int T, int H,
                                                           int Hkv, int pos_offset, float eps) {
  constexpr int D = HV * 16, half = D / 2;
  const int NH = H + Hkv;
  const size_t W = (size_t)(H + 2 * Hkv) * D, WO = (size_t)NH * D;
  const size_t nwork = rows * NH * HV;
  const size_t stride = (size_t)gridDim.x * blockDim.x;  // a multiple of HV: a head's lanes stay together
  for (size_t base = blockIdx.x * (size_t)blockDim.x; base < nwork; base += stride) {
    const size_t i = base + threadIdx.x;
    const bool on = i < nwork;  // whole heads at a time (nwork % HV == 0); idle lanes still take the shuffles
    const int g = (int)(i % HV);
    const size_t rh = on ? i / HV : 0;
    const int h = (int)(rh % NH);
    const size_t r = rh / NH;
    const uint16_t* src = qkv + r * W + (size_t)h * D + g * 8;
    const uint16_t* gam = (h < H ? wq : wk) + g * 8;
    float a[8], b[8], wa[8], wb[8];
    unpack8(ld16(src), a);
    unpack8(ld16(src + half), b);
    unpack8(ld16(gam), wa);
    unpack8(ld16(gam + half), wb);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += a[j] * a[j] + b[j] * b[j];
    ss = head_sum<HV>(ss);
    const float rs = rsqrtf(ss * (1.f / D) + eps);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = a[j] * rs * wa[j];
      b[j] = b[j] * rs * wb[j];
    }
    if (ROPE) {
      const int t = (int)(r % T) + pos_offset;
      const f32x4* cp = reinterpret_cast<const f32x4*>(cosb + (size_t)t * half + g * 8);
      const f32x4* sp = reinterpret_cast<const f32x4*>(sinb + (size_t)t * half + g * 8);
      const f32x4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = j < 4 ? c0[j & 3] : c1[j & 3], s = j < 4 ? s0[j & 3] : s1[j & 3];
        const float x1 = a[j], x2 = b[j];
        a[j] = x1 * c - x2 * s;
        b[j] = x2 * c + x1 * s;
      }
    }
    if (on) {
      uint16_t* dst = qk + r * WO + (size_t)h * D + g * 8;
      st16(dst, pack8(a));
      st16(dst + half, pack8(b));
      if (g == 0) rstd[rh] = rs;
    }
  }
}

// part: fp32 [2][gridDim.x][D] (q gains, then k gains)
template <int HV>
__global__ __launch_bounds__(256) void qk_norm_bwd_kernel(uint16_t* __restrict__ dqkv,
                                                          const uint16_t* __restrict__ qkv,
                                                          const float* __restrict__ rstd,
                                                          const uint16_t* __restrict__ wq,
                                                          const uint16_t* __restrict__ wk, size_t rows, int H, int Hkv,
                                                          float* __restrict__ part) {
  constexpr int D = HV * 16, half = D / 2;
  __shared__ float red[4][HV][32];
  const int NH = H + Hkv;
  const size_t W = (size_t)(H + 2 * Hkv) * D;
  const size_t nwork = rows * NH * HV;
  const size_t stride = (size_t)gridDim.x * blockDim.x;  // a multiple of 256: a thread keeps its chunk g
  const int g = threadIdx.x % HV;
  float gq[16], gk[16];  // this thread's gains: low chunk, then high chunk
  unpack8(ld16(wq + g * 8), gq);
  unpack8(ld16(wq + half + g * 8), gq + 8);
  unpack8(ld16(wk + g * 8), gk);
  unpack8(ld16(wk + half + g * 8), gk + 8);
  float aq[16], ak[16];  // sum of dy x_hat over this thread's q / k items
#pragma unroll
  for (int j = 0; j < 16; ++j) aq[j] = ak[j] = 0.f;
  for (size_t base = blockIdx.x * (size_t)blockDim.x; base < nwork; base += stride) {
    const size_t i = base + threadIdx.x;
    const bool on = i < nwork;
    const size_t rh = on ? i / HV : 0;
    const int h = (int)(rh % NH);
    const size_t r = rh / NH;
    const bool isq = h < H;
    const size_t off = r * W + (size_t)h * D + g * 8;
    float x[16], dy[16];
    unpack8(ld16(qkv + off), x);
    unpack8(ld16(qkv + off + half), x + 8);
    unpack8(ld16(dqkv + off), dy);
    unpack8(ld16(dqkv + off + half), dy + 8);
    const float rs = rstd[rh];
    float gv[16], dot = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      x[j] *= rs;  // x_hat
      gv[j] = dy[j] * (isq ? gq[j] : gk[j]);
      dot += gv[j] * x[j];
    }
    const float c = head_sum<HV>(dot) * (1.f / D);
    if (on) {
      float dx[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        dx[j] = rs * (gv[j] - x[j] * c);
        const float t = dy[j] * x[j];
        aq[j] += isq ? t : 0.f;
        ak[j] += isq ? 0.f : t;
      }
      st16(dqkv + off, pack8(dx));
      st16(dqkv + off + half, pack8(dx + 8));
    }
  }
  // workgroup partial: the lanes of a wave that hold the same chunk (fixed shuffle order), then the 4 waves
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
#pragma unroll
    for (int o = 32; o >= HV; o >>= 1) {
      aq[j] += __shfl_xor(aq[j], o, 64);
      ak[j] += __shfl_xor(ak[j], o, 64);
    }
  }
  if (lane < HV) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      red[w][lane][j] = aq[j];
      red[w][lane][16 + j] = ak[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * D) {
    const int which = threadIdx.x / D, d = threadIdx.x % D;
    const int hi = d >= half, dd = d - hi * half;
    const int cg = dd >> 3, j = which * 16 + hi * 8 + (dd & 7);
    part[((size_t)which * gridDim.x + blockIdx.x) * D + d] =
        (red[0][cg][j] + red[1][cg][j]) + (red[2][cg][j] + red[3][cg][j]);
  }
}

}  // namespace

namespace pllm {

void qk_norm_rope(const void* qkv, const void* wq, const void* wk, void* qk, float* rstd, const float* cosb,
                  const float* sinb, size_t rows, int T, int H, int Hkv, int D, int pos_offset, float eps,
                  hipStream_t st) {
  const size_t nwork = rows * (size_t)(H + Hkv) * (D / 16);
  const size_t gb = (nwork + 255) / 256;
  const dim3 grid((unsigned)(gb < (1u << 30) ? gb : (1u << 30)));
#define L(HV)                                                                                                      \
  do {                                                                                                             \
    if (cosb)                                                                                                      \
      hipLaunchKernelGGL((qk_norm_rope_kernel<HV, true>), grid, dim3(256), 0, st, (const uint16_t*)qkv,           \
                         (const uint16_t*)wq, (const uint16_t*)wk, (uint16_t*)qk, rstd, cosb, sinb, rows, T, H,   \
                         Hkv, pos_offset, eps);                                                                    \
    else                                                                                                           \
      hipLaunchKernelGGL((qk_norm_rope_kernel<HV, false>), grid, dim3(256), 0, st, (const uint16_t*)qkv,          \
                         (const uint16_t*)wq, (const uint16_t*)wk, (uint16_t*)qk, rstd, cosb, sinb, rows, T, H,   \
                         Hkv, pos_offset, eps);                                                                    \
  } while (0)
  if (D == 32) L(2);
  else if (D == 64) L(4);
  else L(8);
#undef L
}

int qk_norm_bwd_grid(size_t rows, int H, int Hkv, int D) {
  const size_t gb = (rows * (size_t)(H + Hkv) * (D / 16) + 255) / 256;
  return (int)(gb < (size_t)kBwdGridCap ? (gb > 0 ? gb : 1) : kBwdGridCap);
}

void qk_norm_bwd(void* dqkv, const void* qkv, const float* rstd, const void* wq, const void* wk, size_t rows, int H,
                 int Hkv, int D, float* part, void* dwq, void* dwk, bool grad_f32, bool accumulate, hipStream_t st) {
  const int G = qk_norm_bwd_grid(rows, H, Hkv, D);
#define L(HV)                                                                                              \
  hipLaunchKernelGGL(qk_norm_bwd_kernel<HV>, dim3(G), dim3(256), 0, st, (uint16_t*)dqkv, (const uint16_t*)qkv, \
                     rstd, (const uint16_t*)wq, (const uint16_t*)wk, rows, H, Hkv, part)
  if (D == 32) L(2);
  else if (D == 64) L(4);
  else L(8);
#undef L
  col_reduce(part, G, D, dwq, grad_f32, accumulate, st);
  col_reduce(part + (size_t)G * D, G, D, dwk, grad_f32, accumulate, st);
}

}  // namespace pllm
