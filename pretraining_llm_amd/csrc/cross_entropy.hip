// Fused softmax cross-entropy, forward + backward in one pass (gfx950).
//
// Reference: F.cross_entropy(logits.view(B*T, V), targets.view(B*T)) in fp32
// under autocast (src/models/transformer.py:72-77).  Here one workgroup of
// 512 threads owns one row of bf16 logits; the row (V = 50304 -> 98 KiB) stays
// in registers (CH chunks of 8 bf16 per lane), so the logits are read from HBM
// exactly once and, in training, overwritten in place by
//     dlogits = (softmax(x) - onehot(t)) * inv_n          (inv_n = 1 / #valid)
// so no probability tensor and no second logits-sized buffer ever exist.
//
// ce_aux_kernel is the same row pass (ce_row, MODE 1 / 2) with two options (op cross_entropy_aux):
//   final-logit soft-capping   y_i = cap * tanh(x_i / cap)   (fp32 from the bf16 x_i, never rounded back; cap 0: y = x)
//   auxiliary z-loss           loss = (lse - y_t) + z * lse^2,   lse = logsumexp(y)
//   dx_i = (p_i (1 + 2 z lse) - [i == t]) * inv_n * (1 - (y_i / cap)^2),   p_i = exp(y_i - lse)
// tanh is recomputed from the packed bf16 row in the sum and the output pass (the row stays at 4 VGPRs per
// 8 logits); it is monotone, so the max pass runs on x and only each lane's maximum is transformed.
// ce_kernel (MODE 0) compiles to the code it had before the options existed (profiles/z_loss.md).
#include <cstdlib>

#include "ab.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int CE_THREADS = 512;
// each lane's (max, exp-sum) pair merged in ONE block reduction (2 barriers per row instead of 5 for
// separate max / sum reductions): 2,524 vs 2,551 us at 65536 x 50304 (bench/ce_bench.py, round 4)

// tanh(u) as 1 - q, q = 2 / (exp2(2 u log2 e) + 1) in [0, 2]: NaN-free at u = +-inf (q = 0 / 2); absolute error
// about one fp32 ulp of 1.  Returns q; 1 - tanh^2 = q (2 - q).
PL_DEV float ce_tanh_q(float x, float k2) { return 2.f * __builtin_amdgcn_rcpf(fast_exp2(x * k2) + 1.f); }
PL_DEV float ce_cap(float x, float k2, float cap) { return __builtin_fmaf(-cap, ce_tanh_q(x, k2), cap); }

// MODE 0: plain; 1: z-loss and the lse output; 2: those and the soft-cap (cap > 0).  A template parameter, not a
// branch on cap: the z-only kernel carries no tanh code (at CH = 32 the unrolled row pass with both forms in it ran
// 3 % behind the plain kernel, 900 vs 871 us at 8192 x 128256; profiles/z_loss.md).
template <int CH, bool WRITE_GRAD, int CE_THREADS, bool NTS, int MODE>
PL_DEV void ce_row(const uint16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ targets, int V,
                   int ignore_index, float* __restrict__ loss, uint16_t* __restrict__ dlogits,
                   const float* __restrict__ inv_n, float z, float cap, float* __restrict__ lse_out) {
  // The row is held PACKED (bf16, 4 VGPRs per 8 logits) so a 512-thread block needs ~52
  // VGPRs for V = 50304 and several blocks fit per CU; exp2 is recomputed in the output
  // pass instead of being stored (VALU is idle in this HBM-bound kernel).
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr bool AUX = MODE > 0;
  constexpr bool capped = MODE == 2;
  constexpr int CE_WAVES = CE_THREADS / 64;
  __shared__ float scratch[3 * CE_WAVES];
  const int row = blockIdx.x;
  const uint16_t* x = logits + (size_t)row * ld;
  const int nch = V >> 3;
  u32x4 v[CH];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + CE_THREADS * k;
#ifndef PL_CE_NTL
#define PL_CE_NTL 1
#endif
    // non-temporal loads of the once-read logits: 2,370 vs 2,490 us at 65536 x 50304, 3 interleaved rounds
    // (profiles/r6_ce_nt_loads.log)
    if (PL_CE_NTL)
      v[k] = c < nch ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + c * 8))
                     : u32x4{0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};
    else
      v[k] = c < nch ? ld16(x + c * 8) : u32x4{0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};  // -inf
  }
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    float f[8];
    unpack8(v[k], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, f[j]);
  }
  // scalar tail when V % 8 != 0
  const int tail0 = nch * 8;
  float tv = -INFINITY;
  const int tj = tail0 + threadIdx.x;
  if (tj < V) {
    tv = bf2f(x[tj]);
    m = fmaxf(m, tv);
  }
  const int64_t t = targets[row];
  const bool valid = t != (int64_t)ignore_index && t >= 0 && t < V;
  // soft-cap: y = cap (1 - q(x k2)), k2 = 2 log2(e) / cap
  const float k2 = capped ? 2.f * LOG2E / cap : 0.f;
  float mc, s;
  float lse = 0.f;  // AUX: the row's log-sum-exp of y, in every lane
  {
    // the lane's own max, its exp-sum against it, then ONE block reduction of (max, sum) pairs
    // (2 barriers instead of 4; the target logit is read before any lane can overwrite it)
    float xt = (threadIdx.x == 0 && valid) ? bf2f(x[t]) : 0.f;
    if constexpr (capped) {  // (a lane with no element, or -inf only, starts from -cap: finite, <= the row's maximum)
      xt = ce_cap(xt, k2, cap);
      m = ce_cap(m, k2, cap);
    }
    // ms: the lane's maximum times log2(e), rounded ONCE.  Every exp-sum is taken against such a rounded value,
    // so rebasing a sum from one maximum to another multiplies it by 2^(difference of two of them).  The merges
    // carry ms itself (its maximum is the scaled maximum): written `m * LOG2E - c`, the compiler contracts the
    // rebase into fma(m, LOG2E, -c), which is off by the product's rounding residual (up to 2^-18 at |m| = 80)
    // even for m's own c -- seven merges per row inflated the sum, and at a confident target softmax - 1 came
    // out as 1e-5 instead of 0.  The empty asm keeps the product from being folded into a later subtraction.
    float ms = m * LOG2E;
    asm volatile("" : "+v"(ms));
    const float ml = m == -INFINITY ? 0.f : ms;
#pragma unroll
    for (int k = 0; k < CH; ++k) asm volatile("" : "+v"(v[k]));
    float sl = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      float f[8];
      unpack8(v[k], f);
      if constexpr (capped) {  // the -inf padding past the row would count as -cap: skip it
        if (threadIdx.x + CE_THREADS * k >= nch) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = ce_cap(f[j], k2, cap);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) sl += fast_exp2(__builtin_fmaf(f[j], LOG2E, -ml));
    }
    if constexpr (capped) {
      if (tj < V) tv = ce_cap(tv, k2, cap);
    }
    if (tj < V) sl += fast_exp2(__builtin_fmaf(tv, LOG2E, -ml));
    // wave: pairwise (scaled max, sum) merge, then across waves through LDS
    const float ms0 = ms;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(ms, o, 64), s2 = __shfl_xor(sl, o, 64);
      const float mn = fmaxf(ms, m2);
      sl = (ms == -INFINITY ? 0.f : sl * fast_exp2(ms - mn)) + (m2 == -INFINITY ? 0.f : s2 * fast_exp2(m2 - mn));
      ms = mn;
    }
    // the plain maximum (for the loss) from a lane that holds it: the rounded product is monotone in m
    // (and distinct for distinct bf16 values)
    m = __shfl(m, __ffsll((unsigned long long)__ballot(ms0 == ms)) - 1, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (l == 0) {
      scratch[w] = m;
      scratch[CE_WAVES + w] = sl;
      scratch[2 * CE_WAVES + w] = ms;
    }
    __syncthreads();
    float mb = -INFINITY;
    mc = -INFINITY;
#pragma unroll
    for (int i = 0; i < CE_WAVES; ++i) {
      mb = fmaxf(mb, scratch[i]);
      mc = fmaxf(mc, scratch[2 * CE_WAVES + i]);
    }
    float sb = 0.f;
#pragma unroll
    for (int i = 0; i < CE_WAVES; ++i) {
      const float mi = scratch[2 * CE_WAVES + i];
      if (mi != -INFINITY) sb += scratch[CE_WAVES + i] * fast_exp2(mi - mc);
    }
    m = mb;
    s = sb;
#pragma unroll
    for (int k = 0; k < CH; ++k) asm volatile("" : "+v"(v[k]));
    if (threadIdx.x == 0) PL_DCHECK(t == (int64_t)ignore_index || (t >= 0 && t < V), "target in [0, vocab) or ignore_index", t);
    if constexpr (AUX) {
      lse = __logf(s) + m;
      if (threadIdx.x == 0) {
        loss[row] = valid ? __builtin_fmaf(z * lse, lse, lse - xt) : 0.f;
        if (lse_out) lse_out[row] = valid ? lse : 0.f;
      }
    } else {
      if (threadIdx.x == 0) loss[row] = valid ? (__logf(s) + m - xt) : 0.f;
    }
    if (!WRITE_GRAD) return;
    __syncthreads();  // lane 0's target-logit read (consumed by the loss above) precedes every store
  }
  const float in = *inv_n;
  float scale = valid ? in / s : 0.f;
  if constexpr (AUX) scale = valid ? scale * __builtin_fmaf(2.f * z, lse, 1.f) : 0.f;  // d(z lse^2) = 2 z lse p
  uint16_t* dx = dlogits + (size_t)row * ld;
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + CE_THREADS * k;
    if (c < nch) {
      float f[8];
      unpack8(v[k], f);
      float d[8];  // AUX, capped: dy/dx = 1 - tanh^2 = q (2 - q)
      if constexpr (capped) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float q = ce_tanh_q(f[j], k2);
          f[j] = __builtin_fmaf(-cap, q, cap);
          d[j] = q * (2.f - q);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = fast_exp2(__builtin_fmaf(f[j], LOG2E, -mc)) * scale;
      if (valid && (int)(t >> 3) == c) f[t & 7] -= in;
      if constexpr (capped) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] *= d[j];
      }
      if constexpr (NTS) __builtin_nontemporal_store(pack8(f), reinterpret_cast<u32x4*>(dx + c * 8));
      else st16(dx + c * 8, pack8(f));
    }
  }
  if (tj < V) {
    float o = fast_exp2(__builtin_fmaf(tv, LOG2E, -mc)) * scale;
    if (valid && tj == t) o -= in;
    if constexpr (capped) {  // tv holds y here: 1 - (y / cap)^2
      const float th = tv / cap;
      o *= __builtin_fmaf(-th, th, 1.f);
    }
    dx[tj] = f2bf_bits(o);
  }
}

// one row per block: stores of the gradient with the non-temporal hint when NTS (A/B)
template <int CH, bool WRITE_GRAD, int CE_THREADS = 512, bool NTS = false>
__global__ __launch_bounds__(CE_THREADS) void ce_kernel(const uint16_t* __restrict__ logits, int64_t ld,
                                                         const int64_t* __restrict__ targets, int V,
                                                         int ignore_index, float* __restrict__ loss,
                                                         uint16_t* __restrict__ dlogits, const float* __restrict__ inv_n) {
  ce_row<CH, WRITE_GRAD, CE_THREADS, NTS, 0>(logits, ld, targets, V, ignore_index, loss, dlogits, inv_n, 0.f, 0.f,
                                                 nullptr);
}

// the same with z-loss and / or the soft-cap; lse_out (optional): the row's log-sum-exp, 0 on ignored rows
template <int CH, bool WRITE_GRAD, bool CAP, int CE_THREADS = 512, bool NTS = false>
__global__ __launch_bounds__(CE_THREADS) void ce_aux_kernel(const uint16_t* __restrict__ logits, int64_t ld,
                                                             const int64_t* __restrict__ targets, int V,
                                                             int ignore_index, float* __restrict__ loss,
                                                             uint16_t* __restrict__ dlogits,
                                                             const float* __restrict__ inv_n, float z, float cap,
                                                             float* __restrict__ lse_out) {
  ce_row<CH, WRITE_GRAD, CE_THREADS, NTS, CAP ? 2 : 1>(logits, ld, targets, V, ignore_index, loss, dlogits, inv_n, z,
                                                       cap, lse_out);
}

}  // namespace

namespace pllm {

template <int NT, bool NTS, bool CAP>
void ce_aux_launch(const void* logits, int64_t ld, const int64_t* targets, int N, int V, int ignore_index, float* loss,
                   void* dlogits, const float* inv_n, float z, float cap, float* lse, hipStream_t st) {
  const int nch = V / 8;
  const int CH = (nch + NT - 1) / NT;
  const bool g = dlogits != nullptr;
#define L(C)                                                                                                       \
  do {                                                                                                             \
    if (g)                                                                                                         \
      hipLaunchKernelGGL((ce_aux_kernel<C, true, CAP, NT, NTS>), dim3(N), dim3(NT), 0, st, (const uint16_t*)logits, ld, \
                         targets, V, ignore_index, loss, (uint16_t*)dlogits, inv_n, z, cap, lse);                  \
    else                                                                                                           \
      hipLaunchKernelGGL((ce_aux_kernel<C, false, CAP, NT, NTS>), dim3(N), dim3(NT), 0, st, (const uint16_t*)logits, ld, \
                         targets, V, ignore_index, loss, (uint16_t*)nullptr, inv_n, z, cap, lse);                  \
  } while (0)
  if (CH <= 1) L(1);
  else if (CH <= 2) L(2);
  else if (CH <= 4) L(4);
  else if (CH <= 8) L(8);
  else if (CH <= 13) L(13);
  else if (CH <= 16) L(16);
  else L(32);
#undef L
}

void cross_entropy_aux(const void* logits, int64_t ld, const int64_t* targets, int N, int V, int ignore_index,
                       float* loss, void* dlogits, const float* inv_n, float z_loss, float softcap, float* lse,
                       hipStream_t st) {
  static const bool nts = pllm::ab_int("ce_nt", 1) != 0;  // as cross_entropy below
#define A(NTS, CAP)                                                                                                  \
  ce_aux_launch<CE_THREADS, NTS, CAP>(logits, ld, targets, N, V, ignore_index, loss, dlogits, inv_n, z_loss, softcap, \
                                      lse, st)
  if (softcap > 0.f) {
    if (nts) A(true, true);
    else A(false, true);
  } else {
    if (nts) A(true, false);
    else A(false, false);
  }
#undef A
}

template <int NT, bool NTS>
void ce_launch(const void* logits, int64_t ld, const int64_t* targets, int N, int V, int ignore_index, float* loss,
               void* dlogits, const float* inv_n, hipStream_t st) {
  const int nch = V / 8;
  const int CH = (nch + NT - 1) / NT;
  const bool g = dlogits != nullptr;
#define L(C)                                                                                               \
  do {                                                                                                     \
    if (g)                                                                                                 \
      hipLaunchKernelGGL((ce_kernel<C, true, NT, NTS>), dim3(N), dim3(NT), 0, st, (const uint16_t*)logits, ld, \
                         targets, V, ignore_index, loss, (uint16_t*)dlogits, inv_n);                       \
    else                                                                                                   \
      hipLaunchKernelGGL((ce_kernel<C, false, NT, NTS>), dim3(N), dim3(NT), 0, st, (const uint16_t*)logits, ld, \
                         targets, V, ignore_index, loss, (uint16_t*)nullptr, inv_n);                       \
  } while (0)
  if (CH <= 1) L(1);
  else if (CH <= 2) L(2);
  else if (CH <= 4) L(4);
  else if (CH <= 8) L(8);
  else if (CH <= 13) L(13);
  else if (CH <= 16) L(16);
  else L(32);
#undef L
}

void cross_entropy(const void* logits, int64_t ld, const int64_t* targets, int N, int V, int ignore_index,
                   float* loss, void* dlogits, const float* inv_n, hipStream_t st) {
  // non-temporal gradient stores: 2,493 vs 2,524 us at 65536 x 50304 (PLLM_AB=ce_nt=0: plain stores);
  // 256- / 1024-thread blocks measured 2,533 / 2,641 us (scripts/gpu/r4_ce2.sh, 3 interleaved rounds)
  static const bool nts = pllm::ab_int("ce_nt", 1) != 0;
  if (nts) ce_launch<CE_THREADS, true>(logits, ld, targets, N, V, ignore_index, loss, dlogits, inv_n, st);
  else ce_launch<CE_THREADS, false>(logits, ld, targets, N, V, ignore_index, loss, dlogits, inv_n, st);
}

// 32 chunks of 8 logits per lane.  The op takes V % 8 == 0 only, so the kernel's scalar tail never adds to that:
// with a "+ CE_THREADS" allowance here, V = 131080 .. 131584 were accepted, ran as CH = 32, and the vectors past
// 131072 were neither read nor written.
int cross_entropy_max_vocab() { return CE_THREADS * 8 * 32; }

}  // namespace pllm
