// Fused per-row temperature / top-k / top-p / min-p sampling for the serving path (gfx950).
//
// One workgroup per row of logits [B, V]; every sampler parameter of the row is read from
// device memory, so one launch serves any mix of samplers and can sit in a captured hipGraph.
// With z_i = x_i / T over the row's VALID entries (not NaN, not -inf):
//   * T <= 0: lowest-index argmax, filters ignored, the kept set is every valid entry;
//   * every filter is a VALUE threshold, so ties stay together:
//       top-k  (0 < k < #valid, else off): z >= the k-th largest valid value;
//       top-p  (p < 1, clamped to [0, 1]; on the top-k survivors of mass M, w_i = exp(z_i - z_max)):
//              z >= t, t the largest value with mass{z >= t} >= p * M (p = 0: the maximum's ties);
//       min-p  (> 0): z >= z_max + ln(min_p)  (min_p >= 1: the maximum's ties);
//     the kept set is z >= the largest of the three thresholds;
//   * the token is the Gumbel-max over the kept set.  The uniform of entry i is a counter-based
//     hash of (seed[row], step[row], i) alone: not of the row index, the batch size or the
//     filters.  So a row draws the same token wherever it sits in any batch, and a filtered draw
//     equals the unfiltered one whenever that one lies inside the kept set.
// Outputs per row: the token, the size of the kept set and its smallest raw logit (+inf and 0
// for a row without a valid entry, whose token is 0).  A row holding +inf logits only promises
// an in-range token: its weights exp(z - z_max) are not meaningful.
//
// Rows with every filter off take ONE pass (the sample_kernel loop: 16 loads in flight per
// thread) and leave by a workgroup-uniform branch.  Filtered rows find their threshold by a
// radix select over an order-preserving integer key of the RAW logit (16 key bits for bf16, 32
// for fp32; 11-bit digits, one LDS histogram per digit, the row re-read from L2 per digit with
// 16-byte loads where it is aligned): element counts for top-k, then masses for top-p.  Masses
// are summed as 64-bit fixed point (scale 2^40; V * 2^40 < 2^64) with integer LDS atomics, so
// the kept set does not depend on the order in which the adds arrive and is bitwise
// reproducible.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NT = 1024;         // threads per row
constexpr int NW = NT / 64;      // waves per row
constexpr int SU = 16;           // loads in flight per thread
constexpr int DIGIT = 11;        // radix-select digit width
constexpr int NBIN = 1 << DIGIT; // 2 bins per thread
constexpr float FIX = 1099511627776.f;  // 2^40

PL_DEV uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// (value, index) argmax with lowest-index tie break
PL_DEV void better(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

template <typename T>
PL_DEV float load_logit(const T* p, int64_t i);
template <>
PL_DEV float load_logit<float>(const float* p, int64_t i) { return p[i]; }
template <>
PL_DEV float load_logit<uint16_t>(const uint16_t* p, int64_t i) { return bf2f(p[i]); }

PL_DEV bool valid(float x) { return x == x && x != -INFINITY; }

// order-preserving key of a valid logit in KB bits (-0 and +0 share a key)
template <int KB>
PL_DEV uint32_t key_of(float x) {
  if (x == 0.f) x = 0.f;
  const uint32_t b = __float_as_uint(x);
  return (b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u)) >> (32 - KB);
}

// f(x_i, i) over the row with SU independent loads in flight per thread; the padding past V
// arrives as NaN, which no caller counts
template <typename T, typename F>
PL_DEV void sweep(const T* __restrict__ x, int V, F f) {
  for (uint32_t i0 = threadIdx.x; i0 < (uint32_t)V; i0 += NT * SU) {  // unsigned: no wrap for V < 2^31
    float v[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const uint32_t i = i0 + u * NT;
      v[u] = i < (uint32_t)V ? load_logit<T>(x, i) : NAN;
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) f(v[u], (int)(i0 + u * NT));
  }
}

// The same over a 16-byte aligned row with 16-byte loads, VU in flight per thread: the selection passes do little
// arithmetic per element, so their time is the number of load round trips (4 per pass over 50,304 fp32 logits with
// the dword loop above, 2 with this one).  Only whole vectors are loaded (nothing is read past the row's end); the
// last V % (16 / sizeof(T)) entries go through scalar loads.  Entries arrive in another order than in sweep(), which
// no caller can tell: counts, integer sums, min / max and the lowest-index argmax do not depend on it.
template <typename T, typename F>
PL_DEV void sweep_vec(const T* __restrict__ x, int V, F f) {
  constexpr int VE = 16 / sizeof(T);
  constexpr int VU = 8;
  const uint32_t nan = sizeof(T) == 2 ? 0x7fc07fc0u : 0x7fc00000u;
  const uint32_t nvec = (uint32_t)V / VE;
  for (uint32_t v0 = threadIdx.x; v0 < nvec; v0 += NT * VU) {
    u32x4 r[VU];
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const uint32_t vi = v0 + u * NT;
      r[u] = vi < nvec ? ld16(x + (int64_t)vi * VE) : u32x4{nan, nan, nan, nan};
    }
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int i = (int)((v0 + u * NT) * VE);
      if constexpr (sizeof(T) == 2) {
        float e[8];
        unpack8(r[u], e);
#pragma unroll
        for (int j = 0; j < 8; ++j) f(e[j], i + j);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) f(__uint_as_float(r[u][j]), i + j);
      }
    }
  }
  const uint32_t t = nvec * VE + threadIdx.x;
  if (t < (uint32_t)V) f(load_logit<T>(x, t), t);
}

template <typename T, typename F>
PL_DEV void sweep_any(bool vec, const T* __restrict__ x, int V, F f) {
  if (vec) sweep_vec<T>(x, V, f);
  else sweep<T>(x, V, f);
}

struct Shared {
  unsigned long long hist[NBIN];
  unsigned long long wtot[NW];
  unsigned long long sel_rem;
  uint32_t sel_digit;
  float rv[NW];
  float rm[NW];
  int ri[NW];
  int rc[NW];
};

// One radix select over the entries with key >= floor_key.  MASS = false: the key of the
// `target`-th largest entry (1 <= target <= their number).  MASS = true: the largest key t with
// mass{key >= t} >= frac * (mass of all of them), at least one fixed-point unit.
template <typename T, int KB, bool MASS>
PL_DEV uint32_t radix_select(Shared& sh, bool vec, const T* __restrict__ x, int V, uint32_t floor_key,
                             unsigned long long target, float frac, float inv_t, float zmax) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t prefix = 0;
  int rem_bits = KB;
  while (rem_bits > 0) {
    const int width = rem_bits < DIGIT ? rem_bits : DIGIT;
    const int shift = rem_bits - width;
    const bool first = rem_bits == KB;
    sh.hist[2 * tid] = 0;
    sh.hist[2 * tid + 1] = 0;
    if (tid == 0) {  // what a scan that finds no digit leaves behind: the lowest digit
      sh.sel_digit = 0;
      sh.sel_rem = 1;
    }
    __syncthreads();
    sweep_any<T>(vec, x, V, [&](float xi, int) {
      if (!valid(xi)) return;
      const uint32_t key = key_of<KB>(xi);
      if (key < floor_key) return;
      if (!first && (key >> rem_bits) != (prefix >> rem_bits)) return;
      unsigned long long add = 1;
      if (MASS) add = (unsigned long long)(__expf(xi * inv_t - zmax) * FIX);
      atomicAdd(&sh.hist[(key >> shift) & ((1u << width) - 1)], add);
    });
    __syncthreads();
    // suffix sums over the digits: this thread owns bins 2 tid and 2 tid + 1
    const unsigned long long a = sh.hist[2 * tid], b = sh.hist[2 * tid + 1];
    unsigned long long incl = a + b;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long up = __shfl_down(incl, o, 64);
      if (lane + o < 64) incl += up;
    }
    if (lane == 0) sh.wtot[w] = incl;
    __syncthreads();
    unsigned long long above = 0, total = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const unsigned long long t = sh.wtot[k];
      total += t;
      if (k > w) above += t;
    }
    if (MASS && first) {
      target = (unsigned long long)((double)total * (double)frac);
      if (target < 1) target = 1;
    }
    above += incl - (a + b);  // entries in the bins above 2 tid + 1
    if (above < target) {
      if (above + b >= target) {
        sh.sel_digit = 2 * tid + 1;
        sh.sel_rem = target - above;
      } else if (above + b + a >= target) {
        sh.sel_digit = 2 * tid;
        sh.sel_rem = target - above - b;
      }
    }
    __syncthreads();
    prefix |= sh.sel_digit << shift;
    target = sh.sel_rem;
    rem_bits = shift;
    __syncthreads();  // sel_* and hist are rewritten by the next digit
  }
  return prefix;
}

template <typename T>
__global__ __launch_bounds__(NT) void sample_rows_kernel(const T* __restrict__ logits, int64_t ld, int V,
                                                         const float* __restrict__ temperature,
                                                         const int* __restrict__ top_k,
                                                         const float* __restrict__ top_p,
                                                         const float* __restrict__ min_p,
                                                         const int64_t* __restrict__ seed,
                                                         const int64_t* __restrict__ step,
                                                         int64_t* __restrict__ tokens, int* __restrict__ kept,
                                                         float* __restrict__ min_kept) {
  constexpr int KB = sizeof(T) == 2 ? 16 : 32;
  __shared__ Shared sh;
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const T* x = logits + row * ld;
  const float temp = temperature[row];
  const int k = top_k[row];
  float p = top_p[row];
  float mp = min_p[row];
  const bool greedy = !(temp > 0.f);
  const float inv_t = greedy ? 1.f : 1.f / temp;
  const bool use_p = p < 1.f;
  const bool use_mp = mp > 0.f;
  const bool filtered = !greedy && (k > 0 || use_p || use_mp);
  const bool vec = filtered && ((uintptr_t)x & 15) == 0;  // workgroup-uniform, like every branch on a parameter
  p = fmaxf(p, 0.f);
  mp = fminf(mp, 1.f);
  // the uniforms' key: (seed, step) of the row, nothing else
  const uint64_t rkey = mix64(mix64((uint64_t)seed[row] + 0x9e3779b97f4a7c15ull) ^
                              ((uint64_t)step[row] * 0xd1342543de82ef95ull + 0x2545f4914f6cdd1dull));
  auto gumbel = [&](float xi, int i) {
    const uint64_t h = mix64(rkey + (uint64_t)i);
    const float uu = ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);  // (0, 1)
    return xi * inv_t - __logf(-__logf(uu));
  };

  float best = -INFINITY, mn = INFINITY;
  int bi = 0x7fffffff, cnt = 0;
  uint32_t tkey = 0;
  float zthr = -INFINITY;

  if (filtered) {
    // pass 1: the maximum and the number of valid entries
    float xmax = -INFINITY;
    sweep_any<T>(vec, x, V, [&](float xi, int) {
      if (!valid(xi)) return;
      xmax = fmaxf(xmax, xi);
      ++cnt;
    });
    xmax = wave_max(xmax);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) {
      sh.rv[w] = xmax;
      sh.rc[w] = cnt;
    }
    __syncthreads();
    xmax = -INFINITY;
    cnt = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      xmax = fmaxf(xmax, sh.rv[j]);
      cnt += sh.rc[j];
    }
    __syncthreads();
    if (cnt > 0) {  // (an empty row falls through to the last pass, which keeps nothing)
      const float zmax = xmax * inv_t;
      if (k > 0 && k < cnt) tkey = radix_select<T, KB, false>(sh, vec, x, V, 0u, (unsigned long long)k, 0.f, inv_t, zmax);
      if (use_p) tkey = radix_select<T, KB, true>(sh, vec, x, V, tkey, 0ull, p, inv_t, zmax);
      if (use_mp) zthr = zmax + __logf(mp);
    }
    cnt = 0;
  }

  // the draw over the kept set (the only pass of an unfiltered row, which takes sample_kernel's loop)
  sweep_any<T>(vec, x, V, [&](float xi, int i) {
    if (!valid(xi)) return;
    if (filtered && (key_of<KB>(xi) < tkey || xi * inv_t < zthr)) return;
    ++cnt;
    mn = fminf(mn, xi);
    better(best, bi, greedy ? xi : gumbel(xi, i), i);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(best, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    better(best, bi, v2, i2);
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) {
    sh.rv[w] = best;
    sh.ri[w] = bi;
    sh.rm[w] = mn;
    sh.rc[w] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < NW; ++j) {
      better(best, bi, sh.rv[j], sh.ri[j]);
      mn = fminf(mn, sh.rm[j]);
      cnt += sh.rc[j];
    }
    tokens[row] = bi < V ? bi : 0;  // no valid entry: token 0, kept 0, min_kept +inf
    kept[row] = cnt;
    min_kept[row] = mn;
  }
}

}  // namespace

namespace pllm {

void sample_rows(const void* logits, bool bf16_in, int64_t ld, int B, int V, const float* temperature,
                 const int* top_k, const float* top_p, const float* min_p, const int64_t* seed, const int64_t* step,
                 int64_t* tokens, int* kept, float* min_kept, hipStream_t st) {
  if (bf16_in)
    hipLaunchKernelGGL(sample_rows_kernel<uint16_t>, dim3(B), dim3(NT), 0, st, (const uint16_t*)logits, ld, V,
                       temperature, top_k, top_p, min_p, seed, step, tokens, kept, min_kept);
  else
    hipLaunchKernelGGL(sample_rows_kernel<float>, dim3(B), dim3(NT), 0, st, (const float*)logits, ld, V, temperature,
                       top_k, top_p, min_p, seed, step, tokens, kept, min_kept);
}

}  // namespace pllm
